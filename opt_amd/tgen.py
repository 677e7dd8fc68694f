"""From a .t file to an energy plug-in: a translator for the subset of Opt's energy DSL that this project's own .t files use.

    .t text --(tokenizer, parser, symbolic interpreter)--> per Energy(...) argument and channel an expression DAG over loads of unknowns, loads of inputs,
    Param scalars and constants --(back end)--> one plug-in source in the shape of examples/plugins/*.hip --(build.build_plugin)--> lib<stem>.so

Nothing below the functor changes: a 2-D or 3-D domain gives a stencil functor (stencil_engine.h), a 1-D domain with a Graph a graph functor (graph_engine.h,
graph_onchip.h, graph_onchip_grid.h); the engines differentiate it with dual numbers.  What a plug-in author writes by hand -- the functor's constants, off(),
depends() / edgeDepends(), excluded(), bindParams, the ParamDecl table and the body hash -- is derived from the DAG and the declarations.

The subset.  Statements: local (several names), assignment, local function / function with return, for .. in Stencil{..},
numeric for, for _, v in ipairs(t), if on values known at generation time, do .. end.  Expressions: table constructors, t[i], t.k, calls, method calls (v:dot(w)),
+ - * /, unary minus, numbers, comparisons and and / or / not on generation-time values, the opt. prefix.  Vocabulary: Dim, Unknown, Array, Image, Param, Graph,
UsePreconditioner, Exclude, Energy; image access A(dx,dy[,dz]), A(0), A(0)(c), A(0,c) on a 1-D domain, X(G.v0), InBounds; Select, eq, greater, greatereq, less,
lesseq, Not, And, Or, All (conditions are 0/1 values: * of conditions is "and"); Vector, Dot3, :dot, Sqrt / sqrt, sin, cos, normalize, Rotate2D, Rotate3D,
Matrix3x3Mul, Slice.  Everything else raises TgenError with the .t line.

    python -m opt_amd.tgen file.t [--emit-only] [--out DIR]      prints the library path (--emit-only: the source path)
"""
import math
import os
import re
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
GEN_DIR = os.path.join(_HERE, "build_plugins", "gen")      # generated sources (not in git)


class TgenError(Exception):
    """A .t file outside the subset: `line` is the .t line, `what` the construct."""

    def __init__(self, path, line, what):
        self.path, self.line, self.what = path, line, what
        super().__init__(f"{os.path.basename(path)}:{line}: {what}")


# =====================================================================================================================================================================
# Front end 1: tokens and syntax tree
# =====================================================================================================================================================================
_KEYWORDS = {"and", "break", "do", "else", "elseif", "end", "false", "for", "function", "if", "in", "local", "nil", "not", "or", "repeat", "return", "then", "true",
             "until", "while", "goto"}
_TOKEN = re.compile(r"""
    (?P<ws>[ \t\r]+) | (?P<nl>\n) | (?P<lcomment>--\[\[.*?\]\]) | (?P<comment>--[^\n]*) |
    (?P<num>0[xX][0-9a-fA-F]+ | (?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?) | (?P<name>[A-Za-z_]\w*) |
    (?P<str>"(?:[^"\\\n]|\\.)*" | '(?:[^'\\\n]|\\.)*') |
    (?P<op>\.\.\.|\.\.|==|~=|<=|>=|[-+*/%^\#<>=(){}\[\];:,.])
""", re.X | re.S)


def _tokenize(text, path):
    toks, line, pos = [], 1, 0
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            raise TgenError(path, line, f"unsupported character {text[pos]!r}")
        kind, s = m.lastgroup, m.group()
        pos = m.end()
        if kind == "nl":
            line += 1
        elif kind in ("lcomment", "comment", "ws"):
            line += s.count("\n")
        elif kind == "num":
            toks.append(("num", float(int(s, 16)) if s[:2] in ("0x", "0X") else float(s), line))
        elif kind == "name":
            toks.append(("kw" if s in _KEYWORDS else "name", s, line))
        elif kind == "str":
            toks.append(("str", s[1:-1], line))
        else:
            toks.append(("op", s, line))
    toks.append(("eof", None, line))
    return toks


class _Parser:
    """Recursive descent over the token list; the tree is tuples (kind, line, ...)."""
    _BINARY = [("or",), ("and",), ("<", ">", "<=", ">=", "~=", "=="), ("..",), ("+", "-"), ("*", "/", "%")]

    def __init__(self, toks, path):
        self.t, self.i, self.path = toks, 0, path

    def peek(self, k=0):
        return self.t[self.i + k]

    def at(self, kind, val=None):
        t = self.t[self.i]
        return t[0] == kind and (val is None or t[1] == val)

    def at_kw(self, *vals):
        t = self.t[self.i]
        return t[0] == "kw" and t[1] in vals

    def at_op(self, *vals):
        t = self.t[self.i]
        return t[0] == "op" and t[1] in vals

    def next(self):
        t = self.t[self.i]
        self.i += 1
        return t

    def fail(self, what, line=None):
        raise TgenError(self.path, line or self.peek()[2], what)

    def expect(self, kind, val=None):
        if not self.at(kind, val):
            t = self.peek()
            self.fail(f"syntax: expected {val or kind!r}, found {t[1]!r}")
        return self.next()

    def block(self, *enders):
        out = []
        while not self.at("eof") and not self.at_kw(*enders):
            if self.at_op(";"):
                self.next()
                continue
            out.append(self.statement())
            if out[-1][0] == "return":
                break
        return out

    def names(self):
        ns = [self.expect("name")[1]]
        while self.at_op(","):
            self.next()
            ns.append(self.expect("name")[1])
        return ns

    def exprs(self):
        es = [self.expr()]
        while self.at_op(","):
            self.next()
            es.append(self.expr())
        return es

    def funcbody(self, line):
        self.expect("op", "(")
        params = []
        if not self.at_op(")"):
            if self.at_op("..."):
                self.fail("unsupported: variadic functions (...)")
            params = self.names()
        self.expect("op", ")")
        body = self.block("end")
        self.expect("kw", "end")
        return ("function", line, params, body)

    def statement(self):
        kind, val, line = self.peek()
        if kind == "kw":
            if val in ("while", "repeat", "goto", "break"):
                self.fail(f"unsupported statement: {val}")
            if val == "local":
                self.next()
                if self.at_kw("function"):
                    self.next()
                    name = self.expect("name")[1]
                    return ("local", line, [name], [self.funcbody(line)])
                ns = self.names()
                es = []
                if self.at_op("="):
                    self.next()
                    es = self.exprs()
                return ("local", line, ns, es)
            if val == "function":
                self.next()
                target = ("name", line, self.expect("name")[1])
                while self.at_op("."):
                    self.next()
                    target = ("index", line, target, ("const", line, self.expect("name")[1]))
                if self.at_op(":"):
                    self.fail("unsupported: method definitions (function a:b)")
                return ("assign", line, [target], [self.funcbody(line)])
            if val == "for":
                self.next()
                ns = self.names()
                if self.at_op("="):
                    self.next()
                    es = self.exprs()
                    if len(ns) != 1 or not 2 <= len(es) <= 3:
                        self.fail("syntax: numeric for takes one name and two or three bounds", line)
                    self.expect("kw", "do")
                    body = self.block("end")
                    self.expect("kw", "end")
                    return ("fornum", line, ns[0], es, body)
                self.expect("kw", "in")
                es = self.exprs()
                self.expect("kw", "do")
                body = self.block("end")
                self.expect("kw", "end")
                return ("forin", line, ns, es, body)
            if val == "if":
                self.next()
                arms, orelse = [], None
                cond = self.expr()
                self.expect("kw", "then")
                arms.append((cond, self.block("elseif", "else", "end")))
                while self.at_kw("elseif"):
                    self.next()
                    cond = self.expr()
                    self.expect("kw", "then")
                    arms.append((cond, self.block("elseif", "else", "end")))
                if self.at_kw("else"):
                    self.next()
                    orelse = self.block("end")
                self.expect("kw", "end")
                return ("if", line, arms, orelse)
            if val == "do":
                self.next()
                body = self.block("end")
                self.expect("kw", "end")
                return ("do", line, body)
            if val == "return":
                self.next()
                es = [] if self.at("eof") or self.at_kw("end", "else", "elseif") or self.at_op(";") else self.exprs()
                return ("return", line, es)
            self.fail(f"syntax: unexpected {val!r}")
        e = self.suffixed()
        if self.at_op("=", ","):
            targets = [e]
            while self.at_op(","):
                self.next()
                targets.append(self.suffixed())
            self.expect("op", "=")
            for t in targets:
                if t[0] not in ("name", "index"):
                    self.fail("syntax: cannot assign to this expression", line)
            return ("assign", line, targets, self.exprs())
        if e[0] not in ("call", "method"):
            self.fail("syntax: an expression is not a statement", line)
        return ("exprstat", line, e)

    def expr(self, level=0):
        if level == len(self._BINARY):
            return self.unary()
        left = self.expr(level + 1)
        while (self.at("op") or self.at("kw")) and self.peek()[1] in self._BINARY[level]:
            _, op, line = self.next()
            if op in ("..", "%"):
                self.fail(f"unsupported operator: {op}", line)
            left = ("binop", line, op, left, self.expr(level + 1))
        return left

    def unary(self):
        kind, val, line = self.peek()
        if (kind == "op" and val in ("-", "#")) or (kind == "kw" and val == "not"):
            self.next()
            return ("unop", line, val, self.unary())
        e = self.suffixed()
        if self.at_op("^"):
            self.fail("unsupported operator: ^ (pow)")
        return e

    def primary(self):
        kind, val, line = self.next()
        if kind == "num" or kind == "str":
            return ("const", line, val)
        if kind == "kw" and val in ("true", "false", "nil"):
            return ("const", line, {"true": True, "false": False, "nil": None}[val])
        if kind == "kw" and val == "function":
            return self.funcbody(line)
        if kind == "name":
            return ("name", line, val)
        if kind == "op" and val == "(":
            e = self.expr()
            self.expect("op", ")")
            return e
        if kind == "op" and val == "{":
            self.i -= 1
            return self.table()
        self.fail(f"syntax: unexpected {val!r}", line)

    def table(self):
        line = self.expect("op", "{")[2]
        items = []      # (key expression or None, value expression)
        while not self.at_op("}"):
            if self.at("name") and self.peek(1)[0] == "op" and self.peek(1)[1] == "=":
                key = ("const", line, self.next()[1])
                self.next()
                items.append((key, self.expr()))
            elif self.at_op("["):
                self.next()
                key = self.expr()
                self.expect("op", "]")
                self.expect("op", "=")
                items.append((key, self.expr()))
            else:
                items.append((None, self.expr()))
            if self.at_op(",", ";"):
                self.next()
            else:
                break
        self.expect("op", "}")
        return ("table", line, items)

    def suffixed(self):
        e = self.primary()
        while True:
            kind, val, line = self.peek()
            if kind == "op" and val == ".":
                self.next()
                e = ("index", line, e, ("const", line, self.expect("name")[1]))
            elif kind == "op" and val == "[":
                self.next()
                k = self.expr()
                self.expect("op", "]")
                e = ("index", line, e, k)
            elif kind == "op" and val == ":":
                self.next()
                name = self.expect("name")[1]
                e = ("method", line, e, name, self.callargs())
            elif (kind == "op" and val in ("(", "{")) or kind == "str":
                e = ("call", line, e, self.callargs())
            else:
                return e

    def callargs(self):
        if self.at("str"):
            t = self.next()
            return [("const", t[2], t[1])]
        if self.at_op("{"):
            return [self.table()]
        self.expect("op", "(")
        args = [] if self.at_op(")") else self.exprs()
        self.expect("op", ")")
        return args


# =====================================================================================================================================================================
# The expression DAG
# =====================================================================================================================================================================
class Node:
    """One node of the DAG.  op: const | param | uload | iload | inb | add sub mul div neg sqrt sin cos | select | cmp | and or not.
    val: the constant / (name, index) of a Param / (image, channel, where) of a load / where of inb / the comparison; where is ("off", (dx, dy, dz)) or ("slot", j) or
    ("vertex",).  cond: a 0/1 value.  dep: reads an unknown on a path that carries derivatives (not through a comparison).  Nodes are hash-consed per IR: the same
    expression built twice is one node, and ids ascend in the .t's evaluation order."""
    __slots__ = ("id", "op", "args", "val", "cond", "dep")

    def __repr__(self):
        return f"n{self.id}:{self.op}{self.val if self.val is not None else ''}({','.join('n%d' % a.id for a in self.args)})"


_CMP = {"eq": "==", "greater": ">", "greatereq": ">=", "less": "<", "lesseq": "<="}


class Graph_:
    def __init__(self):
        self.nodes, self.table = [], {}

    def node(self, op, args=(), val=None, cond=False):
        key = (op, tuple(a.id for a in args), val)
        n = self.table.get(key)
        if n is None:
            n = Node()
            n.id, n.op, n.args, n.val, n.cond = len(self.nodes), op, tuple(args), val, cond
            n.dep = op == "uload" or (op != "cmp" and any(a.dep for a in args))
            self.nodes.append(n)
            self.table[key] = n
        return n

    def const(self, v):
        return self.node("const", val=float(v))

    def true(self):
        return self.node("const", val=1.0, cond=True)

    def false(self):
        return self.node("const", val=0.0, cond=True)


class Vec:
    """A vector of scalars (Nodes or generation-time numbers): what ad.Vector builds and a multi-channel image access returns."""

    def __init__(self, items):
        self.items = list(items)

    def __len__(self):
        return len(self.items)


class _Decl:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class IR:
    """What executing a .t yields.  dims [(name, index)]; images [_Decl(name, kind "unknown"|"array", type, channels, index, img)] in declaration order; params
    [_Decl(name, type, index)]; graph _Decl(name, index, slots [(name, index)]) or None; use_preconditioner; exclude (a cond Node or None); residuals
    [_Decl(node, line, term "pixel"|"vertex"|"edge")] one per scalar residual in Energy order; kind "stencil" | "graph"; body_hash (filled by generate)."""

    def __init__(self, path):
        self.path, self.stem = path, os.path.splitext(os.path.basename(path))[0]
        self.g = Graph_()
        self.dims, self.images, self.params, self.graph = [], [], [], None
        self.use_preconditioner, self.exclude, self.residuals = False, None, []
        self.body_hash = None

    @property
    def ndim(self):
        return len(self.dims)

    @property
    def kind(self):
        return "graph" if self.graph is not None else "stencil"

    @property
    def unknowns(self):
        return [im for im in self.images if im.kind == "unknown"]

    def K(self):
        return sum(im.channels for im in self.unknowns)

    def k_of(self, im, c):
        return sum(u.channels for u in self.unknowns[:im.img]) + c

    def reachable(self, roots):
        seen, order = set(), []
        stack = list(roots)
        while stack:
            n = stack.pop()
            if n.id in seen:
                continue
            seen.add(n.id)
            order.append(n)
            stack.extend(n.args)
        return sorted(order, key=lambda n: n.id)

    def unknown_reads(self, root, derivative_only):
        """{(image name, channel, where)} of the unknown loads below root (derivative_only: not those that only a comparison reads)."""
        seen, out, stack = set(), set(), [root]
        while stack:
            n = stack.pop()
            if n.id in seen or (derivative_only and not n.dep):
                continue
            seen.add(n.id)
            if n.op == "uload":
                out.add(n.val)
            stack.extend(n.args)
        return out

    def offsets(self):
        """The offsets at which some residual reads an unknown: the centre first, the others in the order the .t first reads them."""
        offs = [(0, 0, 0)]
        for n in self.reachable([r.node for r in self.residuals]):
            if n.op == "uload" and n.val[2][0] == "off" and n.val[2][1] not in offs:
                offs.append(n.val[2][1])
        return offs

    def depends(self):
        """[R][NOFF]: residual ri carries a derivative w.r.t. the unknowns at offset oi."""
        offs = self.offsets()
        return [[any(w == ("off", o) for _, _, w in self.unknown_reads(r.node, True)) for o in offs] for r in self.residuals]

    def counts(self):
        """(RV, RE) of a graph energy, (R, 0) of a stencil one."""
        if self.kind == "stencil":
            return len(self.residuals), 0
        return sum(r.term == "vertex" for r in self.residuals), sum(r.term == "edge" for r in self.residuals)

    def edge_depends(self):
        """[RE][V][K] of a graph energy."""
        K, V = self.K(), len(self.graph.slots)
        img = {im.name: im for im in self.images}
        out = []
        for r in self.residuals:
            if r.term != "edge":
                continue
            t = [[False] * K for _ in range(V)]
            for name, c, w in self.unknown_reads(r.node, True):
                t[w[1]][self.k_of(img[name], c)] = True
            out.append(t)
        return out


# =====================================================================================================================================================================
# Front end 2: the symbolic interpreter
# =====================================================================================================================================================================
class _Return(Exception):
    def __init__(self, values):
        self.values = values


class _Table:
    def __init__(self):
        self.d = {}

    def array(self):
        out, i = [], 1
        while i in self.d:
            out.append(self.d[i])
            i += 1
        return out


class _Func:
    def __init__(self, params, body, env):
        self.params, self.body, self.env = params, body, env


class _Type:
    def __init__(self, name, channels):
        self.name, self.channels = name, channels


class _Dim:
    def __init__(self, name, index):
        self.name, self.index = name, index


class _Slot:
    def __init__(self, graph, j, name):
        self.graph, self.j, self.name = graph, j, name


class _Iter:
    def __init__(self, rows):
        self.rows = rows


class _Slice:
    def __init__(self, im, s, e):
        self.im, self.s, self.e = im, s, e


class _Env:
    def __init__(self, parent=None):
        self.vars, self.parent = {}, parent

    def find(self, name):
        e = self
        while e is not None:
            if name in e.vars:
                return e
            e = e.parent
        return None


_REFUSED = {"ComputedArray": "ComputedArray (the engines of a generated energy hold no computed planes)", "ComputedImage": "ComputedImage",
            "L_p": "L_p (it needs pow and a ComputedArray)", "L_2_norm": "L_2_norm", "SampledImage": "SampledImage (no sampled inputs in a generated energy)",
            "sampledimage": "sampledimage", "pow": "pow (the engine's dual numbers have no pow)", "exp": "exp (the engine's dual numbers have no exp)",
            "log": "log (the engine's dual numbers have no log)", "require": "require", "abs": "abs (the engine's dual numbers have no abs)",
            "tan": "tan", "acos": "acos", "asin": "asin", "atan": "atan", "Index": "Index", "length": "length (write Sqrt(Dot3(d, d)))",
            "terralib": "terralib", "setmetatable": "setmetatable", "unpack": "unpack", "pairs": "pairs", "ad": "the ad table", "Result": "Result"}


class _Interp:
    def __init__(self, path):
        self.path, self.ir = path, IR(path)
        self.g = self.ir.g
        self.line = 0
        self.globals = _Env()
        self.depth = 0
        v = self.globals.vars
        for name in ("Dim", "Unknown", "Array", "Image", "Param", "Graph", "UsePreconditioner", "Exclude", "Energy", "InBounds", "Select", "Not", "And", "Or", "All",
                     "Vector", "Dot3", "Sqrt", "sqrt", "sin", "cos", "normalize", "Rotate2D", "Rotate3D", "Matrix3x3Mul", "Slice", "Stencil", "ipairs"):
            v[name] = getattr(self, "f_" + name)
        for name in _CMP:
            v[name] = (lambda kind: lambda *a: self.f_cmp(kind, *a))(name)
        v["opt_float"] = _Type("opt_float", 1)
        v["float"] = _Type("float", 1)
        for c in (2, 3, 4, 9):
            v[f"opt_float{c}"] = _Type(f"opt_float{c}", c)
        opt = _Table()
        opt.d = v      # opt.Dim is Dim: the prefix names the same vocabulary
        v["opt"] = opt

    def fail(self, what, line=None):
        raise TgenError(self.path, line or self.line, what)

    # ---- scalars and vectors ---------------------------------------------------------------------------------------------------------------------------------
    def scalar(self, x):
        """A Node from a Node or a generation-time number."""
        if isinstance(x, Node):
            return x
        if isinstance(x, bool):
            return self.g.true() if x else self.g.false()
        if isinstance(x, (int, float)):
            return self.g.const(x)
        self.fail(f"unsupported: {self.describe(x)} where a number or an expression is expected")

    def value(self, n):
        """A condition used as a number is its 0/1 value."""
        n = self.scalar(n)
        if n.cond:
            if n.op == "const":
                return self.g.const(n.val)
            return self.g.node("select", (n, self.g.const(1), self.g.const(0)))
        return n

    def cond(self, n):
        n = self.scalar(n)
        if n.cond:
            return n
        if n.op == "const":
            return self.g.true() if n.val != 0 else self.g.false()
        return self.g.node("not", (self.g.node("cmp", (n, self.g.const(0)), "eq", cond=True),), cond=True)

    @staticmethod
    def describe(x):
        return {_Table: "a table", _Func: "a function", str: "a string", type(None): "nil", Vec: "a vector", _Type: "a type", _Dim: "a Dim"}.get(type(x), type(x).__name__.strip("_"))

    def broadcast(self, fn, *args):
        n = {len(a) for a in args if isinstance(a, Vec)}
        if not n:
            return fn(*args)
        if len(n) > 1:
            self.fail(f"vectors of different sizes ({sorted(n)}) in one operation")
        n = n.pop()
        return Vec([self.broadcast(fn, *[a.items[i] if isinstance(a, Vec) else a for a in args]) for i in range(n)])

    def arith(self, op, a, b):
        return self.broadcast(lambda x, y: self.arith1(op, x, y), a, b)

    def arith1(self, op, a, b):
        num = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
        if num(a) and num(b):
            if op == "div" and b == 0:
                self.fail("division by zero at generation time")
            return {"add": a + b, "sub": a - b, "mul": a * b, "div": a / b if op == "div" else 0}[op]
        a, b = self.scalar(a), self.scalar(b)
        if op == "mul":
            if a.cond and b.cond:      # conditions are 0/1 values: their product is "and"
                if a.op == "const":
                    return b if a.val else a
                if b.op == "const":
                    return a if b.val else b
                return self.g.node("and", (a, b), cond=True)
            if a.cond or b.cond:       # a condition times a value selects the value
                c, x = (a, b) if a.cond else (b, a)
                if x.op == "const" and x.val == 1.0:
                    return c           # (All, And: the running product starts at the number 1)
                return self.f_Select(c, x, 0.0)
            if a.op == "const" and a.val == 1.0:
                return b
            if b.op == "const" and b.val == 1.0:
                return a
        a, b = self.value(a), self.value(b)
        if op == "add" and a.op == "const" and a.val == 0.0:      # (sum(): the running sum starts at the number 0)
            return b
        return self.g.node(op, (a, b))

    def neg(self, a):
        if isinstance(a, (int, float)):
            return -a
        if isinstance(a, Vec):
            return Vec([self.neg(x) for x in a.items])
        a = self.value(a)
        if a.op == "const":
            return self.g.const(-a.val)
        return self.g.node("neg", (a,))

    def unary_fn(self, op, pyfn):
        def one(x):
            if isinstance(x, (int, float)):
                return pyfn(x)
            return self.g.node(op, (self.value(x),))
        return lambda *a: self.broadcast(one, *self.nargs(op, a, 1))

    def nargs(self, name, a, n, most=None):
        if not n <= len(a) <= (most or n):
            self.fail(f"{name} takes {n}{'' if not most else '..' + str(most)} arguments, got {len(a)}")
        return a

    # ---- the vocabulary --------------------------------------------------------------------------------------------------------------------------------------------
    def lit_int(self, x, what):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or x != int(x):
            self.fail(f"{what} must be a literal integer, got {self.describe(x)}")
        return int(x)

    def f_Dim(self, *a):
        name, index = self.nargs("Dim", a, 2)
        d = _Dim(name, self.lit_int(index, "the index of a Dim"))
        if any(n == name for n, _ in self.ir.dims):
            self.fail(f"Dim \"{name}\" is declared twice")
        self.ir.dims.append((name, d.index))
        return d

    def image_decl(self, kind, a):
        a = list(a)
        if len(a) == 3:
            a.insert(1, _Type("opt_float", 1))      # the typeless form
            typeless = True
        else:
            typeless = False
        name, typ, dims, index = self.nargs(kind, a, 4)
        if not isinstance(name, str) or not isinstance(dims, _Table):
            self.fail(f"{kind}(name, [type,] {{dims}}, index) expected")
        if not isinstance(typ, _Type):
            self.fail(f"unsupported element type of \"{name}\": only float, opt_float and opt_float2/3/4/9 images are read")
        ds = dims.array()
        if [d.name if isinstance(d, _Dim) else None for d in ds] != [n for n, _ in self.ir.dims]:
            self.fail(f"\"{name}\" is not declared over the whole domain {{{', '.join(n for n, _ in self.ir.dims)}}}: one index space per energy")
        d = _Decl(name=name, kind="unknown" if kind == "Unknown" else "array", type="" if typeless else typ.name, channels=typ.channels,
                  index=self.lit_int(index, "a binding index"), img=len(self.ir.unknowns) if kind == "Unknown" else -1, line=self.line)
        if any(im.name == name for im in self.ir.images):
            self.fail(f"\"{name}\" is declared twice")
        self.ir.images.append(d)
        return d

    def f_Unknown(self, *a):
        return self.image_decl("Unknown", a)

    def f_Array(self, *a):
        return self.image_decl("Array", a)

    def f_Image(self, *a):
        return self.image_decl("Image", a)

    def f_Param(self, *a):
        name, typ, index = self.nargs("Param", a, 3)
        if not isinstance(typ, _Type) or typ.name != "float":
            self.fail(f"unsupported Param type of \"{name}\": Params are host floats")
        d = _Decl(name=name, type=typ.name, index=self.lit_int(index, "a binding index"))
        self.ir.params.append(d)
        return self.g.node("param", val=(name, d.index))

    def f_Graph(self, *a):
        if self.ir.graph is not None:
            self.fail("unsupported: more than one Graph")
        if self.ir.ndim != 1:
            self.fail(f"unsupported: a Graph over a domain of {self.ir.ndim} dimensions (mesh energies live on a 1-D domain)")
        if len(a) < 5 or (len(a) - 2) % 3:
            self.fail("Graph(name, index, slot, {dims}, index, ...) expected")
        d = _Decl(name=a[0], index=self.lit_int(a[1], "a binding index"), slots=[])
        t = _Table()
        for j in range((len(a) - 2) // 3):
            sname, sdims, sidx = a[2 + 3 * j: 5 + 3 * j]
            ds = sdims.array() if isinstance(sdims, _Table) else []
            if not isinstance(sname, str) or len(ds) != 1 or not isinstance(ds[0], _Dim):
                self.fail(f"unsupported: Graph slot {j} must index the one 1-D domain")
            d.slots.append((sname, self.lit_int(sidx, "a binding index")))
            t.d[sname] = _Slot(d, j, sname)
        self.ir.graph = d
        return t

    def f_UsePreconditioner(self, *a):
        (v,) = self.nargs("UsePreconditioner", a, 1)
        if not isinstance(v, bool):
            self.fail("UsePreconditioner takes true or false")
        self.ir.use_preconditioner = v

    def f_Exclude(self, *a):
        (c,) = self.nargs("Exclude", a, 1)
        if isinstance(c, Vec):
            self.fail("Exclude takes one condition, not a vector")
        c = self.cond(c)
        for n in self.ir.reachable([c]):
            if n.op == "uload" or n.op == "inb" or (n.op == "iload" and n.val[2] != ("off", (0, 0, 0))):
                self.fail("unsupported: an Exclude condition that reads an unknown, a neighbour or InBounds (it is evaluated from the pixel's own inputs)")
        if self.ir.kind == "graph" or self.ir.ndim == 1:
            self.fail("unsupported: Exclude on a 1-D domain (the graph engine has no excluded vertices)")
        self.ir.exclude = c if self.ir.exclude is None else self.g.node("or", (self.ir.exclude, c), cond=True)

    def f_Energy(self, *a):
        if not a:
            self.fail("Energy() without a term")
        if self.ir.ndim == 0:
            self.fail("Energy before any Dim")
        if self.ir.ndim == 1 and self.ir.graph is None:
            self.fail("unsupported: a 1-D domain without a Graph (the stencil engine serves 2-D and 3-D domains)")
        if self.ir.ndim > 3:
            self.fail("unsupported: a domain of more than 3 dimensions")
        rows = []
        for term in a:
            for x in (self.flatten(term) if isinstance(term, Vec) else [term]):
                rows.append(self.value(x))
        if not any(self.ir.unknown_reads(n, True) for n in rows):
            self.fail("unsupported: an Energy that reads no unknown")
        for n in rows:
            wheres = {w[0] for k in ("uload", "iload") for m in self.ir.reachable([n]) if m.op == k for w in [m.val[2]]}
            if self.ir.kind == "graph":
                if wheres == {"slot", "vertex"}:
                    self.fail("unsupported: one Energy term that reads both the vertex (A(0)) and graph slots (A(G.v))")
                term = "edge" if "slot" in wheres else "vertex"
            else:
                term, n = "pixel", self.default_guard(n)
            self.ir.residuals.append(_Decl(node=n, line=self.line, term=term))

    def flatten(self, v):
        out = []
        for x in v.items:
            out.extend(self.flatten(x) if isinstance(x, Vec) else [x])
        return out

    def f_InBounds(self, *a):
        if self.ir.kind == "graph" or self.ir.ndim == 1:
            self.fail("unsupported: InBounds on a 1-D domain")
        return self.g.node("inb", val=self.offset(a, "InBounds"), cond=True)      # (the centre too: a residual that asks InBounds opts out of the default guard)

    def default_guard(self, n):
        """The reference's default for a residual of an image domain that never asks InBounds: it is 0 wherever the bounding box of its accesses (the centre
        included) leaves the image.  A residual that uses InBounds anywhere states its own rule and gets none."""
        nodes = self.ir.reachable([n])
        if any(m.op == "inb" for m in nodes):
            return n
        offs = [m.val[2][1] for m in nodes if m.op in ("uload", "iload")] + [(0, 0, 0)]
        lo, hi = tuple(min(o[a] for o in offs) for a in range(3)), tuple(max(o[a] for o in offs) for a in range(3))
        guard = None
        for corner in (lo, hi):
            if corner != (0, 0, 0):
                c = self.g.node("inb", val=corner, cond=True)
                guard = c if guard is None or guard is c else self.g.node("and", (guard, c), cond=True)
        return n if guard is None else self.g.node("select", (guard, n, self.g.const(0)))

    def offset(self, a, what):
        if len(a) != self.ir.ndim:
            self.fail(f"{what} takes {self.ir.ndim} offsets on this domain, got {len(a)}")
        for x in a:
            if isinstance(x, bool) or not isinstance(x, (int, float)) or x != int(x):
                self.fail(f"unsupported: a stencil offset that is not a literal integer ({self.describe(x)})")
        return tuple(int(x) for x in a) + (0,) * (3 - len(a))

    def access(self, im, a):
        """A(...) on a declared image."""
        def load(where, c):
            if im.kind == "unknown":
                return self.g.node("uload", val=(im.name, c, where))
            return self.g.node("iload", val=(im.name, c, where))

        def whole(where):
            return load(where, 0) if im.channels == 1 else Vec([load(where, c) for c in range(im.channels)])

        if self.ir.ndim == 1:
            if self.ir.graph is None:
                self.fail("unsupported: a 1-D domain without a Graph (the stencil engine serves 2-D and 3-D domains)")
            if not a or len(a) > 2:
                self.fail(f"\"{im.name}\" takes A(0), A(0, c) or A(G.v) on a 1-D domain")
            if isinstance(a[0], _Slot):
                if len(a) != 1:
                    self.fail(f"\"{im.name}\"(G.v) takes no channel argument")
                return whole(("slot", a[0].j))
            if isinstance(a[0], bool) or not isinstance(a[0], (int, float)) or a[0] != int(a[0]):
                self.fail("unsupported: a stencil offset that is not a literal integer")
            if a[0] != 0:
                what = "reads an unknown" if im.kind == "unknown" else "reads an input"
                self.fail(f"unsupported: a vertex term of a mesh energy that {what} at a non-zero offset ({int(a[0])}); neighbours are reached through the Graph")
            if len(a) == 2:
                c = self.lit_int(a[1], "a channel")
                if not 0 <= c < im.channels:
                    self.fail(f"channel {c} of \"{im.name}\" ({im.channels} channels)")
                return load(("vertex",), c)
            return whole(("vertex",))
        if a and isinstance(a[0], _Slot):
            self.fail("unsupported: a Graph over a domain of more than one dimension")
        return whole(("off", self.offset(a, f"\"{im.name}\"")))

    def f_cmp(self, kind, *a):
        x, y = self.nargs(kind, a, 2)

        def one(p, q):
            p, q = self.value(p), self.value(q)
            if p.op == "const" and q.op == "const":
                r = {"eq": p.val == q.val, "greater": p.val > q.val, "greatereq": p.val >= q.val, "less": p.val < q.val, "lesseq": p.val <= q.val}[kind]
                return self.g.true() if r else self.g.false()
            return self.g.node("cmp", (p, q), kind, cond=True)
        return self.broadcast(one, x, y)

    def f_Select(self, *a):
        c, x, y = self.nargs("Select", a, 3)

        def one(c, x, y):
            c = self.cond(c)
            if c.op == "const":
                return x if c.val else y
            x, y = self.scalar(x), self.scalar(y)
            if x.cond and y.cond:
                self.fail("unsupported: Select between two conditions (write And / Or)")
            return self.g.node("select", (c, self.value(x), self.value(y)))
        return self.broadcast(one, c, x, y)

    def f_Not(self, *a):
        def one(c):
            c = self.cond(c)
            if c.op == "const":
                return self.g.false() if c.val else self.g.true()
            return self.g.node("not", (c,), cond=True)
        return self.broadcast(one, *self.nargs("Not", a, 1))

    def f_And(self, *a):
        r = 1.0
        for x in a:
            r = self.arith("mul", r, self.broadcast(self.cond, x))
        return r

    def f_Or(self, *a):
        def or2(p, q):
            p, q = self.cond(p), self.cond(q)
            if p.op == "const":
                return p if p.val else q
            if q.op == "const":
                return q if q.val else p
            return p if p is q else self.g.node("or", (p, q), cond=True)
        r = self.g.false()
        for x in a:
            r = self.broadcast(or2, r, x)
        return r

    def f_All(self, *a):
        (v,) = self.nargs("All", a, 1)
        r = 1.0
        for x in (v.items if isinstance(v, Vec) else [v]):
            r = self.arith("mul", r, x)
        return r

    def f_Vector(self, *a):
        for x in a:
            if not isinstance(x, (Node, Vec, int, float)):
                self.fail(f"Vector of {self.describe(x)}")
        return Vec(a)

    def vec(self, v, n, what):
        if not isinstance(v, Vec) or len(v) < n:
            self.fail(f"{what} takes a vector of at least {n} channels")
        return v.items

    def f_Dot3(self, *a):
        p, q = self.nargs("Dot3", a, 2)
        p, q = self.vec(p, 3, "Dot3"), self.vec(q, 3, "Dot3")
        mul, add = (lambda x, y: self.arith("mul", x, y)), (lambda x, y: self.arith("add", x, y))
        return add(add(mul(p[0], q[0]), mul(p[1], q[1])), mul(p[2], q[2]))

    def f_Sqrt(self, *a):
        return self.unary_fn("sqrt", math.sqrt)(*a)

    f_sqrt = f_Sqrt

    def f_sin(self, *a):
        return self.unary_fn("sin", math.sin)(*a)

    def f_cos(self, *a):
        return self.unary_fn("cos", math.cos)(*a)

    def f_normalize(self, *a):
        (v,) = self.nargs("normalize", a, 1)
        return self.arith("div", v, self.f_Sqrt(self.f_Dot3(v, v)))

    def f_Matrix3x3Mul(self, *a):
        m, v = self.nargs("Matrix3x3Mul", a, 2)
        m, v = self.vec(m, 9, "Matrix3x3Mul"), self.vec(v, 3, "Matrix3x3Mul")
        mul, add = (lambda x, y: self.arith("mul", x, y)), (lambda x, y: self.arith("add", x, y))
        return Vec([add(add(mul(m[3 * i], v[0]), mul(m[3 * i + 1], v[1])), mul(m[3 * i + 2], v[2])) for i in range(3)])

    def f_Rotate3D(self, *a):
        """Euler angles (alpha, beta, gamma) about x, y, z: R = Rz(gamma) Ry(beta) Rx(alpha), row-major, then Matrix3x3Mul."""
        ang, v = self.nargs("Rotate3D", a, 2)
        al, be, ga = self.vec(ang, 3, "Rotate3D")[:3]
        ca, cb, cg, sa, sb, sg = self.f_cos(al), self.f_cos(be), self.f_cos(ga), self.f_sin(al), self.f_sin(be), self.f_sin(ga)
        mul, add, neg = (lambda x, y: self.arith("mul", x, y)), (lambda x, y: self.arith("add", x, y)), self.neg
        m = Vec([mul(cg, cb), add(mul(neg(sg), ca), mul(mul(cg, sb), sa)), add(mul(sg, sa), mul(mul(cg, sb), ca)),
                 mul(sg, cb), add(mul(cg, ca), mul(mul(sg, sb), sa)), add(mul(neg(cg), sa), mul(mul(sg, sb), ca)),
                 neg(sb), mul(cb, sa), mul(cb, ca)])
        return self.f_Matrix3x3Mul(m, v)

    def f_Rotate2D(self, *a):
        ang, v = self.nargs("Rotate2D", a, 2)
        if isinstance(ang, Vec):
            self.fail("Rotate2D takes a scalar angle")
        v = self.vec(v, 2, "Rotate2D")
        c, s = self.f_cos(ang), self.f_sin(ang)
        mul, add = (lambda x, y: self.arith("mul", x, y)), (lambda x, y: self.arith("add", x, y))
        return Vec([add(mul(c, v[0]), mul(self.neg(s), v[1])), add(mul(s, v[0]), mul(c, v[1]))])

    def f_Slice(self, *a):
        im, s, e = self.nargs("Slice", a, 3)
        if not isinstance(im, (_Decl, _Slice)):
            self.fail("Slice takes an image")
        s, e = self.lit_int(s, "a Slice bound"), self.lit_int(e, "a Slice bound")
        if not 0 <= s < e:
            self.fail(f"Slice bounds {s}, {e}")
        return _Slice(im, s, e)

    def f_Stencil(self, *a):
        (t,) = self.nargs("Stencil", a, 1)
        if not isinstance(t, _Table):
            self.fail("Stencil takes a table of offsets")
        rows = []
        for r in t.array():
            if not isinstance(r, _Table):
                self.fail("Stencil takes a table of offset tables")
            rows.append(tuple(r.array()))
        return _Iter(rows)

    def f_ipairs(self, *a):
        (t,) = self.nargs("ipairs", a, 1)
        if not isinstance(t, _Table):
            self.fail("ipairs takes a table")
        return _Iter([(float(i + 1), v) for i, v in enumerate(t.array())])

    # ---- evaluation ------------------------------------------------------------------------------------------------------------------------------------------------
    def lookup(self, name, env, line):
        e = env.find(name)
        if e is not None:
            return e.vars[name]
        if name in _REFUSED:
            self.fail(f"unsupported: {_REFUSED[name]}", line)
        self.fail(f"unsupported: the name '{name}' is not part of the subset (or is undefined)", line)

    def call(self, f, args, line):
        self.line = line
        if isinstance(f, _Func):
            if self.depth > 64:
                self.fail("unsupported: recursion deeper than 64 calls")
            env = _Env(f.env)
            for i, p in enumerate(f.params):
                env.vars[p] = args[i] if i < len(args) else None
            self.depth += 1
            try:
                self.exec_block(f.body, env)
            except _Return as r:
                return r.values
            finally:
                self.depth -= 1
                self.line = line
            return []
        if isinstance(f, _Decl) and hasattr(f, "channels"):
            return [self.access(f, args)]
        if isinstance(f, _Slice):
            v = self.call(f.im, args, line)[0]
            items = v.items if isinstance(v, Vec) else [v]
            if f.e > len(items):
                self.fail(f"Slice bound {f.e} beyond the {len(items)} channels of the image")
            return [items[f.s] if f.s + 1 == f.e else Vec(items[f.s:f.e])]
        if isinstance(f, Vec):
            (i,) = self.nargs("a vector index", args, 1)
            i = self.lit_int(i, "a vector index")
            if not 0 <= i < len(f):
                self.fail(f"channel {i} of a vector of {len(f)}")
            return [f.items[i]]
        if callable(f):
            r = f(*args)
            self.line = line
            return [r]
        if isinstance(f, Node):
            self.fail("unsupported: indexing a scalar expression like a vector")
        self.fail(f"unsupported: calling {self.describe(f)}")

    def method(self, obj, name, args, line):
        self.line = line
        if isinstance(obj, Vec):
            if name == "dot":
                (w,) = self.nargs("dot", args, 1)
                if not isinstance(w, Vec) or len(w) != len(obj):
                    self.fail("dot takes a vector of the same size")
                return self.method(self.arith("mul", obj, w), "sum", [], line)
            if name == "sum":
                s = 0.0
                for x in obj.items:
                    s = self.arith("add", s, x)
                return s
            if name == "size":
                return float(len(obj))
        self.fail(f"unsupported: method :{name} of {self.describe(obj)}")

    def eval_multi(self, es, env):
        """Lua's adjustment: every expression gives one value, the last one all of its values."""
        out = []
        for i, e in enumerate(es):
            if e[0] == "call" and i == len(es) - 1:
                out.extend(self.call(self.eval(e[2], env), self.eval_multi(e[3], env), e[1]))
            else:
                out.append(self.eval(e, env))
        return out

    def eval(self, e, env):
        kind, line = e[0], e[1]
        if kind == "const":
            return e[2]
        if kind == "name":
            return self.lookup(e[2], env, line)
        if kind == "call":
            r = self.call(self.eval(e[2], env), self.eval_multi(e[3], env), line)
            return r[0] if r else None
        if kind == "method":
            return self.method(self.eval(e[2], env), e[3], self.eval_multi(e[4], env), line)
        if kind == "index":
            obj, key = self.eval(e[2], env), self.eval(e[3], env)
            self.line = line
            if isinstance(obj, _Table):
                if isinstance(key, float) and key == int(key):
                    key = int(key)
                if obj.d is self.globals.vars and key not in obj.d:
                    return self.lookup(key, self.globals, line)
                return obj.d.get(key)
            if isinstance(obj, Vec) and isinstance(key, (int, float)):
                return self.call(obj, [key], line)[0]
            self.fail(f"unsupported: indexing {self.describe(obj)}")
        if kind == "table":
            t, n = _Table(), 0
            for i, (k, v) in enumerate(e[2]):
                if k is None:
                    vals = self.eval_multi([v], env) if i == len(e[2]) - 1 else [self.eval(v, env)]
                    for x in vals:
                        n += 1
                        t.d[n] = x
                else:
                    key = self.eval(k, env)
                    t.d[int(key) if isinstance(key, float) and key == int(key) else key] = self.eval(v, env)
            return t
        if kind == "function":
            return _Func(e[2], e[3], env)
        if kind == "unop":
            x = self.eval(e[3], env)
            self.line = line
            if e[2] == "-":
                if not isinstance(x, (Node, Vec, int, float)) or isinstance(x, bool):
                    self.fail(f"unsupported: - of {self.describe(x)}")
                return self.neg(x)
            if e[2] == "not":
                if isinstance(x, (Node, Vec)):
                    self.fail("unsupported: 'not' of an expression (write Not(...))")
                return x is None or x is False
            if isinstance(x, _Table):
                return float(len(x.array()))
            self.fail(f"unsupported: # of {self.describe(x)}")
        if kind == "binop":
            op = e[2]
            if op in ("and", "or"):
                a = self.eval(e[3], env)
                if isinstance(a, (Node, Vec)):
                    self.fail(f"unsupported: '{op}' on an expression (write And / Or)", line)
                truthy = not (a is None or a is False)
                return self.eval(e[4], env) if truthy == (op == "and") else a
            a, b = self.eval(e[3], env), self.eval(e[4], env)
            self.line = line
            if op in ("==", "~=", "<", ">", "<=", ">="):
                if isinstance(a, (Node, Vec)) or isinstance(b, (Node, Vec)):
                    self.fail(f"unsupported: '{op}' on an expression (write eq / greater / ... ; an 'if' needs a value known at generation time)")
                if op in ("==", "~="):
                    return (a == b) == (op == "==")
                if not (isinstance(a, (int, float)) and isinstance(b, (int, float))):
                    self.fail(f"'{op}' on {self.describe(a)} and {self.describe(b)}")
                return {"<": a < b, ">": a > b, "<=": a <= b, ">=": a >= b}[op]
            for x in (a, b):
                if not isinstance(x, (Node, Vec, int, float)) or isinstance(x, bool):
                    self.fail(f"unsupported: arithmetic on {self.describe(x)}")
            return self.arith({"+": "add", "-": "sub", "*": "mul", "/": "div"}[op], a, b)
        self.fail(f"unsupported expression: {kind}", line)

    def assign(self, target, value, env):
        if target[0] == "name":
            e = env.find(target[2]) or self.globals
            e.vars[target[2]] = value
        else:
            obj, key = self.eval(target[2], env), self.eval(target[3], env)
            if not isinstance(obj, _Table) or obj.d is self.globals.vars:
                self.fail(f"unsupported: assignment into {self.describe(obj)}", target[1])
            obj.d[int(key) if isinstance(key, float) and key == int(key) else key] = value

    def exec_block(self, stmts, env):
        for s in stmts:
            kind, line = s[0], s[1]
            self.line = line
            if kind == "local":
                vals = self.eval_multi(s[3], env) if s[3] else []
                if len(s[3]) == 1 and s[3][0][0] == "function":      # local function f: the name is in scope of its own body
                    env.vars[s[2][0]] = None
                    f = _Func(s[3][0][2], s[3][0][3], env)
                    env.vars[s[2][0]] = f
                    continue
                for i, n in enumerate(s[2]):
                    env.vars[n] = vals[i] if i < len(vals) else None
            elif kind == "assign":
                vals = self.eval_multi(s[3], env)
                for i, t in enumerate(s[2]):
                    self.assign(t, vals[i] if i < len(vals) else None, env)
            elif kind == "exprstat":
                self.eval(s[2], env)
            elif kind == "return":
                raise _Return(self.eval_multi(s[2], env))
            elif kind == "do":
                self.exec_block(s[2], _Env(env))
            elif kind == "if":
                done = False
                for cond, body in s[2]:
                    c = self.eval(cond, env)
                    if isinstance(c, (Node, Vec)):
                        self.fail("unsupported: 'if' on a value that is not known at generation time (write Select)", line)
                    if not (c is None or c is False):
                        self.exec_block(body, _Env(env))
                        done = True
                        break
                if not done and s[3] is not None:
                    self.exec_block(s[3], _Env(env))
            elif kind == "fornum":
                b = [self.eval(x, env) for x in s[3]]
                for x in b:
                    if isinstance(x, bool) or not isinstance(x, (int, float)):
                        self.fail("unsupported: a numeric for whose bounds are not known at generation time", line)
                lo, hi, step = b[0], b[1], (b[2] if len(b) > 2 else 1.0)
                if step == 0:
                    self.fail("numeric for with step 0", line)
                i = lo
                while (i <= hi) if step > 0 else (i >= hi):
                    inner = _Env(env)
                    inner.vars[s[2]] = i
                    self.exec_block(s[4], inner)
                    i += step
            elif kind == "forin":
                it = self.eval_multi(s[3], env)
                if len(it) != 1 or not isinstance(it[0], _Iter):
                    self.fail("unsupported: for .. in over anything but Stencil{...} or ipairs(t)", line)
                for row in it[0].rows:
                    inner = _Env(env)
                    for i, n in enumerate(s[2]):
                        inner.vars[n] = row[i] if i < len(row) else None
                    self.exec_block(s[4], inner)
            else:
                self.fail(f"unsupported statement: {kind}", line)


def parse(t_path):
    """Execute a .t symbolically: the IR of its energy (no GPU code, no library needed)."""
    t_path = os.path.abspath(t_path)
    text = open(t_path).read()
    if text.startswith("\ufeff"):
        text = text[1:]
    it = _Interp(t_path)
    tree = _Parser(_tokenize(text, t_path), t_path).block()
    try:
        it.exec_block(tree, it.globals)
    except _Return:
        pass
    ir = it.ir
    last = text.count("\n") + 1
    if not ir.residuals:
        raise TgenError(t_path, last, "the file has no Energy")
    if not ir.unknowns:
        raise TgenError(t_path, last, "the file declares no Unknown")
    if sorted(i for _, i in ir.dims) != list(range(ir.ndim)):
        raise TgenError(t_path, last, "the Dim indices must be 0 .. n-1")
    ir.dims.sort(key=lambda d: d[1])
    idx = [im.index for im in ir.images] + [p.index for p in ir.params] + ([ir.graph.index] + [i for _, i in ir.graph.slots] if ir.graph else [])
    if len(set(idx)) != len(idx):
        raise TgenError(t_path, last, "two declarations share a binding index")
    if not re.fullmatch(r"[A-Za-z_]\w*", ir.stem):
        raise TgenError(t_path, 1, f"the file stem '{ir.stem}' names the energy and its functor: it must be an identifier")
    return ir


# =====================================================================================================================================================================
# evaluate: the DAG in float64 numpy
# =====================================================================================================================================================================
def evaluate(ir, problem):
    """Float64 evaluation of the DAG on a workloads.Problem (params by binding index).  Returns (residuals, cost).  Stencil energies: residuals[R, D, H, W] with the
    axes beyond the domain's dimensions dropped ([R, H, W] for a 2-D domain); loads outside the image are 0; the residuals centred on an excluded pixel are returned
    but do not count in the cost (stencil_engine.h).  Graph energies: residuals is the pair (vertex residuals [RV, N], hyperedge residuals [RE, nE]).
    cost = 1/2 sum r^2."""
    P = problem.params
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    img = {im.name: im for im in ir.images}
    memo = {}
    if ir.kind == "stencil":
        shape = tuple(int(d) for d in problem.dims[:ir.ndim])[::-1]
        shape = (1,) * (3 - len(shape)) + shape      # (D, H, W)
        arrays = {im.name: f64(P[im.index]).reshape(shape + (im.channels,)) for im in ir.images}
        zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")

        def inb(off):
            dx, dy, dz = off
            return (xx + dx >= 0) & (xx + dx < shape[2]) & (yy + dy >= 0) & (yy + dy < shape[1]) & (zz + dz >= 0) & (zz + dz < shape[0])

        def load(name, c, where):
            dx, dy, dz = where[1]
            ok = inb(where[1])
            a = arrays[name][np.clip(zz + dz, 0, shape[0] - 1), np.clip(yy + dy, 0, shape[1] - 1), np.clip(xx + dx, 0, shape[2] - 1), c]
            return np.where(ok, a, 0.0)
        full = shape
    else:
        N = int(problem.dims[0])
        arrays = {im.name: f64(P[im.index]).reshape(N, im.channels) for im in ir.images}
        nE = int(np.asarray(P[ir.graph.index]))
        vidx = [np.asarray(P[i], dtype=np.int64).reshape(-1)[:nE] for _, i in ir.graph.slots]

        def inb(off):
            raise AssertionError("InBounds in a graph energy")

        def load(name, c, where):
            return arrays[name][:, c] if where[0] == "vertex" else arrays[name][vidx[where[1]], c]
        full = None

    def ev(n):
        r = memo.get(n.id)
        if r is not None:
            return r
        a = [ev(x) for x in n.args]
        op = n.op
        if op == "const":
            r = np.float64(n.val) if not n.cond else np.bool_(n.val != 0)
        elif op == "param":
            r = np.float64(np.asarray(P[n.val[1]], dtype=np.float32))      # Params are host floats
        elif op in ("uload", "iload"):
            r = load(*n.val)
        elif op == "inb":
            r = inb(n.val)
        elif op == "add":
            r = a[0] + a[1]
        elif op == "sub":
            r = a[0] - a[1]
        elif op == "mul":
            r = a[0] * a[1]
        elif op == "div":
            r = a[0] / a[1]
        elif op == "neg":
            r = -a[0]
        elif op == "sqrt":
            r = np.sqrt(a[0])
        elif op == "sin":
            r = np.sin(a[0])
        elif op == "cos":
            r = np.cos(a[0])
        elif op == "select":
            r = np.where(a[0], a[1], a[2])
        elif op == "cmp":
            r = {"eq": np.equal, "greater": np.greater, "greatereq": np.greater_equal, "less": np.less, "lesseq": np.less_equal}[n.val](a[0], a[1])
        elif op == "and":
            r = np.logical_and(a[0], a[1])
        elif op == "or":
            r = np.logical_or(a[0], a[1])
        elif op == "not":
            r = np.logical_not(a[0])
        else:
            raise AssertionError(op)
        memo[n.id] = r
        return r

    with np.errstate(all="ignore"):
        if ir.kind == "stencil":
            res = np.stack([np.broadcast_to(ev(r.node), full).astype(np.float64) for r in ir.residuals])
            keep = np.logical_not(np.broadcast_to(ev(ir.exclude), full)) if ir.exclude is not None else np.ones(full, bool)
            cost = 0.5 * float(np.sum(np.where(keep, np.sum(res * res, axis=0), 0.0)))
            return res.reshape((len(ir.residuals),) + full[3 - ir.ndim:]), cost
        rv = [np.broadcast_to(ev(r.node), (N,)).astype(np.float64) for r in ir.residuals if r.term == "vertex"]
        re_ = [np.broadcast_to(ev(r.node), (nE,)).astype(np.float64) for r in ir.residuals if r.term == "edge"]
        rv = np.stack(rv) if rv else np.zeros((0, N))
        re_ = np.stack(re_) if re_ else np.zeros((0, nE))
        return (rv, re_), 0.5 * float(np.sum(rv * rv) + np.sum(re_ * re_))


# =====================================================================================================================================================================
# Back end: the plug-in source
# =====================================================================================================================================================================
def _chain(var, values, fmt=str):
    """`var == 0 ? a : var == 1 ? b : ... : last` with runs of equal trailing values folded (a constexpr function body without tables)."""
    values = list(values)
    if len(set(values)) <= 1:
        return fmt(values[0]) if values else "0"
    while len(values) > 1 and values[-1] == values[-2]:
        values.pop()
    return " : ".join([f"{var} == {i} ? {fmt(v)}" for i, v in enumerate(values[:-1])] + [fmt(values[-1])])


def _lit(v):
    """A double literal that reads back as the same double (T(...) rounds it once to the working type, like a hand-written T(0.1))."""
    if v == int(v) and abs(v) < 1e15:
        return f"{int(v)}.0" if v >= 0 else f"-{int(-v)}.0"
    return repr(float(v))


class _Emitter:
    """Static single-assignment text of the DAG below some roots: one `const <type> tN = ...;` per load, per condition on the image (InBounds) and per node that
    more than one node reads; everything else is inlined into its one reader, fully parenthesised, in the order the .t wrote it."""

    def __init__(self, ir, mode):
        self.ir, self.mode = ir, mode      # mode: "pixel" | "excluded" | "vertex" | "edge"
        self.img = {im.name: im for im in ir.images}

    def ctype(self, n):
        return "bool" if n.cond else ("S" if n.dep else "T")

    def load(self, n):
        name, c, where = n.val
        im = self.img[name]
        if im.kind == "unknown":
            k = self.ir.k_of(im, c)
            if self.mode == "pixel":
                dx, dy, dz = where[1]
                return f"Xc({k})" if where[1] == (0, 0, 0) else f"Xc({k}, {dx}, {dy}, {dz})"
            return f"Xc({k})" if self.mode == "vertex" else f"Xc({where[1]}, {k})"
        ch = lambda i: (f"{im.channels} * {i} + {c}" if c else f"{im.channels} * {i}") if im.channels > 1 else i
        if self.mode in ("pixel", "excluded"):
            if where[1] == (0, 0, 0):
                return f"a_{name}[{ch('i')}]"
            dx, dy, dz = where[1]
            at = f"Xc.at({dx}, {dy}, {dz})"
            return f"({self.guard(where[1])} ? a_{name}[{ch(at)}] : T(0))"      # loads outside the image give 0
        return f"a_{name}[{ch('v' if self.mode == 'vertex' else 'v%d' % where[1])}]"

    def ref(self, n):
        return self.names.get(n.id) or self.expr(n)

    def guard(self, off):
        """The name of `is the pixel at this offset inside the image`, tested once per function."""
        if off not in self.guards:
            self.guards[off] = "b%d" % len(self.guards)
            self.lines.append("%sconst bool %s = Xc.in(%d, %d, %d);" % ((self.indent, self.guards[off]) + off))
        return self.guards[off]

    def as_type(self, n, want):
        s = self.ref(n)
        return f"S({s})" if want == "S" and self.ctype(n) == "T" else s

    def expr(self, n):
        op, a = n.op, n.args
        if op == "const":
            return ("true" if n.val else "false") if n.cond else f"T({_lit(n.val)})"
        if op == "param":
            return f"s_{n.val[0]}"
        if op in ("uload", "iload"):
            return self.load(n)
        if op == "inb":
            return self.guard(n.val)
        if op in ("add", "sub", "mul"):
            return f"({self.ref(a[0])} {'+-*'[('add', 'sub', 'mul').index(op)]} {self.ref(a[1])})"
        if op == "div":      # with an unknown below: a * (1 / b), the form the dual numbers' value takes, so that every pass forms the same residual bits
            return f"tg_div({self.ref(a[0])}, {self.ref(a[1])})" if n.dep else f"({self.ref(a[0])} / {self.ref(a[1])})"
        if op == "neg":
            return f"(-{self.ref(a[0])})"
        if op in ("sqrt", "sin", "cos"):
            return f"{op}({self.ref(a[0])})"
        if op == "select":
            t = self.ctype(n)
            return f"({self.ref(a[0])} ? {self.as_type(a[1], t)} : {self.as_type(a[2], t)})"
        if op == "cmp":      # a condition on an unknown's value takes valueOf
            side = lambda x: f"valueOf({self.ref(x)})" if x.dep else self.ref(x)
            return f"({side(a[0])} {_CMP[n.val]} {side(a[1])})"
        if op in ("and", "or"):
            return f"({self.ref(a[0])} {'&&' if op == 'and' else '||'} {self.ref(a[1])})"
        if op == "not":
            return f"(!{self.ref(a[0])})"
        raise AssertionError(op)

    def emit(self, roots, indent):
        """(lines, [text of each root])."""
        nodes = self.ir.reachable(roots)
        uses = {}
        for n in nodes:
            for x in n.args:
                uses[x.id] = uses.get(x.id, 0) + 1
        for r in roots:
            uses[r.id] = uses.get(r.id, 0) + 1
        self.names, self.lines, self.guards, self.indent = {}, [], {}, indent
        for n in nodes:      # ascending ids: the .t's own evaluation order
            if n.op in ("const", "param", "inb"):
                continue
            if n.op in ("uload", "iload") or uses.get(n.id, 0) > 1:
                text = self.expr(n)
                self.names[n.id] = f"t{n.id}"
                self.lines.append(f"{indent}const {self.ctype(n)} t{n.id} = {text};")
        texts = [self.ref(r) for r in roots]
        return self.lines, texts


def _functor_name(stem):
    return "Gen_" + stem


def emit_source(ir):
    """The text of the plug-in source for an IR whose body_hash is set."""
    assert ir.body_hash, "emit_source needs ir.body_hash (generate() sets it)"
    name = _functor_name(ir.stem)
    un = ir.unknowns
    K = ir.K()
    img_of = [im.img for im in un for _ in range(im.channels)]
    ch_of = [c for im in un for c in range(im.channels)]
    inputs = [im for im in ir.images if im.kind == "array"]
    members = []
    if inputs:
        members.append("    const T " + ", ".join("*a_" + im.name for im in inputs) + ";")
    if ir.params:
        members.append("    T " + ", ".join("s_" + p.name for p in ir.params) + ";")
    binds = []      # in binding order
    for im in ir.images:
        binds.append((im.index, f"X[{im.img}] = (const T*)p[{im.index}];" if im.kind == "unknown" else f"a_{im.name} = (const T*)p[{im.index}];"))
    for p in ir.params:
        binds.append((p.index, f"s_{p.name} = (T) * (const float*)p[{p.index}];"))
    if ir.graph:
        binds.append((ir.graph.index, f"nE = *(const int*)p[{ir.graph.index}];"))
        for j, (_, i) in enumerate(ir.graph.slots):
            binds.append((i, f"vidx[{j}] = (const int*)p[{i}];"))
    binds = ["        " + b for _, b in sorted(binds)]
    decls = []
    for im in ir.images:
        decls.append((im.index, f'{{ParamDecl::{"kUnknown" if im.kind == "unknown" else "kArray"}, "{im.name}", "{im.type or "opt_float"}", {im.index}}}'))
    for p in ir.params:
        decls.append((p.index, f'{{ParamDecl::kScalar, "{p.name}", "{p.type}", {p.index}}}'))
    if ir.graph:
        decls.append((ir.graph.index, f'{{ParamDecl::kGraphCount, "{ir.graph.name}", "int", {ir.graph.index}}}'))
        for sname, i in ir.graph.slots:
            decls.append((i, f'{{ParamDecl::kGraphIndex, "{ir.graph.name}.{sname}", "int", {i}}}'))
    decls = [d for _, d in sorted(decls)]
    common = [
        f"    static constexpr __host__ __device__ int imgOf(int k) {{ return {_chain('k', img_of)}; }}",
        f"    static constexpr __host__ __device__ int chOf(int k) {{ return {_chain('k', ch_of)}; }}",
        f"    static constexpr __host__ __device__ int channels(int img) {{ return {_chain('img', [im.channels for im in un])}; }}",
    ]
    unknown_param = f"    static int unknownParam(int img) {{ return {_chain('img', [im.index for im in un])}; }}"
    out = []
    w = out.append
    rel = os.path.basename(ir.path)
    w(f"// Generated by opt_amd/tgen.py from {rel} -- do not edit: edit the .t and generate again.")
    w(f"// An energy plug-in (include/OptAmdPlugin.h): {rel} served by the {'functor stencil engine' if ir.kind == 'stencil' else 'graph functor engine'}.")
    w("// No fused multiply-adds: the cost pass (S = T) and the derivative passes (S = dual numbers) must form the same residual bits.")
    w("#pragma clang fp contract(off)")
    w('#include "OptAmdPlugin.h"')
    if ir.kind == "stencil":
        w('#include "stencil_engine.h"      // cost, J^T F, J^T J p, model cost; three launches per PCG iteration, two with amd_stencil_fused = 1')
        w('#include "graph_pcg.h"           // (the flat pass of the two-launch iteration; stencil_engine.h includes it)')
    else:
        w('#include "graph_engine.h"')
        w('#include "graph_onchip.h"      // the whole linear solve of a small mesh in one workgroup (amd_onchip = 6)')
        w('#include "graph_onchip_grid.h" // ... and of a larger one as one launch of several workgroups (amd_onchip = 7, amd_onchip_workgroups)')
    w("")
    w("namespace optamd {      // (the functor's sqrt / sin / cos on S = T are the engine's overloads, found here)")
    w("namespace {")
    w("")
    w("// a / b where an unknown is below: a * (1 / b), as the dual numbers form their value (stencil_engine.h operator/)")
    w("template <class T> __device__ __forceinline__ T tg_div(T a, T b) { return a * (T(1) / b); }")
    w("template <class T, int N> __device__ __forceinline__ Dual<T, N> tg_div(const Dual<T, N>& a, const Dual<T, N>& b) { return a / b; }")
    w("template <class T, int N> __device__ __forceinline__ Dual<T, N> tg_div(const Dual<T, N>& a, T b) { return a / b; }")
    w("template <class T, int N> __device__ __forceinline__ Dual<T, N> tg_div(T a, const Dual<T, N>& b) { return a / b; }")
    w("")
    RV, RE = ir.counts()
    if ir.kind == "stencil":
        offs = ir.offsets()
        dep = ir.depends()
        R = len(ir.residuals)
        w(f"// {rel}: {len(un)} unknown image(s), {K} scalars and {R} residuals per pixel; unknowns are read at {len(offs)} offsets: {', '.join(str(o[:ir.ndim]) for o in offs)}.")
        w("template <class T>")
        w(f"struct {name} : StencilFunctorDefaults<T> {{")
        w(f'    static constexpr const char* kName = "{name}";')
        w(f"    static constexpr int NDIM = {ir.ndim}, NIMG = {len(un)}, K = {K}, R = {R}, NOFF = {len(offs)};")
        axes = " : ".join([f"a == {ax} ? ({_chain('i', [o[ax] for o in offs])})" for ax in range(2)] + [f"({_chain('i', [o[2] for o in offs])})"])
        w(f"    static constexpr __host__ __device__ int off(int i, int a) {{ return {axes}; }}")
        for line in common:
            w(line)
        masks = [sum(1 << oi for oi, d in enumerate(row) if d) for row in dep]
        w("    // bit oi of a row's mask: the residual carries a derivative w.r.t. the unknowns at offset oi")
        w(f"    static constexpr __host__ __device__ bool depends(int ri, int oi) {{ return (({_chain('ri', masks, lambda m: hex(m) + 'u')}) >> oi) & 1u; }}")
        w(unknown_param)
        w("    int W, H, D;")
        w("    const T* X[NIMG];")
        for m in members:
            w(m)
        w("    void bindParams(void** p) {")
        for b in binds:
            w(b)
        w("    }")
        if ir.exclude is not None:
            em = _Emitter(ir, "excluded")
            lines, (text,) = em.emit([ir.exclude], "        ")
            w("    __device__ bool excluded(int x, int y, int z) const {")
            w("        const long i = ((long)z * H + y) * W + x;")
            for line in lines:
                w(line)
            w(f"        return {text};")
            w("    }")
        em = _Emitter(ir, "pixel")
        lines, texts = em.emit([r.node for r in ir.residuals], "        ")
        w("    template <class S, class C>")
        w("    __device__ __forceinline__ void residuals(const C& Xc, int x, int y, int z, S* r) const {")
        w("        const long i = ((long)z * H + y) * W + x;")
        for line in lines:
            w(line)
        for ri, (r, text) in enumerate(zip(ir.residuals, texts)):
            w(f"        r[{ri}] = {text if r.node.dep else 'S(' + text + ')'};      // {rel}:{r.line}")
        w("    }")
        w("};")
        info = f"stencilEnergyInfo<{name}, {'true' if ir.use_preconditioner else 'false'}>"
    else:
        V = len(ir.graph.slots)
        ed = ir.edge_depends()
        w(f"// {rel}: {len(un)} unknown image(s), {K} scalars per vertex; {RV} residuals per vertex, {RE} per hyperedge of {V} vertices.  The tuning constants of the")
        w("// on-chip solves are GraphFunctorDefaults'.")
        w("template <class T>")
        w(f"struct {name} : GraphFunctorDefaults {{")
        w(f'    static constexpr const char* kName = "{name}";')
        w(f"    static constexpr int NIMG = {len(un)}, K = {K}, V = {V}, RV = {RV}, RE = {RE};")
        for line in common:
            w(line)
        masks = [sum(1 << (j * K + k) for j in range(V) for k in range(K) if t[j][k]) for t in ed]
        if V * K > 63:
            raise TgenError(ir.path, ir.residuals[0].line, f"unsupported: {V} slots of {K} unknown scalars (the pruning mask holds 63 bits)")
        if not masks or all(m == (1 << (V * K)) - 1 for m in masks):
            w("    static constexpr __host__ __device__ bool edgeDepends(int, int, int) { return true; }")
        else:
            w("    // bit j * K + k of a row's mask: the hyperedge residual carries a derivative w.r.t. unknown k of slot j")
            w(f"    static constexpr __host__ __device__ bool edgeDepends(int ri, int j, int k) {{ return (({_chain('ri', masks, lambda m: hex(m) + 'ul')}) >> (j * K + k)) & 1ul; }}")
        w(unknown_param)
        w("    long N; int nE; const int* vidx[V]; const T* X[NIMG];")
        for m in members:
            w(m)
        w("    void bindParams(void** p) {")
        for b in binds:
            w(b)
        w("    }")
        for term, sig in (("vertex", "vertexResiduals(const C& Xc, long v, S* r)"), ("edge", "edgeResiduals(const C& Xc, long e, S* r)")):
            rows = [r for r in ir.residuals if r.term == term]
            em = _Emitter(ir, term)
            lines, texts = em.emit([r.node for r in rows], "        ")
            w(f"    template <class S, class C> __device__ __forceinline__ void {sig} const {{")
            if term == "edge":
                used = sorted({n.val[2][1] for n in ir.reachable([r.node for r in rows]) if n.op == "iload"})
                for j in used:
                    w(f"        const long v{j} = vidx[{j}][e];")
            for line in lines:
                w(line)
            for ri, (r, text) in enumerate(zip(rows, texts)):
                w(f"        r[{ri}] = {text if r.node.dep else 'S(' + text + ')'};      // {rel}:{r.line}")
            w("    }")
        w("};")
        info = f"graphEnergyInfo<{name}, {'true' if ir.use_preconditioner else 'false'}>"
    w("")
    w(f"EnergyInfo {name}_info() {{")
    w(f'    EnergyInfo e = {info}("{ir.stem}");')
    w("    e.params = {" + ",\n                ".join(decls) + "};")
    w(f'    e.bodyHashes = {{0x{ir.body_hash:016x}ul}};     // OptAmd_ProblemFileHash("{rel}")')
    w("    return e;")
    w("}")
    w("")
    w("}  // namespace")
    w("}  // namespace optamd")
    w("")
    w(f"OPTAMD_ENERGY_PLUGIN(optamd::{name}_info)")
    return "\n".join(out) + "\n"


# =====================================================================================================================================================================
# Interface
# =====================================================================================================================================================================
class GeneratedEnergy:
    def __init__(self, name, kind, hip_path, ir):
        self.name, self.kind, self.hip_path, self.ir = name, kind, hip_path, ir

    def __repr__(self):
        return f"GeneratedEnergy(name={self.name!r}, kind={self.kind!r}, hip_path={self.hip_path!r})"


def generate(t_path, out_dir=None):
    """Translate t_path into <out_dir>/<stem>.hip (default opt_amd/build_plugins/gen/).  The energy's name is the .t stem.  The source is rewritten only when its
    text changes, so a library built from it stays up to date."""
    from . import api
    ir = parse(t_path)
    ir.body_hash = api.problem_file_hash(ir.path)
    if not ir.body_hash:
        raise TgenError(ir.path, 1, "the file could not be hashed")
    out_dir = os.path.abspath(out_dir or GEN_DIR)
    os.makedirs(out_dir, exist_ok=True)
    hip = os.path.join(out_dir, ir.stem + ".hip")
    text = emit_source(ir)
    if not os.path.exists(hip) or open(hip).read() != text:
        with open(hip, "w") as f:
            f.write(text)
    return GeneratedEnergy(ir.stem, ir.kind, hip, ir)


def compile_energy(t_path, force=True, out=None):
    """generate, then build.build_plugin into opt_amd/lib/plugins/lib<stem>.so (or `out`); returns that path.  force=False: only if the source, which is rewritten
    only when the .t changes it, or a header is newer than the library.  A .t whose stem a hand-written plug-in source already has (the two samples) lands on that
    plug-in's library path: give such a library another place with `out`."""
    from . import build
    g = generate(t_path)
    return build.build_plugin(g.hip_path, out=out, force=force)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m opt_amd.tgen", description="Generate (and build) an energy plug-in from a .t file of the documented subset.")
    ap.add_argument("t_file")
    ap.add_argument("--emit-only", action="store_true", help="write the plug-in source and print its path; do not compile")
    ap.add_argument("--out", metavar="DIR", help="where the source goes (with --emit-only) or the library (default: opt_amd/lib/plugins)")
    a = ap.parse_args(argv)
    try:
        if a.emit_only:
            print(generate(a.t_file, a.out).hip_path)
            return 0
        g = generate(a.t_file)
        from . import build
        out = os.path.join(os.path.abspath(a.out), f"lib{g.name}.so") if a.out else None
        if out:
            os.makedirs(os.path.dirname(out), exist_ok=True)
        print(build.build_plugin(g.hip_path, out=out))
        return 0
    except TgenError as e:
        sys.stderr.write(f"tgen: {e}\n")
        return 1


if __name__ == "__main__":
    sys.exit(main())
