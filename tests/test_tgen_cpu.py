"""CPU tests (no GPU needed) of opt_amd/tgen.py: the front end against the CPU oracle and against the numpy restatements of the two samples, the tables it derives,
the source it emits (body hash, shared nodes), the cross-compilation of the six energies the GPU tests run, and the refusals.

No plug-in is loaded in the pytest process (the registry is process-global): the loader runs in a fresh child (tests/tgen_driver.py)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tgen_cases as tc
from opt_amd import build, tgen, workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "tgen_driver.py")
CSRC = build.CSRC


def child(case, args=None, timeout=120):
    e = dict(os.environ)
    e.pop("OPT_AMD_ENERGY_PLUGINS", None)
    r = subprocess.run([sys.executable, DRIVER, case, json.dumps(args or {})], capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---- the front end against the oracle --------------------------------------------------------------------------------------------------------------------------
def _laplacian(W, H):
    P = wl.laplacian(W, H, seed=2)
    P.params = [np.asarray(p, np.float64) for p in P.params]
    P.params[0] = P.params[0] + 0.1 * np.random.default_rng(3).standard_normal(P.params[0].shape)      # (the generator starts at the target: every fit residual 0)
    P.double = True
    return P


ORACLE_CASES = {
    "image_warping-13x9": lambda: wl.image_warping(13, 9, double=True, random_state=3, mask_fraction=0.2, perturb=0.3, jitter_urshape=0.2),
    "image_warping-5x3": lambda: wl.image_warping(5, 3, double=True, random_state=4, mask_fraction=0.2, perturb=0.3, jitter_urshape=0.2),
    "poisson_image_editing-13x9": lambda: wl.poisson_image_editing(13, 9, double=True, seed=1),
    "poisson_image_editing-5x3": lambda: wl.poisson_image_editing(5, 3, double=True, seed=1),
    "laplacian-13x9": lambda: _laplacian(13, 9),
    "laplacian-5x3": lambda: _laplacian(5, 3),
    "volumetric_mesh_deformation-5x4x4": lambda: wl.volumetric_mesh_deformation(5, 4, 4, double=True, seed=5, perturb=0.05),
    "arap_mesh_deformation-7x5": lambda: wl.arap_mesh_deformation(7, 5, double=True, seed=1, perturb=0.05),
    "embedded_mesh_deformation-7x5": lambda: wl.embedded_mesh_deformation(7, 5, double=True, seed=1, perturb=0.05),
    "cotangent_mesh_smoothing-7x5": lambda: wl.cotangent_mesh_smoothing(7, 5, double=True, seed=1),
    "robust_nonrigid_alignment-7x5": lambda: wl.robust_nonrigid_alignment(7, 5, double=True, seed=1, perturb=0.05),
}
# the registry's residualsPerElement / residualsPerEdge: where the entry states them, the entry's line; for the functor energies the functor's constants (what
# stencilEnergyInfo / graphEnergyInfo put into the entry of a plug-in); laplacian's entry states none -- its three Energy lines are scalar
REGISTRY_SOURCE = {"image_warping": "energy_image_warping.hip", "poisson_image_editing": "energy_poisson.hip", "arap_mesh_deformation": "energy_graph.hip",
                   "volumetric_mesh_deformation": ("energy_functors.hip", "VolumetricE"), "cotangent_mesh_smoothing": ("energy_graph_functors.hip", "CotangentG"),
                   "embedded_mesh_deformation": ("energy_graph_functors.hip", "EmbeddedG"), "robust_nonrigid_alignment": ("energy_graph_functors.hip", "RobustG")}


def registry_counts(energy):
    if energy == "laplacian":
        return 3, 0
    src = REGISTRY_SOURCE[energy]
    if isinstance(src, str):
        line = next(l for l in open(os.path.join(CSRC, src)) if 'e.name = "%s"' % energy in l)
        per = re.search(r"residualsPerElement = (\d+)", line)
        edge = re.search(r"residualsPerEdge = (\d+)", line)
        return int(per.group(1)), int(edge.group(1)) if edge else 0
    text = open(os.path.join(CSRC, src[0])).read()
    body = text[text.index("struct %s " % src[1]):]
    m = re.search(r"static constexpr int [^;]*?\bRV = (\d+), RE = (\d+)", body) or re.search(r"static constexpr int [^;]*?\bR = (\d+)", body)
    return int(m.group(1)), int(m.group(2)) if m.lastindex == 2 else 0


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_the_front_end_against_the_oracle(oracle_lib, opt_lib, case):
    """tgen.evaluate of the project's own .t on small inputs in double against the oracle's eval_cost on the same arrays: 1e-12 relative, the project's double
    bar; as many residuals as the registry states."""
    P = ORACLE_CASES[case]()
    ir = tgen.parse(opt_lib.energy_file(P.energy))
    res, cost = tgen.evaluate(ir, P)
    o = oracle_lib.OracleSolver(P.energy, "gaussNewtonGPU", True, P.dims)
    ref = o.eval_cost(P.params)
    o.close()
    err = abs(cost - ref) / abs(ref)
    print(case, cost, ref, "rel", err)
    assert ref > 0 and err <= 1e-12, (cost, ref, err)
    assert ir.counts() == registry_counts(P.energy), (ir.counts(), registry_counts(P.energy))
    if ir.kind == "stencil":
        assert res.shape == (ir.counts()[0],) + tuple(P.dims)[::-1]
    else:
        assert res[0].shape == (ir.counts()[0], P.dims[0]) and res[1].shape == (ir.counts()[1], P.meta["n_edges"])


# ---- the two samples against their numpy restatements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["13x9-block", "13x9-border", "13x9-nomask", "70x5-block", "1x7-nomask", "7x1-border"])
def test_vector_tv_against_its_numpy_restatement(name):
    import stencil_plugin_cases as sc
    P = sc.problem(sc.case(name), True)
    m = sc.Model(P)
    ir = tgen.parse(wl.VECTOR_TV_T)
    res, cost = tgen.evaluate(ir, P)
    H, W = m.H, m.W
    want = np.zeros((4, H, W))
    want[0], want[1] = m.F0[..., 0], m.F0[..., 1]
    want[2][:, :-1] = m.Fx      # 0 where the forward neighbour is outside: Select(InBounds(dx,dy), ., 0)
    want[3][:-1, :] = m.Fy
    assert res.shape == want.shape
    assert np.max(np.abs(res - want)) <= 1e-12 * np.max(np.abs(want))
    assert abs(cost - m.cost()) <= 1e-12 * m.cost(), (cost, m.cost())


def test_spring_against_its_numpy_restatement():
    import plugin_energy_driver as drv
    from test_plugin_energy_gpu import residuals_and_jacobian
    P = drv.problem("grid", True)
    X = np.asarray(P.params[0], np.float64)
    F, _ = residuals_and_jacobian(P, X)
    ir = tgen.parse(wl.SPRING_T)
    (rv, re_), cost = tgen.evaluate(ir, P)
    N = len(X)
    assert rv.shape == (3, N) and re_.shape == (1, P.meta["n_edges"])
    got = np.concatenate([rv.T.reshape(-1), re_[0]])
    assert np.max(np.abs(got - F)) <= 1e-12 * np.max(np.abs(F))
    assert abs(cost - 0.5 * float(F @ F)) <= 1e-12 * cost


# ---- derived tables --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_derived_for_vector_tv(opt_lib, tmp_path):
    ir = tgen.parse(wl.VECTOR_TV_T)
    assert ir.kind == "stencil" and ir.ndim == 2
    assert ir.offsets() == [(0, 0, 0), (1, 0, 0), (0, 1, 0)]      # centre first
    assert ir.counts() == (4, 0) and ir.K() == 2 and len(ir.unknowns) == 1
    hand = lambda ri, oi: oi == 0 or (ri >= 2 and ri - 1 == oi)      # examples/plugins/vector_tv_denoising.hip depends()
    assert ir.depends() == [[hand(ri, oi) for oi in range(3)] for ri in range(4)]
    assert ir.use_preconditioner and ir.exclude is not None
    text = open(tgen.generate(wl.VECTOR_TV_T, str(tmp_path)).hip_path).read()
    assert "NDIM = 2, NIMG = 1, K = 2, R = 4, NOFF = 3;" in text and 'kName = "Gen_vector_tv_denoising"' in text
    assert "stencilEnergyInfo<Gen_vector_tv_denoising, true>(\"vector_tv_denoising\")" in text
    # the ParamDecl table of the hand-written source, entry for entry
    hand_src = open(build.SAMPLE_STENCIL_PLUGIN).read()
    decl = lambda s: re.findall(r'\{ParamDecl::(\w+), "([\w.]+)", "(\w+)", (\d+)\}', s)
    assert decl(text) == decl(hand_src) and len(decl(text)) == 6
    assert "#pragma clang fp contract(off)" in text and "OPTAMD_ENERGY_PLUGIN(optamd::Gen_vector_tv_denoising_info)" in text


def test_the_tables_derived_for_the_mesh_energies(opt_lib, tmp_path):
    ir = tgen.parse(opt_lib.energy_file("cotangent_mesh_smoothing"))
    assert ir.kind == "graph" and len(ir.graph.slots) == 4 and ir.counts() == (3, 3) and ir.K() == 3
    assert all(all(all(row) for row in t) for t in ir.edge_depends())      # the weight couples every component of all four vertices
    ir = tgen.parse(opt_lib.energy_file("embedded_mesh_deformation"))
    assert ir.counts() == (9, 3) and ir.K() == 12 and len(ir.graph.slots) == 2
    hand = lambda ri, j, k: (k == ri) if k < 3 else (j == 0 and (k - 3) // 3 == ri)      # energy_graph_functors.hip EmbeddedG::edgeDepends
    assert ir.edge_depends() == [[[hand(ri, j, k) for k in range(12)] for j in range(2)] for ri in range(3)]
    text = open(tgen.generate(wl.SPRING_T, str(tmp_path)).hip_path).read()
    assert "NIMG = 1, K = 3, V = 2, RV = 3, RE = 1;" in text and "graphEnergyInfo<Gen_spring_mesh_deformation, true>" in text
    decl = lambda s: re.findall(r'\{ParamDecl::(\w+), "([\w.]+)", "(\w+)", (\d+)\}', s)
    assert decl(text) == decl(open(build.SAMPLE_PLUGIN).read()) and len(decl(text)) == 8
    # bindParams in binding order
    binds = re.findall(r"p\[(\d+)\]", text[text.index("void bindParams"):text.index("vertexResiduals")])
    assert binds == [str(i) for i in range(8)]


# ---- body hash and shared nodes --------------------------------------------------------------------------------------------------------------------------------
def test_the_body_hash_and_shared_nodes(opt_lib, tmp_path):
    t = tc.t_file("gen_image_warping", tmp_path)
    g = tgen.generate(t, str(tmp_path / "out"))
    assert (g.name, g.kind) == ("gen_image_warping", "stencil") and g.hip_path == str(tmp_path / "out" / "gen_image_warping.hip") and g.ir.stem == g.name
    text = open(g.hip_path).read()
    h = opt_lib.problem_file_hash(t)
    assert h and "e.bodyHashes = {0x%016xul};" % h in text
    assert h == opt_lib.problem_file_hash(opt_lib.energy_file("image_warping"))      # the copy has the built-in file's body
    # inShape = eq(Mask(0,0), 0) is read by Exclude and by the four `usable` conditions: inside residuals() the load and the comparison are emitted once
    body = text[text.index("void residuals("):]
    body = body[:body.index("\n    }\n")]
    assert len(re.findall(r"= a_Mask\[i\];", body)) == 1
    shared = re.findall(r"const bool (t\d+) = \(t\d+ == T\(0\.0\)\);", body)
    assert len(shared) == 1 and len(re.findall(r"&& %s\)" % shared[0], body)) == 4      # ... into one name that all four read
    # sin and cos of the angle once each, whatever the number of offsets
    assert len(re.findall(r"= cos\(", body)) == 1 and len(re.findall(r"= sin\(", body)) == 1
    # written again only when the text changes
    m = os.path.getmtime(g.hip_path)
    os.utime(g.hip_path, (m - 100, m - 100))
    tgen.generate(t, str(tmp_path / "out"))
    assert os.path.getmtime(g.hip_path) == m - 100


# ---- compilation -----------------------------------------------------------------------------------------------------------------------------------------------
STENCIL_KERNELS = ["se_cost<%(p)s, %(E)s >", "se_modelCost<%(p)s, %(E)s >", "se_gather<%(p)s, %(E)s, false>", "se_gather<%(p)s, %(E)s, true>"] + \
    ["se_gatherIter<%%(p)s, %%(E)s, %s, %s>" % (lm, pre) for lm in ("false", "true") for pre in ("false", "true")]


@pytest.fixture(scope="module")
def six(opt_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tgen")
    return tmp, tc.build_all(tmp, jobs=4, force=False)


@pytest.mark.parametrize("name", tc.SIX)
def test_the_generated_source_compiles_for_gfx950_without_scratch(six, name):
    """plugin_kernel_resources lists every engine kernel for the generated functor in float and double with 0 bytes of scratch -- except variants in which the
    hand-written functor of the same energy spills too (its own remarks, or for a built-in functor the library's)."""
    tmp, libs = six
    assert libs[name] == tc.library_path(name) and os.path.exists(libs[name])
    res = build.plugin_kernel_resources(tc.remarks_stem(name))
    functor = "Gen_" + name
    assert res, tc.remarks_stem(name)
    stencil = name in tc.IMAGE_ENERGIES
    for prec in ("float", "double"):
        E = "%s<%s>" % (functor, prec)
        mine = [k for k in res if E in k]
        if stencil:
            for w in STENCIL_KERNELS:
                w = w % {"p": prec, "E": E}
                assert len([k for k in res if k.endswith(w)]) == 1, (w, sorted(res))
            assert len(mine) == 8
        else:      # the launch-per-iteration kernels, the one-workgroup solve and the grid solve, Gauss-Newton and Levenberg-Marquardt
            for kernel in ("ge_vertices<", "ge_edges<", "ge_gather<", "ge_onchipPcg<", "ge_onchipPcgGrid<"):
                assert [k for k in mine if kernel in k], (kernel, sorted(mine))
    hand = {}
    if name in tc.SAMPLES:
        hand_functor = {"vector_tv_denoising": "VectorTvE", "spring_mesh_deformation": "SpringG"}[name]
        build.build_plugin({"vector_tv_denoising": build.SAMPLE_STENCIL_PLUGIN, "spring_mesh_deformation": build.SAMPLE_PLUGIN}[name], force=False)
        hand = {k.replace(hand_functor, functor): v for k, v in build.plugin_kernel_resources(name).items()}
        assert set(hand) == set(res), set(hand) ^ set(res)
    elif name in tc.KEY and name != "gen_arap_mesh_deformation":
        hand_functor = {"gen_embedded_mesh_deformation": "EmbeddedG", "gen_cotangent_mesh_smoothing": "CotangentG"}[name]
        hand = {k.replace("optamd::", "").replace(hand_functor, functor): v for k, v in build.kernel_resources().items() if hand_functor in k}
    for k, v in sorted(res.items()):
        spills_too = k in hand and hand[k]["scratch"] > 0
        print(k, "vgprs", v["vgprs"], "scratch", v["scratch"], "| hand-written:", hand.get(k, {}).get("vgprs"), hand.get(k, {}).get("scratch"))
        assert v["scratch"] == 0 or spills_too, (k, v, hand.get(k))
    und = subprocess.run(["nm", "-D", "--undefined-only", libs[name]], capture_output=True, text=True).stdout
    assert "optamd" not in und and "OptAmd_" not in und and "Opt_" not in und, und


def test_the_loader_accepts_the_six_and_their_t_files(six, opt_lib):
    """In a child: all six libraries load beside the built-in twelve, and OptAmd_CheckProblemFile says ok for each .t -- the derived ParamDecl table, the
    UsePreconditioner flag and the recorded hash are what the library's own reading of the file expects."""
    tmp, libs = six
    files = {n: tc.t_file(n, tmp) for n in tc.SIX}
    out = child("check", {"plugins": [libs[n] for n in tc.SIX], "files": files})
    assert out["n"] == [1] * 6 and out["names"] == out["before"] + tc.SIX and len(out["before"]) == 12
    for n in tc.SIX:
        assert out["check"][n] == [True, "ok: " + n], (n, out["check"][n])
        assert out["hash"][n] in open(os.path.join(tgen.GEN_DIR, n + ".hip")).read()


def test_an_edited_energy_line_needs_a_new_library(six, opt_lib, tmp_path):
    """An edited Energy line regenerates with a new hash, and the old library refuses the edited file (in a child)."""
    tmp, libs = six
    t = tc.t_file("gen_embedded_mesh_deformation", tmp)
    src = open(t).read()
    edited = src.replace("Energy(w_rotSqrt * Dot3(col[1], col[2]))", "Energy(2 * w_rotSqrt * Dot3(col[1], col[2]))")
    assert edited != src
    t2 = str(tmp_path / "gen_embedded_mesh_deformation.t")
    open(t2, "w").write(edited)
    old = open(os.path.join(tgen.GEN_DIR, "gen_embedded_mesh_deformation.hip")).read()
    new = open(tgen.generate(t2, str(tmp_path / "out")).hip_path).read()
    h = lambda s: re.search(r"e\.bodyHashes = \{(0x[0-9a-f]{16})ul\};", s).group(1)
    assert h(old) != h(new) and int(h(new), 16) == opt_lib.problem_file_hash(t2)
    assert "T(2.0) * s_w_rotSqrt" in new and "T(2.0) * s_w_rotSqrt" not in old
    out = child("check", {"plugins": [libs["gen_embedded_mesh_deformation"]], "files": {"own": t, "edited": t2}})
    assert out["check"]["own"][0] and not out["check"]["edited"][0] and "hash" in out["check"]["edited"][1], out["check"]


def test_the_inputs_of_the_gpu_tests_build_and_evaluate(opt_lib, tmp_path):
    """Every input tests/test_tgen_gpu.py hands to a child builds on the host and gives a finite, non-zero cost under tgen.evaluate, in float and double inputs."""
    for name in tc.SIX:
        ir = tgen.parse(tc.t_file(name, tmp_path))
        for inp in tc.inputs_of(name):
            for double in (True, False):
                _, cost = tgen.evaluate(ir, tc.problem(name, inp, double))
                assert np.isfinite(cost) and cost > 0, (name, inp, double, cost)
    t = str(tmp_path / (tc.ROUND_TRIP_STEM + ".t"))
    open(t, "w").write(tc.ROUND_TRIP_T)
    P = tc.round_trip_problem(True)
    ir = tgen.parse(t)
    assert ir.counts() == (3, 4)
    F, _ = tc.round_trip_residuals_and_jacobian(P, np.asarray(P.params[0], np.float64))
    _, cost = tgen.evaluate(ir, P)
    assert abs(cost - 0.5 * float(F @ F)) <= 1e-12 * cost


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
HEAD2 = 'local W, H = Dim("W", 0), Dim("H", 1)\nlocal X = Unknown("X", opt_float2, {W,H}, 0)\nlocal A = Array("A", opt_float2, {W,H}, 1)\nlocal w = Param("w", float, 2)\n'
HEAD1 = 'local N = Dim("N", 0)\nlocal X = Unknown("X", opt_float3, {N}, 0)\nlocal A = Array("A", opt_float3, {N}, 1)\n'
GRAPH = 'local G = Graph("G", 2, "v0", {N}, 3, "v1", {N}, 4)\n'
REFUSALS = {      # name: (text, the line the error names, a word of the message)
    "ComputedArray": (HEAD2 + 'local C = ComputedArray("C", {W,H}, X(0,0)(0) * X(0,0)(0))\nEnergy(X(0,0) - A(0,0))\n', 5, "ComputedArray"),
    "L_p": (HEAD2 + "Energy(L_p(X(0,0) - X(1,0), X(0,0) - X(1,0), 0.8, {W,H}))\n", 5, "L_p"),
    "SampledImage": (HEAD2 + "local S = SampledImage(A, A, A)\nEnergy(X(0,0) - A(0,0))\n", 5, "SampledImage"),
    "pow": (HEAD2 + "Energy(X(0,0) - A(0,0))\nEnergy(pow(X(0,0)(0), 2))\n", 6, "pow"),
    "exp": (HEAD2 + "Energy(exp(X(0,0)(0)))\n", 5, "exp"),
    "log": (HEAD2 + "Energy(\n  w * log(X(0,0)(0)))\n", 6, "log"),
    "while": (HEAD2 + "local i = 0\nwhile i < 2 do i = i + 1 end\nEnergy(X(0,0) - A(0,0))\n", 6, "while"),
    "require": (HEAD2 + 'local m = require("helpers")\nEnergy(X(0,0) - A(0,0))\n', 5, "require"),
    "graph_on_2d": (HEAD2 + 'local G = Graph("G", 3, "v0", {W,H}, 4, "v1", {W,H}, 5)\nEnergy(X(G.v0) - X(G.v1))\n', 5, "Graph"),
    "two_graphs": (HEAD1 + GRAPH + 'local G2 = Graph("G2", 5, "v0", {N}, 6, "v1", {N}, 7)\nEnergy(X(G.v0) - X(G2.v1))\n', 5, "more than one Graph"),
    "vertex_term_offset": (HEAD1 + GRAPH + "Energy(X(0) - X(1))\n", 5, "non-zero offset"),
    "offset_not_literal": (HEAD2 + "local d = X(0,0)(0)\nEnergy(X(0,0) - X(d,0))\n", 6, "literal"),
    "1d_without_graph": (HEAD1 + "Energy(X(0) - A(0))\n", 4, "without a Graph"),
    "reads_no_unknown": (HEAD2 + "Energy(X(0,0) - A(0,0))\nEnergy(w * A(0,0))\n", 6, "no unknown"),
    "if_on_an_expression": (HEAD2 + "if X(0,0)(0) > 0 then Energy(X(0,0)) end\n", 5, "generation time"),
    "unknown_name": (HEAD2 + "Energy(frobnicate(X(0,0)))\n", 5, "frobnicate"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_line(tmp_path, name):
    text, line, word = REFUSALS[name]
    t = str(tmp_path / "refused.t")
    open(t, "w").write(text)
    with pytest.raises(tgen.TgenError) as e:
        tgen.parse(t)
    print(e.value)
    assert e.value.line == line and word in e.value.what and str(e.value).startswith("refused.t:%d: " % line), str(e.value)


def test_the_project_s_other_t_files_are_refused_with_a_reason(opt_lib):
    """optical_flow (SampledImage), intrinsic_image_decomposition (a Param that is not a float, then L_p), shape_from_shading (string concatenation in a loop of
    declarations, ComputedArray) and curveFitting (two index spaces) are outside the subset: a TgenError, not a wrong functor."""
    for e in ("optical_flow", "intrinsic_image_decomposition", "shape_from_shading", "curveFitting"):
        with pytest.raises(tgen.TgenError) as err:
            tgen.parse(opt_lib.energy_file(e))
        assert err.value.line >= 1 and err.value.what, e


def test_the_command_line_emits_and_refuses(opt_lib, tmp_path):
    r = subprocess.run([sys.executable, "-m", "opt_amd.tgen", wl.SPRING_T, "--emit-only", "--out", str(tmp_path)], capture_output=True, text=True, cwd=tc.ROOT)
    assert r.returncode == 0 and r.stdout.strip() == str(tmp_path / "spring_mesh_deformation.hip") and os.path.exists(r.stdout.strip()), (r.stdout, r.stderr)
    t = str(tmp_path / "refused.t")
    open(t, "w").write(REFUSALS["pow"][0])
    r = subprocess.run([sys.executable, "-m", "opt_amd.tgen", t, "--emit-only", "--out", str(tmp_path)], capture_output=True, text=True, cwd=tc.ROOT)
    assert r.returncode == 1 and "refused.t:6: " in r.stderr and "pow" in r.stderr and not os.path.exists(str(tmp_path / "refused.hip"))
