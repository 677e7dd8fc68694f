"""CPU tests (-m "not gpu") of the graph-shape cases: the inputs test_graph_shapes_gpu.py feeds the HIP kernels are what they claim to be, and the oracle
those tests lean on is pinned on the new shapes first -- it does not depend on the hyperedge order, and its J^T F is the gradient of its cost also where a
hyperedge names one vertex twice, a vertex has no hyperedge, or a half-edge is repeated."""
from collections import Counter

import numpy as np
import pytest

import graph_cases as gc
from helpers import oracle_solver, rel_err
from test_oracle import _fd_gradient

HOWS = ("shuffle", "reverse", "interleave")
ORDER_CASES = [(e, "armadillo", how) for e in gc.ENERGIES for how in HOWS] + [(e, "raptor", "shuffle") for e in gc.ENERGIES]


def _tuples(P):
    return Counter(zip(*[c.tolist() for c in gc.index_arrays(P)]))


@pytest.mark.parametrize("energy,mesh,how", ORDER_CASES)
def test_reorder_is_a_permutation(energy, mesh, how):
    P = gc.base_problem(energy, mesh, True)
    Q = gc.reorder(P, how, seed=1)
    assert _tuples(P) == _tuples(Q)
    assert int(Q.params[gc.layout(Q)["count"]]) == int(P.params[gc.layout(P)["count"]]) == len(gc.index_arrays(Q)[0])
    assert any(not np.array_equal(a, b) for a, b in zip(gc.index_arrays(P), gc.index_arrays(Q)))
    for s in gc.layout(P)["vertex"]:
        assert np.array_equal(P.params[s], Q.params[s])


@pytest.mark.parametrize("mesh", ["armadillo", "raptor", "open_patch"])
def test_interleave_leaves_no_run_longer_than_one(mesh):
    """Round-robin over heads: two consecutive hyperedges share a head only in the tail where a single head is left (ranks at or beyond the second-largest valence)."""
    P = gc.base_problem("embedded", mesh, True)
    heads = gc.reorder(P, "interleave").params[gc.layout(P)["idx"][0]]
    val = np.sort(np.bincount(heads))
    rank = np.zeros(len(heads), dtype=np.int64)
    seen = Counter()
    for i, h in enumerate(heads.tolist()):
        rank[i] = seen[h]; seen[h] += 1
    same = np.flatnonzero(heads[1:] == heads[:-1]) + 1
    assert np.all(rank[same] >= val[-2])
    if val[-1] - val[-2] <= 1:
        assert len(same) == 0
    assert mesh == "open_patch" or len(same) == 0      # the two closed meshes have several vertices of the largest valence


def test_the_ordered_graphs_are_grouped_by_head_and_the_meshes_are_what_the_cases_say():
    for mesh, nv, ne, vmin, vmax in (("armadillo", 130, 768, 3, 10), ("raptor", 2000, 12108, 3, 12), ("armadillo_sub", 386, 2304, 3, 10), ("open_patch", 35, 164, 2, 6)):
        P = gc.base_problem("arap" if mesh != "open_patch" else "cotangent", mesh, True)
        heads = gc.index_arrays(P)[0]
        deg = np.bincount(heads, minlength=nv)
        assert gc.n_vertices(P) == nv and len(heads) == ne and np.all(np.diff(heads) >= 0)
        assert deg.min() >= vmin and deg.max() <= vmax, (mesh, deg.min(), deg.max())
    P = gc.base_problem("cotangent", "open_patch", True)
    assert int(np.sum(P.params[7] == P.params[8])) == 4      # v2 == v3 at the two valence-2 corners


COTANGENT_SHAPES = {
    "armadillo": lambda: gc.base_problem("cotangent", "armadillo", True),
    "armadillo_sub": lambda: gc.base_problem("cotangent", "armadillo_sub", True),
    "raptor": lambda: gc.base_problem("cotangent", "raptor", True),
    "open_patch": lambda: gc.base_problem("cotangent", "open_patch", True),
    "hub300": lambda: gc.with_hub(gc.base_problem("cotangent", "armadillo_sub", True), 300),
    "tail_only": lambda: gc.with_tail_only_vertex(gc.base_problem("cotangent", "armadillo", True)),
    "isolated": lambda: gc.with_isolated_vertex(gc.base_problem("cotangent", "armadillo", True)),
    "duplicates": lambda: gc.with_duplicate_edges(gc.base_problem("cotangent", "armadillo", True), 9),
}


@pytest.mark.parametrize("name", sorted(COTANGENT_SHAPES))
def test_cotangent_guard_margins(name):
    """Every |w| and every discriminant of every cotangent input is at least 1e-4 at the start: two correct implementations cannot take different branches of the
    .t's guards (cotangent_mesh_smoothing.t:25, 33) at either precision, so no GPU test passes or fails by luck."""
    w, disc, _ = gc.cotangent_margins(COTANGENT_SHAPES[name]())
    print(f"{name}: min |w| = {w:.3g}, min disc = {disc:.3g}")
    assert w >= 1e-4 and disc >= 1e-4


@pytest.mark.parametrize("mesh", ["armadillo", "raptor"])
def test_cotangent_guard_is_covered(mesh):
    """More than 5 % of the hyperedges take the w <= 0 branch (none does on the generated torus)."""
    share = gc.cotangent_margins(gc.base_problem("cotangent", mesh, True))[2]
    print(f"{mesh}: {100 * share:.1f} % of the hyperedges have w <= 0")
    assert share > 0.05


def _stages(o, P, v):
    f, d = o.eval_jtf(P.params)
    return o.eval_cost(P.params), f, d, o.apply_jtj(P.params, v)


@pytest.mark.parametrize("energy,mesh,how", ORDER_CASES)
def test_oracle_does_not_depend_on_the_hyperedge_order(oracle_lib, energy, mesh, how):
    """Cost, J^T F, the diagonal and J^T J v in double on the reordered graph against the ordered one: only the summation order differs."""
    P = gc.base_problem(energy, mesh, True)
    Q = gc.reorder(P, how, seed=1)
    o = oracle_solver(oracle_lib, P)
    v = np.random.default_rng(5).standard_normal(o.n)
    a, b = _stages(o, P, v), _stages(o, Q, v)
    o.close()
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    for x, y in zip(a[1:], b[1:]):
        assert rel_err(y, x) < 1e-12


GRADIENT_SHAPES = {
    "open_patch": lambda e: gc.base_problem(e, "open_patch", True),
    "isolated": lambda e: gc.with_isolated_vertex(gc.base_problem(e, "armadillo", True)),
    "duplicates": lambda e: gc.with_duplicate_edges(gc.base_problem(e, "armadillo", True), 9),
}


@pytest.mark.parametrize("shape", sorted(GRADIENT_SHAPES))
@pytest.mark.parametrize("energy", gc.ENERGIES)
def test_oracle_jtf_is_gradient_of_cost_on_the_new_shapes(oracle_lib, energy, shape):
    """As test_oracle.py::test_jtf_is_gradient_of_cost (central differences, h = 1e-6, 1e-6 norm-wise)."""
    P = GRADIENT_SHAPES[shape](energy)
    s = oracle_solver(oracle_lib, P)
    f, d = s.eval_jtf(P.params)
    g = _fd_gradient(s, P, 1e-6)
    s.close()
    assert rel_err(f, g) < 1e-6
    assert np.all(d >= 0)


def test_repeated_vertex_hyperedge_diagonal_is_the_sum_of_squares_per_slot(oracle_lib):
    """A hyperedge that names one vertex in two slots (v2 == v3 at an open mesh's valence-2 corner: its ring has two entries, so the neighbour before and after v1 is the same vertex): J^T F and J^T J v add the two slots' partials (the gradient test
    above covers that), but the preconditioner diagonal can be read two ways -- the square of the summed partial or the sum of the squares per slot.  The reference's
    generated code decides: createjtfgraph (API/src/o.t:2241-2250) keeps one scatter per unknown of the residual's support, keyed by (graph slot, channel), and adds
    partial * partial to each -- per slot; the graph kernel PCGInit1_Graph (solverGPUGaussNewton.t:687-692) runs exactly that function per hyperedge.  So the diagonal
    is the sum of squares per slot: the oracle's Inst lists carry one entry per slot (oracle/solver.hpp evalJTF adds dv * dv per entry), the HIP engine one record per
    (hyperedge, slot).  Here: the oracle's diagonal at the corners' neighbours equals the per-slot sum rebuilt from one-hot J^T J products, and differs from J^T J's own
    diagonal there by the cross term."""
    P = gc.base_problem("cotangent", "open_patch", True)
    v0, v1, v2, v3 = gc.index_arrays(P)
    rep = np.flatnonzero(v2 == v3)
    assert len(rep) == 4
    o = oracle_solver(oracle_lib, P)
    _, d = o.eval_jtf(P.params)
    # the same problem with the repeated slot split over two coincident vertices: every partial is unchanged, the two slots now scatter to different rows
    N = gc.n_vertices(P)
    Q = P
    for _ in sorted(set(v3[rep].tolist())):
        Q = gc._append_vertex(Q, [0, 0, 0])
    twins = {}
    cols = [c.copy() for c in gc.index_arrays(P)]
    for e in rep:
        t = twins.setdefault(int(v3[e]), N + len(twins))
        cols[3][e] = t
    assert len(twins) == gc.n_vertices(Q) - N == 4      # each corner's two hyperedges repeat the corner's other neighbour
    for v, t in twins.items():
        Q.params[2][t] = Q.params[2][v]; Q.params[3][t] = Q.params[3][v]
    Q = gc._with_indices(Q, cols)
    oq = oracle_solver(oracle_lib, Q)
    _, dq = oq.eval_jtf(Q.params)
    w_fit2 = float(P.params[0]) ** 2
    for v, t in twins.items():
        per_slot = dq[3 * v:3 * v + 3] + (dq[3 * t:3 * t + 3] - w_fit2)      # (the twin's own fit residual adds w_fit^2 to its rows)
        assert np.allclose(d[3 * v:3 * v + 3], per_slot, rtol=1e-13, atol=0)
        # ... and it is NOT J^T J's own diagonal there: that one squares the summed partial
        jj = np.array([o.apply_jtj(P.params, np.eye(1, o.n, 3 * v + c).reshape(-1))[3 * v + c] for c in range(3)])
        assert np.all(np.abs(jj - d[3 * v:3 * v + 3]) > 1e-9 * np.abs(jj))
    o.close(); oq.close()
