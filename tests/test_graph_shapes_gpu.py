"""GPU parity tests (-m gpu) of the four mesh kernel sets on the graphs the generated workloads never produce (tests/graph_cases.py): hyperedges in any order (shuffled,
descending, interleaved so that every run of one head has length 1), real irregular meshes (valence 3..12), a hub, a vertex without hyperedges, a vertex that is only ever
a tail, repeated half-edges, a hyperedge that names one vertex twice -- and one plan bound to several graphs in turn.

GraphOps (graph_engine.h: cotangent, embedded, robust) and ArapOps (energy_graph.hip) read the caller's index arrays through lists built once per graph (incidence lists;
out- / in-lists, the symmetry verdict, ELL planes, the one-workgroup variant) and rebuild them when the pointers, the edge count or a position-weighted checksum change.
Everything here runs beside the CPU oracle on the same arrays; the functor energies in gather mode (the default) and in scatter mode (OPT_AMD_GRAPH_GATHER=0, whose
segmentedAtomicAdd only ever saw grouped runs).  A re-bound plan is compared with a fresh plan bit for bit: gather mode and the ARAP paths use no atomics.
Bars: stages 1e-11 / 3e-5 norm-wise (double / float), initial cost 1e-12 / 1e-5, double trajectories 1e-10 on costs, 1e-9 on the unknowns, 1e-8 on the LM radius."""
import numpy as np
import pytest

import graph_cases as gc
from opt_amd import api
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

ORDERS = [("armadillo", "shuffle"), ("armadillo", "reverse"), ("armadillo", "interleave"), ("raptor", "shuffle")]
MODES = {"cotangent": ("gather", "scatter"), "embedded": ("gather", "scatter"), "robust": ("gather", "scatter"), "arap": ("gather",)}      # (ARAP: its own kernel set, no scatter switch)
PREC = {"f32": False, "f64": True}


def _mode(monkeypatch, mode):
    if mode == "scatter":
        monkeypatch.setenv("OPT_AMD_GRAPH_GATHER", "0")
    else:
        monkeypatch.delenv("OPT_AMD_GRAPH_GATHER", raising=False)


def _order_cases(precisions=("f32", "f64")):
    return [pytest.param(e, mesh, how, PREC[p], m, id=f"{e}-{mesh}-{how}-{p}-{m}")
            for e in gc.ENERGIES for mesh, how in ORDERS for p in precisions for m in MODES[e]]


_BASE = {}


def _base(energy, mesh, double):
    """The ordered problem (built once per session; every user clones or transforms it, none changes it)."""
    k = (energy, mesh, double)
    if k not in _BASE:
        _BASE[k] = gc.base_problem(energy, mesh, double)
    return _BASE[k]


def _hip_stages(P, v, timing=False):
    import torch
    g = hip_solver(P, timing=timing)
    dev = api.to_device(P)
    c = g.eval_cost(dev)
    f, d = g.eval_jtf(dev)
    Av, dot = g.apply_jtj(dev, torch.from_numpy(v).cuda())
    out = (c, f.cpu().numpy(), d.cpu().numpy(), Av.cpu().numpy(), dot)
    t = g.kernel_timings() if timing else None
    g.close()
    return out, t


def _as_double(P):
    """The float problem P for the double oracle: the same float values, widened."""
    X = P.clone(); X.double = True
    for s in gc.layout(P)["vertex"]:
        X.params[s] = X.params[s].astype(np.float64)
    return X


def _check_stages(oracle_lib, P, timing=False):
    """tests/test_energies_gpu.py::test_cost_jtf_diag_jtjp on P; returns the timer table."""
    tol = 1e-11 if P.double else 3e-5
    o = oracle_solver(oracle_lib, P)
    v = np.random.default_rng(5).standard_normal(o.n).astype(o.dtype)
    c_ref = o.eval_cost(P.params)
    f_ref, d_ref = o.eval_jtf(P.params)
    Av_ref = o.apply_jtj(P.params, v)
    o.close()
    (c, f, d, Av, dot), t = _hip_stages(P, v, timing)
    errs = dict(cost=abs(c - c_ref) / abs(c_ref), jtf=rel_err(f, f_ref), diag=rel_err(d, d_ref), jtjv=rel_err(Av, Av_ref))
    print("stages", P.energy, "double" if P.double else "float", {k: f"{e:.3g}" for k, e in errs.items()})
    if not P.double:      # printed, not asserted: how far float arithmetic itself is from the exact value on this input -- the double oracle on the same float arrays
        X = _as_double(P)
        ox = oracle_solver(oracle_lib, X)
        fx, dx = ox.eval_jtf(X.params)
        Ax = ox.apply_jtj(X.params, v.astype(np.float64))
        ox.close()
        print("   float oracle against the exact value:", {k: f"{e:.3g}" for k, e in dict(jtf=rel_err(f_ref, fx), diag=rel_err(d_ref, dx), jtjv=rel_err(Av_ref, Ax)).items()})
        print("   float kernel against the exact value:", {k: f"{e:.3g}" for k, e in dict(jtf=rel_err(f, fx), diag=rel_err(d, dx), jtjv=rel_err(Av, Ax)).items()})
    assert abs(c - c_ref) <= (1e-12 if P.double else 1e-5) * abs(c_ref) + 1e-30
    assert errs["jtf"] < tol and errs["diag"] < tol and errs["jtjv"] < tol, errs
    assert abs(dot - float(v.astype(np.float64) @ Av_ref.astype(np.float64))) <= 10 * tol * abs(dot) + 1e-30
    return t


def _check_trajectory(oracle_lib, P, kind, nsteps, liters, between_steps=None, timing=False, **params):
    """Step by step beside the oracle (double bars).  between_steps(step, host params, device params) may change the inputs in place after a step."""
    assert P.double
    kw = dict(nIterations=nsteps, lIterations=liters)
    o = oracle_solver(oracle_lib, P, kind, **kw)
    g = hip_solver(P, kind, timing=timing, **kw, **params)
    Pref = P.clone(); dev = api.to_device(P)
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    assert_close("cost0", g.cost(), o.cost(), 1e-12, floor=scale, double=True)
    step = 0
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        step += 1
        print("cost", step, g.cost(), o.cost(), abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-7 * scale))
        assert_close("cost", g.cost(), o.cost(), 1e-10, floor=1e-7 * scale, double=True, step=step)      # (relative to the initial cost where the energy has converged: test_energies_gpu.py::test_trajectory)
        if kind == "LMGPU":
            assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), 1e-8, double=True, step=step)
        if not a:
            break
        if between_steps:
            between_steps(step, Pref.params, dev)
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    t = g.kernel_timings() if timing else None
    g.close(); o.close()
    return t


# ---- any hyperedge order ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy,mesh,how,double,mode", _order_cases())
def test_stages_on_reordered_graphs(oracle_lib, monkeypatch, energy, mesh, how, double, mode):
    """Every stage beside the oracle, bars 1e-11 (double) / 3e-5 (float) norm-wise.  cotangent-raptor-shuffle-f32 is the case that needs the cotangent functor to round like
    the oracle (no fused multiply-adds, the cost pass dividing as the dual numbers do): the raptor's sliver triangles (smallest discriminant 1.6e-4) turn one ulp of
    1 - cos^2 into 4e-4 of the stage.  _check_stages also prints how far float arithmetic itself is from the exact value there (about 1e-3)."""
    _mode(monkeypatch, mode)
    _check_stages(oracle_lib, gc.reorder(_base(energy, mesh, double), how, seed=1))


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("energy,mesh,how,double,mode", _order_cases(("f64",)))
def test_trajectory_on_reordered_graphs(oracle_lib, monkeypatch, energy, mesh, how, double, mode, kind):
    _mode(monkeypatch, mode)
    _check_trajectory(oracle_lib, gc.reorder(_base(energy, mesh, double), how, seed=1), kind, 3, 12)


@pytest.mark.parametrize("energy,mesh,how", [pytest.param(e, m, h, id=f"{e}-{m}-{h}") for e in gc.ENERGIES for m, h in ORDERS])
def test_kernel_stages_do_not_depend_on_the_hyperedge_order(energy, mesh, how):
    """In double the HIP stages on the reordered and on the ordered graph differ by the summation order alone (gather mode: lists sorted by hyperedge id)."""
    P = _base(energy, mesh, True)
    v = np.random.default_rng(5).standard_normal(sum(int(np.asarray(P.params[s]).size) for s in P.unknown_slots))
    a, _ = _hip_stages(P, v)
    b, _ = _hip_stages(gc.reorder(P, how, seed=1), v)
    assert abs(a[0] - b[0]) <= 1e-11 * abs(a[0])
    for x, y, name in zip(a[1:4], b[1:4], ("jtf", "diag", "jtjv")):
        assert rel_err(y, x) < 1e-11, name


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------------------------
def _shape(name, energy, double=True):
    if name == "hub300":          # a grouped run of 300 hyperedges of one head: across lanes 63 / 64 and a 256-thread workgroup
        return gc.with_hub(_base(energy, "armadillo_sub", double), 300)
    if name == "hub70":           # more out-neighbours than csr_symmetric compares (64) and than the ELL width (16)
        return gc.with_hub(_base(energy, "armadillo", double), 70)
    if name == "isolated":
        return gc.with_isolated_vertex(_base(energy, "armadillo", double))
    if name == "tail_only":
        return gc.with_tail_only_vertex(_base(energy, "armadillo", double))
    if name == "duplicates":
        return gc.with_duplicate_edges(_base(energy, "armadillo", double), 9)
    assert name == "open_patch"   # four hyperedges with v2 == v3
    return _base(energy, "open_patch", double)


SHAPES = ([("hub300", e) for e in gc.FUNCTOR_ENERGIES] + [("hub70", "arap")] + [(s, e) for s in ("isolated", "tail_only", "duplicates") for e in gc.ENERGIES] +
          [("open_patch", "cotangent")])
# which J^T J p kernels the ARAP plan must have run: the plane gather of a symmetric graph within the ELL width (packVertexRecords) or the edge-list gather (packDerivativeRows)
ARAP_PLANES = {"hub70": False, "isolated": True, "tail_only": False, "duplicates": True}


@pytest.mark.parametrize("shape,energy,mode", [pytest.param(s, e, m, id=f"{s}-{e}-{m}") for s, e in SHAPES for m in MODES[e]])
def test_graph_shapes(oracle_lib, monkeypatch, shape, energy, mode):
    """Stages, then a 2 x 12 Gauss-Newton trajectory, in double."""
    _mode(monkeypatch, mode)
    P = _shape(shape, energy)
    t = _check_stages(oracle_lib, P, timing=True)
    if energy == "arap":
        assert ("packVertexRecords" in t) == ARAP_PLANES[shape] and ("packDerivativeRows" in t) == (not ARAP_PLANES[shape]), t.keys()
    _check_trajectory(oracle_lib, P, "gaussNewtonGPU", 2, 12)


@pytest.mark.parametrize("shape,energy", [("hub300", "cotangent"), ("isolated", "embedded"), ("tail_only", "robust"), ("duplicates", "arap"), ("open_patch", "cotangent")])
def test_graph_shapes_stages_in_float(oracle_lib, shape, energy):
    """One float case per shape, the project's float stage bar (3e-5 norm-wise)."""
    _check_stages(oracle_lib, _shape(shape, energy, double=False))


# ---- one plan, several graphs ---------------------------------------------------------------------------------------------------------------------------------------
KW = dict(nIterations=2, lIterations=8)


def _solve(g, P, dev=None):
    """(costs after init and after every step, final unknowns) of a solve of P on plan g."""
    dev = api.to_device(P) if dev is None else dev
    g.init(dev)
    costs = [g.cost()]
    while True:
        more = g.step(dev)
        costs.append(g.cost())
        if not more:
            break
    return costs, device_unknowns(P, dev), dev


def _fresh(P, **params):
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **KW, **params)
    out = _solve(g, P)
    g.close()
    return out[:2]


def _same_bits(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1], b[1])


def _permute_in_place(P, perm, host=None, dev=None):
    """The index arrays of the problem permuted in place, in the host arrays and / or the device tensors: pointers and count stay."""
    import torch
    for s in gc.layout(P)["idx"]:
        if host is not None:
            host[s][:] = host[s][perm]
        if dev is not None:
            dev[s].copy_(dev[s][torch.from_numpy(perm).cuda()])


def _rebind_cases():
    return [pytest.param(e, PREC[p], id=f"{e}-{p}") for e in gc.ENERGIES for p in ("f32", "f64")]


@pytest.mark.parametrize("energy,double", _rebind_cases())
def test_rebind_same_graph_in_new_buffers(energy, double):
    P = _base(energy, "armadillo", double)
    want = _fresh(P)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **KW)
    first = _solve(g, P)                 # (its device buffers stay alive: the second upload cannot land on the same addresses)
    second = _solve(g, P)
    assert all(first[2][s].data_ptr() != second[2][s].data_ptr() for s in gc.layout(P)["idx"])
    g.close()
    _same_bits(first, want); _same_bits(second, want)


@pytest.mark.parametrize("energy,double", _rebind_cases())
def test_rebind_same_buffers_permuted_in_place(energy, double):
    """Pointers and count unchanged: only the checksum can notice."""
    import torch
    P = _base(energy, "armadillo", double)
    Q = gc.reorder(P, "shuffle", seed=1)
    perm = gc.edge_permutation(gc.index_arrays(P)[0], "shuffle", seed=1)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **KW)
    first = _solve(g, P)
    dev = first[2]
    _permute_in_place(P, perm, dev=dev)
    for s in gc.layout(P)["idx"]:
        assert np.array_equal(dev[s].cpu().numpy(), Q.params[s])
    for s in P.unknown_slots:            # the unknowns back to their start, in place
        dev[s].copy_(torch.from_numpy(np.ascontiguousarray(P.params[s])).cuda())
    second = _solve(g, Q, dev)
    g.close()
    _same_bits(first, _fresh(P)); _same_bits(second, _fresh(Q))


@pytest.mark.parametrize("energy,double", _rebind_cases())
def test_rebind_larger_then_smaller_edge_count(energy, double):
    """A plan is made for one vertex count, so the larger graph is the armadillo plus a hub (768 -> 894 half-edges, cotangent: its margin-checked hyperedges) and back:
    the record, incidence, derivative-row and edge-record buffers grow and are then used below their capacity."""
    P = _base(energy, "armadillo", double)
    H = gc.with_hub(P, 70)
    assert H.meta["n_edges"] > P.meta["n_edges"]
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **KW)
    runs = [_solve(g, X) for X in (P, H, P)]
    g.close()
    small, large = _fresh(P), _fresh(H)
    _same_bits(runs[0], small); _same_bits(runs[1], large); _same_bits(runs[2], small)


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("energy", gc.ENERGIES)
def test_index_arrays_permuted_in_place_between_two_steps(oracle_lib, energy, kind):
    """Opt_ProblemStep binds at every call (the oracle reads its arrays at every call): hyperedges permuted in place, on both sides, between steps 1 and 2 of one solve."""
    P = _base(energy, "armadillo", True)
    perm = gc.edge_permutation(gc.index_arrays(P)[0], "shuffle", seed=2)

    def between(step, host, dev):
        if step == 1:
            _permute_in_place(P, perm, host=host, dev=dev)

    _check_trajectory(oracle_lib, P, kind, 3, 12, between_steps=between)


@pytest.mark.parametrize("energy", gc.ENERGIES)
def test_binding_the_same_graph_again_does_not_rebuild(energy):
    """The timer table counts buildIncidenceLists / buildEdgeLists once over two binds of the identical graph, and again once the arrays are permuted in place."""
    P = _base(energy, "armadillo", True)
    name = "buildEdgeLists" if energy == "arap" else "buildIncidenceLists"
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **KW)
    dev = api.to_device(P)
    g.init(dev)                          # (Opt_ProblemInit restarts the table, then binds)
    assert g.kernel_timings()[name][0] == 1
    g.eval_cost(dev)                     # binds again: same pointers, count and checksum
    g.step(dev)
    assert g.kernel_timings()[name][0] == 1
    _permute_in_place(P, gc.edge_permutation(gc.index_arrays(P)[0], "shuffle", seed=1), dev=dev)
    g.eval_cost(dev)
    assert g.kernel_timings()[name][0] == 2
    g.close()


def test_arap_one_workgroup_plan_follows_the_graph_it_is_bound_to():
    """amd_onchip = 5, one plan: on chip -> a 17th neighbour through a larger edge count (streams: the ELL width) -> the first graph again (on chip, the bits of a fresh
    plan) -> one reverse edge removed (streams: asymmetric graph)."""
    P = _base("arap", "armadillo", True)
    H = gc.with_hub(P, 17)
    R = gc.without_one_reverse_edge(P)
    assert gc.max_out_degree(P) <= 16 and gc.max_out_degree(H) == 17 and H.meta["n_edges"] > P.meta["n_edges"]
    g = hip_solver(P, "gaussNewtonGPU", timing=True, amd_onchip=5, **KW)
    want = {"P": _fresh(P, amd_onchip=5), "H": _fresh(H, amd_onchip=5), "R": _fresh(R, amd_onchip=5)}
    for X, key, why in ((P, "P", None), (H, "H", "more than 16 neighbours"), (P, "P", None), (R, "R", "asymmetric graph")):
        run = _solve(g, X)
        d, t = g.describe(), g.kernel_timings()
        if why is None:
            assert d["path"] == "on-chip" and "PCGSolveOnChip" in t and "PCGStep1" not in t and g.on_chip_status() == 1, (d, t.keys())
        else:
            assert d["path"] == "launch-per-iteration" and why in d["why_not_on_chip"], d
            assert "PCGSolveOnChip" not in t and "PCGStep1" in t and g.on_chip_status() == 0, t.keys()
        _same_bits(run, want[key])
    g.close()
