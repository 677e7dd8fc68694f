"""GPU tests (-m gpu) of the one-workgroup linear solve of the functor mesh energies (solver parameter amd_onchip = 6; opt_amd/csrc/graph_onchip.h:
ge_onchipPcg<T, G, V, LMV>) -- cotangent_mesh_smoothing, embedded_mesh_deformation, robust_nonrigid_alignment, Gauss-Newton and Levenberg-Marquardt, float and double.

By default these energies run four launches per PCG iteration, two with amd_graph_fused = 1.  With amd_onchip = 6 a mesh whose vertices fit a variant (V vertices per
lane of one workgroup of up to 512 threads) runs its whole linear solve as one launch of one workgroup.  Here:
  * the path is taken and visible for every offered variant (GRAPH_VARIANTS), and below level 6 nothing changes, bits included; ARAP at 6 is ARAP at 5;
  * the same iterates as the four-launch loop (trace rows and unknowns at 1e-9, the bar of test_graph_fused_gpu.py's recipe);
  * beside the CPU oracle, with the bars, builders and stepping routines of the existing tests, imported: stages, trajectories (test_energies_gpu.CASES, armadillo,
    armadillo_sub), the reference's head.ply (689 vertices, two vertices per lane), the variant boundaries of embedded and robust, graph shapes (hub, isolated and
    tail-only vertices, duplicate hyperedges, v2 == v3, shuffled order), LM inner and outer controls;
  * refusals (scatter mode, OPT_AMD_ONCHIP=0, too many vertices) keep today's loops and say why; re-binding, determinism, Opt_ProblemSolve.
Bars: double 1e-10 on costs / 1e-9 on the unknowns / 1e-8 on the LM radius; float 1e-5 on costs (2e-5 on the unknowns, or twice the frozen envelope of legal float
runs where test_energies_gpu.ENVELOPES has the case) / 1e-3 on the radius.
The kernel has no wait that could time out, so there is no time-out test.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import graph_cases as gc
import lm_control_cases as lc
import test_energies_gpu as te
import test_graph_fused_gpu as gf
import test_graph_shapes_gpu as gs
import test_lm_controls_gpu as lmc
import test_lm_outer_controls_gpu as lmo
from opt_amd import api, workloads as wl
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

ONCHIP = dict(amd_onchip=6)
ENERGIES = gc.FUNCTOR_ENERGIES
FUNCTOR = {"cotangent": "CotangentG", "embedded": "EmbeddedG", "robust": "RobustG"}
KINDS = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}
LANES = 512
# (precision, functor, vertices per lane, Levenberg-Marquardt) of every kernel ge_onchipPcg<T, G, V, LMV> the library offers; tests/test_onchip_graph_resources.py holds
# the list against the build.  A variant serves up to V * 512 vertices.  Not offered: V = 2 for embedded and robust -- measured, it lost to the two-launch loop at 529
# and at 1024 vertices (profiles/onchip_graph.md); cotangent keeps V = 2, which is what serves head.ply.
GRAPH_VARIANTS = ([(p, f, 1, lm) for p in ("float", "double") for f in FUNCTOR.values() for lm in (False, True)] +
                  [(p, "CotangentG", 2, lm) for p in ("float", "double") for lm in (False, True)])
OLD_NAMES = ("PCGStep1_Graph", "PCGStep1", "PCGStep2", "PCGStep3")
HEAD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "head_mesh.npz")


def _prec(double):
    return "double" if double else "float"


def _largest(energy, double, lm):
    return LANES * max(v for p, f, v, l in GRAPH_VARIANTS if p == _prec(double) and f == FUNCTOR[energy] and l == lm)


def _variant(energy, double, lm, n):
    return min(v for p, f, v, l in GRAPH_VARIANTS if p == _prec(double) and f == FUNCTOR[energy] and l == lm and n <= v * LANES)


def _energy(P):
    return {v: k for k, v in gc.STEM.items()}[P.energy]


def _check_path(g, P, lm, expect_onchip=True, why=None):
    t, d = g.kernel_timings(), g.describe()
    assert ("PCGSolveOnChip" in t) == expect_onchip, t.keys()
    assert g.on_chip_status() == (1 if expect_onchip else 0)
    if expect_onchip:
        n = int(P.dims[0])
        assert not any(k in t for k in OLD_NAMES) and "PCGStep2+PCGStep3" not in t, t.keys()
        assert d["path"] == "on-chip" and d["workgroups"] == "1" and d["vertices"] == str(n) and d["hyperedges"] == str(P.meta["n_edges"]), d
        e = _energy(P)
        assert d["variant"] == "ge_onchipPcg<%s, %s, %d, %s>" % (_prec(P.double), FUNCTOR[e], _variant(e, P.double, lm, n), "LM" if lm else "GN"), d
    else:
        assert d["path"] == "launch-per-iteration" and (why is None or why in d["why_not_on_chip"]), d
        assert "PCGStep1" in t, t.keys()


def _run(P, kind, nsteps, liters, timing=True, trace=False, **params):
    """(costs after init and every step, final unknowns, timer table, describe(), trace, on-chip status) of Init + Step by Step."""
    g = hip_solver(P, kind, timing=timing, nIterations=nsteps, lIterations=liters, **params)
    if trace:
        g.enable_trace()
    dev = api.to_device(P)
    g.init(dev)
    costs = [g.cost()]
    while True:
        more = g.step(dev)
        costs.append(g.cost())
        if not more:
            break
    out = (costs, device_unknowns(P, dev), g.kernel_timings() if timing else None, g.describe(), g.trace() if trace else None, g.on_chip_status())
    g.close()
    return out


def _beside(oracle_lib, P, kind, nsteps, liters, ctol, xtol, rtol=None, expect_onchip=True, why=None, hip=ONCHIP, **controls):
    """Step by step beside the oracle: the same return values (accept / reject, end of the solve), costs at ctol, the LM radius at rtol, the final unknowns at xtol;
    then the path.  Returns [(oracle cost, library cost, oracle radius)]."""
    lm = kind == "LMGPU"
    kw = dict(nIterations=nsteps, lIterations=liters, **controls)
    o = oracle_solver(oracle_lib, P, kind, **kw)
    g = hip_solver(P, kind, timing=True, **kw, **hip)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    assert_close("cost0", g.cost(), o.cost(), 1e-12 if P.double else 1e-5, floor=scale, double=P.double)
    hist = [(o.cost(), g.cost(), o.trust_region_radius() if lm else 0.0)]
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        hist.append((o.cost(), g.cost(), o.trust_region_radius() if lm else 0.0))
        print("step", len(hist) - 1, a, b, "cost", g.cost(), o.cost(), abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-7 * scale),
              "radius", g.trust_region_radius() if lm else "", o.trust_region_radius() if lm else "")
        assert a == b, (a, b, hist)
        assert_close("cost", g.cost(), o.cost(), ctol, floor=1e-7 * scale, double=P.double, step=len(hist) - 1)
        if lm:
            assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), rtol, double=P.double, step=len(hist) - 1)
        if not a:
            break
    _check_path(g, P, lm, expect_onchip, why)
    x = rel_err(device_unknowns(P, dev), flat_unknowns(Pref))
    print("x", x, xtol)
    if xtol is not None:
        assert_close("x", x, 0.0, xtol, absolute=True, double=P.double)
    g.close(); o.close()
    return hist


def _bars(double):
    return dict(ctol=1e-10, xtol=1e-9, rtol=1e-8) if double else dict(ctol=1e-5, xtol=None, rtol=1e-3)


_MESH = {}


def _head(double):
    """cotangent_mesh_smoothing on the reference example's own mesh head.ply (tests/golden/meshes/make_head_mesh.py): 689 vertices, 4086 hyperedges, the input
    wl.cotangent_from_mesh makes of it by default (seed 0, noise 0.05).  The horizons asserted below are the ones at which legal summation orders of the CPU oracle
    (set_reduction(1, seed), seeds 1-3, against its exact-order run) agree far below the bars ON THIS INPUT: GN 2 x 6 1e-15 (double) / 2.8e-7 (float), LM 5 x 25
    2.6e-14.  Without the noise the same LM run already spreads 1.7e-10 among legal orders, above the double bar, and is not used."""
    if double not in _MESH:
        z = np.load(HEAD)
        _MESH[double] = wl.cotangent_from_mesh(z["vertices"].astype(np.float64), z["faces"].tolist(), double=double, seed=0)
    return _MESH[double]


def _grid(energy, nx, ny, double):
    make = {"embedded": wl.embedded_mesh_deformation, "robust": wl.robust_nonrigid_alignment}[energy]
    return make(nx, ny, double=double, seed=3, perturb=0.01)


def _problem_for(prec, functor, v):
    """The smallest shared input that reaches the variant: the armadillo (130 vertices) at V = 1; head.ply (cotangent, 689 vertices) at V = 2."""
    energy, double = {f: e for e, f in FUNCTOR.items()}[functor], prec == "double"
    if v == 1:
        return gs._base(energy, "armadillo", double)
    assert energy == "cotangent"
    return _head(double)


# ---- the path is taken and visible (fails without the feature) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,functor,v,lm", GRAPH_VARIANTS, ids=lambda x: str(x))
def test_the_on_chip_path_is_taken_and_visible(prec, functor, v, lm):
    P = _problem_for(prec, functor, v)
    costs, x, t, d, _, status = _run(P, KINDS["LM" if lm else "GN"], 2, 6, **ONCHIP)
    assert d["path"] == "on-chip" and d["workgroups"] == "1" and d["vertices"] == str(P.dims[0]) and d["hyperedges"] == str(P.meta["n_edges"]), d
    assert d["variant"] == f"ge_onchipPcg<{prec}, {functor}, {v}, {'LM' if lm else 'GN'}>", d
    assert t["PCGSolveOnChip"][0] == 2, t
    assert not any(k in t for k in ("PCGStep1_Graph", "PCGStep2", "PCGStep3", "PCGStep1", "PCGStep2+PCGStep3")), t.keys()
    assert status == 1
    assert np.isfinite(costs).all() and np.isfinite(x).all()


def test_every_variant_is_reached():
    reached = set()
    for prec, functor, v, lm in GRAPH_VARIANTS:
        P = _problem_for(prec, functor, v)
        energy = _energy(P)
        assert P.double == (prec == "double") and FUNCTOR[energy] == functor
        reached.add((prec, functor, _variant(energy, P.double, lm, int(P.dims[0])), lm))
    assert reached == set(GRAPH_VARIANTS) and len(set(GRAPH_VARIANTS)) == len(GRAPH_VARIANTS)
    for energy in ENERGIES:      # the required variants: float, V = 1 everywhere; cotangent at V = 2, which serves head.ply
        for lm in (False, True):
            assert ("float", FUNCTOR[energy], 1, lm) in GRAPH_VARIANTS
            assert ("float", "CotangentG", 2, lm) in GRAPH_VARIANTS
    assert _head(False).dims[0] == 689 and _head(False).meta["n_edges"] == 4086


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_the_record_placement_does_not_change_a_bit(monkeypatch, energy, kind):
    """The records of an iteration live in LDS where they fit beside the vectors (the armadillo's do), else in the plan's buffer (head.ply: 196 KB); the placement only
    moves them (OPT_AMD_ONCHIP_REC_LDS=0: always the buffer)."""
    P = gs._base(energy, "armadillo", False)
    a = _run(P, KINDS[kind], 2, 6, residual_reset_period=3, **ONCHIP)
    monkeypatch.setenv("OPT_AMD_ONCHIP_REC_LDS", "0")
    b = _run(P, KINDS[kind], 2, 6, residual_reset_period=3, **ONCHIP)
    assert a[3]["records"] == "LDS" and b[3]["records"] == "memory" and a[5] == b[5] == 1, (a[3], b[3])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    if energy == "cotangent":
        assert _run(_head(False), KINDS[kind], 1, 2, **ONCHIP)[3]["records"] == "memory"


# ---- nothing changes below 6 --------------------------------------------------------------------------------------------------------------------------------------------
def _without_level(d):
    return {k: v for k, v in d.items() if k != "amd_onchip"}      # (the solver's own echo of the parameter, there before this path)


@pytest.mark.parametrize("params", [dict(), dict(amd_onchip=1), dict(amd_onchip=5), dict(amd_onchip=6, amd_reference_order=1)], ids=["unset", "1", "5", "6-reference_order"])
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_nothing_changes_below_6(energy, kind, params):
    """The four launches, today's describe(), and the bits of a plan that was never given the parameter."""
    P = gs._base(energy, "armadillo", False)
    never = {k: v for k, v in params.items() if k != "amd_onchip"}
    a = _run(P, KINDS[kind], 2, 6, **params)
    b = _run(P, KINDS[kind], 2, 6, **never)
    assert all(k in a[2] for k in OLD_NAMES) and "PCGSolveOnChip" not in a[2] and a[5] == 0, a[2].keys()
    assert _without_level(a[3]) == _without_level(b[3]) and "why_not_on_chip" not in a[3] and a[3]["path"] != "on-chip", (a[3], b[3])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert {k: c for k, (c, _) in a[2].items()} == {k: c for k, (c, _) in b[2].items()}


@pytest.mark.parametrize("kind,double", [("GN", False), ("LM", True)])
def test_arap_at_6_is_arap_at_5(kind, double):
    P = gs._base("arap", "armadillo", double)
    a = _run(P, KINDS[kind], 2, 6, amd_onchip=6)
    b = _run(P, KINDS[kind], 2, 6, amd_onchip=5)
    assert a[5] == b[5] == 1 and a[2]["PCGSolveOnChip"][0] == b[2]["PCGSolveOnChip"][0] == 2
    assert _without_level(a[3]) == _without_level(b[3]) and "arap_onchipPcg" in a[3]["variant"], (a[3], b[3])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ---- the same iterates as the four-launch loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy", ENERGIES)
def test_same_iterates_as_the_four_launch_loop(energy):
    """The recipe and bar (1e-9) of test_graph_fused_gpu.py::test_same_iterates_as_the_four_launch_loop: double, Gauss-Newton, 1 x 10 on the armadillo, traced."""
    P = gs._base(energy, "armadillo", True)
    res = {lvl: _run(P, "gaussNewtonGPU", 1, 10, trace=True, amd_onchip=lvl) for lvl in (6, 1)}
    assert "PCGSolveOnChip" in res[6][2] and "PCGSolveOnChip" not in res[1][2] and "PCGStep1_Graph" in res[1][2]
    assert rel_err(res[6][1], res[1][1]) <= 1e-9
    a, b = res[6][4], res[1][4]
    assert a.shape == b.shape == (10, 6), (a.shape, b.shape)
    assert np.array_equal(a[:, :2], b[:, :2])      # (outer step, PCG iteration)
    err = np.abs(a[:, 2:5] - b[:, 2:5]) / np.maximum(np.abs(b[:, 2:5]), 1e-300)
    print("largest relative difference of a trace entry:", err.max())
    assert err.max() <= 1e-9, (err.max(), np.unravel_index(err.argmax(), err.shape))


# ---- stages and trajectories beside the oracle ------------------------------------------------------------------------------------------------------------------------------
def _onchip_solver(P, *a, **k):
    return hip_solver(P, *a, **k, **ONCHIP)


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", ["armadillo", "armadillo_sub"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_stages_beside_the_oracle(oracle_lib, monkeypatch, energy, mesh, double):
    """test_graph_shapes_gpu.py's stage check (1e-11 / 3e-5 norm-wise) with every plan it makes at level 6: the probes keep the record kernels."""
    monkeypatch.setattr(gs, "hip_solver", _onchip_solver)
    t = gs._check_stages(oracle_lib, gs._base(energy, mesh, double), timing=True)
    assert "PCGStep1_Graph" in t and t["PCGStep1"][0] == 1, t.keys()


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["cotangent", "embedded", "embedded_rest", "robust"])
def test_trajectory(oracle_lib, name, double, kind):
    """test_energies_gpu.py::test_trajectory's recipe on its CASES, 4 x 12, with its bars (see test_graph_fused_gpu.py::test_trajectory)."""
    P = te.CASES[name](double)
    ctol, xtol = (1e-10, 1e-9) if double else (1e-5, 2e-5)
    if not double:
        env = te.ENVELOPES.get(f"{name}_{kind}")
        if env is not None:
            ctol, xtol = max(ctol, 2.0 * env[0]), max(xtol, 2.0 * env[1])
    _beside(oracle_lib, P, kind, 4, 12, ctol, xtol, 1e-8 if double else 1e-3)


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("mesh", ["armadillo", "armadillo_sub"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_trajectory_on_the_armadillo(oracle_lib, energy, mesh, kind):
    t = gs._check_trajectory(oracle_lib, gs._base(energy, mesh, True), kind, 3, 12, timing=True, **ONCHIP)
    assert "PCGSolveOnChip" in t and not any(k in t for k in OLD_NAMES), t.keys()


# ---- the reference's head.ply: 689 vertices, two vertices per lane -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
def test_head_gn(oracle_lib, double):
    """Gauss-Newton 2 x 6.  (Legal summation orders of the CPU oracle spread 1e-15 in double and 2.8e-7 in float at this horizon; the example's own 5 x 25 is NOT held
    against the oracle: its legal runs are 4e-5 apart in double and 3.7e-4 in float.)"""
    _beside(oracle_lib, _head(double), "gaussNewtonGPU", 2, 6, **_bars(double))


def test_head_lm_double(oracle_lib):
    """Levenberg-Marquardt 5 x 25 (legal orders spread 2.6e-14)."""
    _beside(oracle_lib, _head(True), "LMGPU", 5, 25, **_bars(True))


# ---- variant boundaries: embedded and robust -----------------------------------------------------------------------------------------------------------------------------------
# one partial wave; the largest size of these energies' variants (V = 1: 512 vertices) and one vertex more; 529, 1024 and 1025: the sizes a V = 2 variant would
# have served -- it is not offered for these energies (it lost in the measurement), so they stream, in float and in double.
GRIDS = [(8, 8), (32, 16), (27, 19), (23, 23), (32, 32), (41, 25)]


@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("energy", ["embedded", "robust"])
def test_variant_boundaries(oracle_lib, energy, nx, ny, kind, double):
    lm = kind == "LM"
    largest = _largest(energy, double, lm)
    _beside(oracle_lib, _grid(energy, nx, ny, double), KINDS[kind], 2, 8, expect_onchip=nx * ny <= largest,
            why="too many vertices (the variants serve up to %d)" % largest, **_bars(double), **(dict(residual_reset_period=3) if lm else {}))


def test_the_grids_sit_on_every_boundary():
    sizes = {nx * ny for nx, ny in GRIDS}
    for energy in ("embedded", "robust"):
        for double in (False, True):
            for lm in (False, True):
                assert _largest(energy, double, lm) in sizes and _largest(energy, double, lm) + 1 in sizes


@pytest.mark.parametrize("energy", ["embedded", "robust"])
def test_the_raptor_streams(oracle_lib, energy):
    P = gs._base(energy, "raptor", False)
    assert P.dims[0] == 2000
    _beside(oracle_lib, P, "gaussNewtonGPU", 1, 5, 1e-5, None, expect_onchip=False, why="too many vertices (the variants serve up to %d)" % _largest(energy, False, False))


# ---- graph shapes ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _shape(name, energy, double):
    if name == "open_patch":      # (cotangent: four hyperedges with v2 == v3)
        return gs._base(energy, "open_patch", double)
    B = gs._base(energy, "armadillo", double)
    return {"hub": lambda: gc.with_hub(B, 70), "isolated": lambda: gc.with_isolated_vertex(B), "tail_only": lambda: gc.with_tail_only_vertex(B),
            "duplicates": lambda: gc.with_duplicate_edges(B, 9), "shuffle": lambda: gc.reorder(B, "shuffle", seed=1)}[name]()


SHAPES = ("hub", "isolated", "tail_only", "duplicates", "open_patch", "shuffle")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("energy", ENERGIES)
def test_graph_shapes_double(oracle_lib, monkeypatch, energy, shape):
    """Stages, then a 2 x 8 Gauss-Newton trajectory on chip."""
    monkeypatch.setattr(gs, "hip_solver", _onchip_solver)
    P = _shape(shape, energy, True)
    gs._check_stages(oracle_lib, P)
    monkeypatch.undo()
    t = gs._check_trajectory(oracle_lib, P, "gaussNewtonGPU", 2, 8, timing=True, **ONCHIP)
    assert t["PCGSolveOnChip"][0] == 2 and not any(k in t for k in OLD_NAMES), t.keys()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("energy", ENERGIES)
def test_graph_shapes_float_stages(oracle_lib, monkeypatch, energy, shape):
    monkeypatch.setattr(gs, "hip_solver", _onchip_solver)
    gs._check_stages(oracle_lib, _shape(shape, energy, False))


# ---- LM inner controls ---------------------------------------------------------------------------------------------------------------------------------------------------------------
LM_GRID = gf._arap_grid()      # (period, qtol, liters) of test_lm_controls_gpu.py::test_arap_two_kernel_lm_iteration_controls


def _controls(period, qtol):
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    return kw


@pytest.mark.parametrize("period,qtol,liters", LM_GRID)
@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_inner_controls_double(oracle_lib, energy, period, qtol, liters):
    """Step for step beside the oracle: the same accept / reject decisions, costs at 1e-10, unknowns at 1e-9, radius at 1e-8 -- resets inside the solve, early-outs on,
    next to and between resets, all decided inside the kernel."""
    P = te.CASES[energy](True)
    _beside(oracle_lib, P, "LMGPU", 4, liters, 1e-10, 1e-9, 1e-8, **_controls(period, qtol))


@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_inner_controls_float(oracle_lib, energy):
    """One float row per energy: 1e-5 on the first step's cost, the project's float bar 1e-3 on the radius (test_lm_controls_gpu.py's routine)."""
    P = te.CASES[energy](False)
    lmc._side_by_side(oracle_lib, P, 1, 12, 1e-5, None, 1e-3, hip_only=ONCHIP, residual_reset_period=5)
    assert _run(P, "LMGPU", 1, 12, residual_reset_period=5, **ONCHIP)[5] == 1


def test_verbose_run_prints_the_early_out_and_keeps_the_bits(capfd):
    P = te.CASES["embedded"](True)
    silent = _run(P, "LMGPU", 3, 10, q_tolerance=0.5, **ONCHIP)
    assert silent[5] == 1
    capfd.readouterr()
    g = hip_solver(P, "LMGPU", verbosity=1, nIterations=3, lIterations=10, q_tolerance=0.5, **ONCHIP)
    dev = api.to_device(P)
    g.init(dev)
    costs = [g.cost()]
    while True:
        more = g.step(dev)
        costs.append(g.cost())
        if not more:
            break
    assert g.on_chip_status() == 1
    x = device_unknowns(P, dev)
    g.close()
    ctypes.CDLL(None).fflush(None)      # the library prints through C stdio
    out = capfd.readouterr().out
    assert costs == silent[0] and np.array_equal(x, silent[1]), (costs, silent[0])
    assert "breaking at iteration" in out, out[-2000:]


def test_a_rejected_step_restores_the_unknowns(oracle_lib):
    """LM rejects every step on the cotangent torus of test_energies_gpu.CASES (the CPU oracle does; the assertion below keeps the test from passing empty): the radius
    shrinks, the cost stays, and the unknowns are the ones the solve started from, bit for bit."""
    P = te.CASES["cotangent"](True)
    hist = _beside(oracle_lib, P, "LMGPU", 3, 12, 1e-10, 1e-9, 1e-8)
    rejected = [i for i in range(1, len(hist)) if hist[i][0] == hist[i - 1][0] and hist[i][2] < hist[i - 1][2]]
    assert len(rejected) >= 1, hist
    if len(rejected) == len(hist) - 1:
        costs, x, _, _, _, status = _run(P, "LMGPU", 3, 12, **ONCHIP)
        assert status == 1 and np.array_equal(x, flat_unknowns(P)) and all(c == costs[0] for c in costs)


# ---- LM outer controls -----------------------------------------------------------------------------------------------------------------------------------------------------------------
ONCHIP_PATHS = {"cotangent": dataclasses.replace(lc.PATHS["cotangent"], hip=dict(ONCHIP), onchip=True, kernels=("PCGFinalizeDiagonal", "PCGSolveOnChip"),
                                                 absent=OLD_NAMES + ("PCGStep2+PCGStep3",))}


def _outer(oracle_lib, base, name, double):
    """The oracle side of the on-chip path is its base path's (the same problem and controls): lm_control_cases.oracle_run."""
    p = ONCHIP_PATHS[base]
    sc = lc.scenario(oracle_lib, base, name)
    P = lc.problem(base, double)
    g = hip_solver(P, "LMGPU", timing=True, **lc.all_controls(base, sc), **p.hip)
    lmo._run(base, sc, P, g, lc.oracle_run(oracle_lib, base, name, double=double))
    t = g.kernel_timings()
    assert all(k in t for k in p.kernels) and not any(k in t for k in p.absent), t.keys()
    assert g.describe()["path"] == "on-chip"
    g.close()


@pytest.mark.parametrize("base,name", lc.cases(list(ONCHIP_PATHS)))
def test_lm_outer_controls_double(oracle_lib, base, name):
    _outer(oracle_lib, base, name, True)


@pytest.mark.parametrize("base,name", [(p, s) for p, s in lc.cases(list(ONCHIP_PATHS)) if lc.PATHS[p].float_too])
def test_lm_outer_controls_float(oracle_lib, base, name):
    _outer(oracle_lib, base, name, False)


# ---- refusals: today's loop, and why ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_scatter_mode_keeps_the_four_launches(monkeypatch, energy, kind):
    monkeypatch.setenv("OPT_AMD_GRAPH_GATHER", "0")
    P = gs._base(energy, "armadillo", True)
    costs, x, t, d, _, status = _run(P, KINDS[kind], 2, 6, **ONCHIP)
    assert all(k in t for k in OLD_NAMES) and "PCGSolveOnChip" not in t and status == 0, t.keys()
    assert d["path"] == "launch-per-iteration" and "scatter mode" in d["why_not_on_chip"], d


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_the_switch_keeps_the_four_launches(monkeypatch, energy, kind):
    P = gs._base(energy, "armadillo", False)
    want = _run(P, KINDS[kind], 2, 6)
    monkeypatch.setenv("OPT_AMD_ONCHIP", "0")
    costs, x, t, d, _, status = _run(P, KINDS[kind], 2, 6, **ONCHIP)
    assert all(k in t for k in OLD_NAMES) and "PCGSolveOnChip" not in t and status == 0, t.keys()
    assert d["path"] == "launch-per-iteration" and "switched off" in d["why_not_on_chip"], d
    assert costs == want[0] and np.array_equal(x, want[1])


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ["embedded", "robust"])
def test_level_6_with_the_fused_loop_on_1025_vertices_runs_two_launches(energy, kind):
    """Where level 6 refuses a plan it takes the loop amd_graph_fused selects, with that loop's bits."""
    P = _grid(energy, 41, 25, False)
    assert P.dims[0] == 1025 > _largest(energy, False, kind == "LM")
    a = _run(P, KINDS[kind], 2, 6, amd_graph_fused=1, **ONCHIP)
    b = _run(P, KINDS[kind], 2, 6, amd_graph_fused=1)
    t, d = a[2], a[3]
    assert "PCGStep2+PCGStep3" in t and "PCGSolveOnChip" not in t and not any(k in t for k in ("PCGStep1_Graph", "PCGStep2", "PCGStep3")), t.keys()
    assert d["launches_per_iteration"] == "2" and "too many vertices (the variants serve up to %d)" % _largest(energy, False, kind == "LM") in d["why_not_on_chip"], d
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[5] == 0


# ---- re-binding, determinism, Opt_ProblemSolve ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy,double", [pytest.param(e, d, id=f"{e}-{'f64' if d else 'f32'}") for e in ENERGIES for d in (False, True)])
def test_rebind_shuffled_and_back(energy, double):
    """One plan bound to the armadillo, to its shuffled order and to the armadillo again gives the bits of fresh plans."""
    P = gs._base(energy, "armadillo", double)
    Q = gc.reorder(P, "shuffle", seed=1)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **gs.KW, **ONCHIP)
    runs = [gs._solve(g, X) for X in (P, Q, P)]
    assert "PCGSolveOnChip" in g.kernel_timings() and g.on_chip_status() == 1
    g.close()
    ordered, shuffled = gs._fresh(P, **ONCHIP), gs._fresh(Q, **ONCHIP)
    gs._same_bits(runs[0], ordered); gs._same_bits(runs[1], shuffled); gs._same_bits(runs[2], ordered)


@pytest.mark.parametrize("energy", ENERGIES)
def test_rebind_larger_then_smaller_graph(energy):
    """A plan is made for one vertex count, so the larger graph is the armadillo plus a hub (more hyperedges: the record buffer the kernel writes grows) and back."""
    P = gs._base(energy, "armadillo", False)
    H = gc.with_hub(P, 70)
    assert H.meta["n_edges"] > P.meta["n_edges"]
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **gs.KW, **ONCHIP)
    runs = [gs._solve(g, X) for X in (P, H, P)]
    assert g.on_chip_status() == 1 and g.describe()["hyperedges"] == str(P.meta["n_edges"])
    g.close()
    small, large = gs._fresh(P, **ONCHIP), gs._fresh(H, **ONCHIP)
    gs._same_bits(runs[0], small); gs._same_bits(runs[1], large); gs._same_bits(runs[2], small)


@pytest.mark.parametrize("kind,double", [("GN", False), ("LM", True)])
@pytest.mark.parametrize("energy", ENERGIES)
def test_two_fresh_plans_give_the_same_bits(energy, kind, double):
    P = gs._base(energy, "armadillo_sub", double)
    a, b = (_run(P, KINDS[kind], 3, 12, timing=False, **ONCHIP) for _ in range(2))
    assert a[5] == b[5] == 1
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_solve_gives_the_costs_of_init_and_steps(energy, kind):
    """Opt_ProblemSolve is Opt_ProblemInit + Opt_ProblemStep until 0 on the same kernels: the same final cost and unknowns, bit for bit."""
    P = gs._base(energy, "armadillo", False)
    stepped = _run(P, KINDS[kind], 3, 12, **ONCHIP)
    g = hip_solver(P, KINDS[kind], timing=True, nIterations=3, lIterations=12, **ONCHIP)
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert "PCGSolveOnChip" in t and not any(k in t for k in OLD_NAMES) and g.on_chip_status() == 1, t.keys()
    assert g.cost() == stepped[0][-1] and np.array_equal(device_unknowns(P, dev), stepped[1])
    g.close()
