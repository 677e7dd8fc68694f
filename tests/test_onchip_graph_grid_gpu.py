"""GPU tests (-m gpu) of the functor mesh energies' linear solve as ONE persistent launch of several workgroups (solver parameters amd_onchip = 7 and
amd_onchip_workgroups; opt_amd/csrc/graph_onchip_grid.h: ge_onchipPcgGrid<T, G, LMV>, partition: graph_partition.h) -- cotangent_mesh_smoothing,
embedded_mesh_deformation, robust_nonrigid_alignment, Gauss-Newton and Levenberg-Marquardt, float and double.

The builders, stepping routines and bars are those of test_onchip_graph_gpu.py (imported): double 1e-10 on costs / 1e-9 on the unknowns / 1e-8 on the LM radius; float
1e-5 on costs (or twice the frozen envelope where test_energies_gpu.ENVELOPES has the case) / 1e-3 on the radius.  amd_onchip_workgroups forces the workgroup count, so the
protocol between workgroups runs on meshes of 35 and 130 vertices:
  * the path is taken and visible (describe(): workgroups=G, the timer table holds PCGSolveOnChip and none of the loops' kernels, status 1), on the raptor's 2000 vertices
    too, which level 6 refuses; level 6 keeps its path text and its bits, which are level 7's with one workgroup; refusals say why; a forced count is clamped;
  * the same iterates as the four-launch loop (trace rows and unknowns at 1e-9) for 2, 3 and 8 workgroups;
  * beside the CPU oracle: trajectories per energy, solver and precision, the shuffled raptor, head.ply, graph shapes (hub, isolated and tail-only vertices, duplicate
    hyperedges, v2 == v3);
  * LM: a reset inside the solve, the q early-outs of lm_control_cases.py, the outer controls;
  * the time-out path (OPT_AMD_ONCHIP_FAIL_AT): the step is redone with the bits of a step with the path off, status 2, and the plan returns to the chip after its back-off;
  * determinism, re-binding (the partition is rebuilt), Opt_ProblemSolve.
"""
import dataclasses

import numpy as np
import pytest

import graph_cases as gc
import lm_control_cases as lc
import test_energies_gpu as te
import test_graph_shapes_gpu as gs
import test_lm_outer_controls_gpu as lmo
import test_onchip_graph_gpu as og
from test_onchip_graph_gpu import ENERGIES, FUNCTOR, KINDS, OLD_NAMES, _bars, _beside, _run
from opt_amd import api
from helpers import device_unknowns, hip_solver, rel_err

pytestmark = pytest.mark.gpu

CAP = 32      # workgroup cap of the family (graph_engine.h kGeGridMaxG)


def grid(G):
    return dict(amd_onchip=7, amd_onchip_workgroups=G)


def _check_grid(d, t, status, P, lm, G):
    n = int(P.dims[0])
    assert "PCGSolveOnChip" in t and not any(k in t for k in OLD_NAMES) and "PCGStep2+PCGStep3" not in t, t.keys()
    assert status == 1
    assert d["path"] == "on-chip" and d["workgroups"] == str(G) and d["vertices"] == str(n) and d["hyperedges"] == str(P.meta["n_edges"]), d
    assert int(d["evaluated_hyperedges"]) >= P.meta["n_edges"] and 1 <= int(d["held_vertices_max"]) <= n, d
    assert d["variant"] == "ge_onchipPcgGrid<%s, %s, %s>" % (og._prec(P.double), FUNCTOR[og._energy(P)], "LM" if lm else "GN"), d


@pytest.fixture
def grid_path_check(monkeypatch):
    """_beside checks the path through test_onchip_graph_gpu._check_path, which expects one workgroup: here the several-workgroup text."""
    def use(G):
        def check(g, P, lm, expect_onchip=True, why=None):
            assert expect_onchip
            _check_grid(g.describe(), g.kernel_timings(), g.on_chip_status(), P, lm, G)
        monkeypatch.setattr(og, "_check_path", check)
    return use


# ---- the path is taken and visible (fails without the feature: 7 is 6 there, and amd_onchip_workgroups is unknown) -----------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("mesh", ["open_patch", "armadillo"])
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_the_path_is_taken_and_visible(energy, kind, mesh, G):
    P = gs._base(energy, mesh, (G + len(mesh)) % 2 == 0)      # float and double alternate over the cases
    costs, x, t, d, _, status = _run(P, KINDS[kind], 2, 6, **grid(G))
    _check_grid(d, t, status, P, kind == "LM", G)
    assert t["PCGSolveOnChip"][0] == 2, t
    assert np.isfinite(costs).all() and np.isfinite(x).all()


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ["embedded", "robust"])
def test_the_raptor_runs_on_chip(energy, kind):
    """2000 vertices: refused by level 6 ("too many vertices").  Forced to 16 workgroups it is on chip; left to the plan it is on chip with more than one workgroup where the
    automatic table (GraphOps::ggAutoWorkgroups) names the workload and does what level 6 does elsewhere."""
    P = gs._base(energy, "raptor", False)
    costs, x, t, d, _, status = _run(P, KINDS[kind], 1, 5, **grid(16))
    _check_grid(d, t, status, P, kind == "LM", 16)
    auto = _run(P, KINDS[kind], 1, 5, amd_onchip=7)
    six = _run(P, KINDS[kind], 1, 5, amd_onchip=6)
    if auto[3]["path"] == "on-chip":
        assert int(auto[3]["workgroups"]) > 1 and auto[5] == 1, auto[3]
    else:
        assert og._without_level(auto[3]) == og._without_level(six[3]) and auto[0] == six[0] and np.array_equal(auto[1], six[1]), (auto[3], six[3])
    assert six[3]["path"] == "launch-per-iteration" and "too many vertices" in six[3]["why_not_on_chip"], six[3]


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_level_6_is_unchanged_and_is_level_7_with_one_workgroup(energy, kind):
    P = gs._base(energy, "armadillo", False)
    six = _run(P, KINDS[kind], 2, 6, amd_onchip=6)
    for params in (dict(amd_onchip=6, amd_onchip_workgroups=3), grid(1), dict(amd_onchip=7)):      # the count is consulted at level 7 only; automatic: see ggAutoWorkgroups
        r = _run(P, KINDS[kind], 2, 6, **params)
        if "amd_onchip_workgroups" not in params and r[3].get("workgroups") != "1":
            continue      # (only the automatic choice may take several workgroups here -- a table that names the armadillo: covered by the forced cases)
        assert r[3].get("workgroups") == "1", r[3]
        assert og._without_level(r[3]) == og._without_level(six[3]), (r[3], six[3])
        assert r[0] == six[0] and np.array_equal(r[1], six[1]) and r[5] == 1
    assert six[3]["workgroups"] == "1" and "ge_onchipPcg<" in six[3]["variant"], six[3]
    assert _run(P, KINDS[kind], 2, 6, amd_onchip=6, amd_onchip_workgroups=3)[3]["workgroups"] == "1"


@pytest.mark.parametrize("kind", ["GN", "LM"])
def test_refusals_say_why_and_a_forced_count_is_clamped(monkeypatch, kind):
    P = gs._base("embedded", "open_patch", False)
    n = int(P.dims[0])
    assert n == 35
    costs, x, t, d, _, status = _run(P, KINDS[kind], 2, 6, **grid(1000))      # more workgroups than the cap: the cap (every workgroup still owns a vertex)
    _check_grid(d, t, status, P, kind == "LM", min(CAP, n))
    Q = gs._base("robust", "armadillo", False)
    want = _run(Q, KINDS[kind], 2, 6)
    monkeypatch.setenv("OPT_AMD_ONCHIP", "0")
    costs, x, t, d, _, status = _run(Q, KINDS[kind], 2, 6, **grid(3))
    assert all(k in t for k in OLD_NAMES) and "PCGSolveOnChip" not in t and status == 0, t.keys()
    assert d["path"] == "launch-per-iteration" and "switched off" in d["why_not_on_chip"], d
    assert costs == want[0] and np.array_equal(x, want[1])
    monkeypatch.delenv("OPT_AMD_ONCHIP")
    monkeypatch.setenv("OPT_AMD_GRAPH_GATHER", "0")
    costs, x, t, d, _, status = _run(Q, KINDS[kind], 2, 6, **grid(3))
    assert all(k in t for k in OLD_NAMES) and "PCGSolveOnChip" not in t and status == 0, t.keys()
    assert d["path"] == "launch-per-iteration" and "scatter mode" in d["why_not_on_chip"], d


# ---- the same iterates as the four-launch loop ----------------------------------------------------------------------------------------------------------------------------------
_FOUR = {}


def _four_launch(energy, mesh):
    if (energy, mesh) not in _FOUR:
        _FOUR[(energy, mesh)] = _run(gs._base(energy, mesh, True), "gaussNewtonGPU", 1, 10, trace=True, amd_onchip=1)
    return _FOUR[(energy, mesh)]


@pytest.mark.parametrize("mesh,G", [("armadillo", 2), ("armadillo", 3), ("armadillo", 8), ("open_patch", 2)])
@pytest.mark.parametrize("energy", ENERGIES)
def test_same_iterates_as_the_four_launch_loop(energy, mesh, G):
    """The recipe and bar (1e-9) of test_onchip_graph_gpu.py::test_same_iterates_as_the_four_launch_loop: double, Gauss-Newton, 1 x 10, traced."""
    a, b = _run(gs._base(energy, mesh, True), "gaussNewtonGPU", 1, 10, trace=True, **grid(G)), _four_launch(energy, mesh)
    assert a[3]["workgroups"] == str(G) and "PCGSolveOnChip" in a[2] and "PCGStep1_Graph" in b[2]
    assert rel_err(a[1], b[1]) <= 1e-9
    ta, tb = a[4], b[4]
    assert ta.shape == tb.shape == (10, 6), (ta.shape, tb.shape)
    assert np.array_equal(ta[:, :2], tb[:, :2])
    err = np.abs(ta[:, 2:5] - tb[:, 2:5]) / np.maximum(np.abs(tb[:, 2:5]), 1e-300)
    print("largest relative difference of a trace entry:", err.max())
    assert err.max() <= 1e-9, (err.max(), np.unravel_index(err.argmax(), err.shape))


# ---- beside the oracle ----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_stages_beside_the_oracle(oracle_lib, monkeypatch, energy, double):
    """test_graph_shapes_gpu.py's stage check with every plan it makes at level 7 and three workgroups: the probes keep the record kernels."""
    monkeypatch.setattr(gs, "hip_solver", lambda P, *a, **k: hip_solver(P, *a, **k, **grid(3)))
    t = gs._check_stages(oracle_lib, gs._base(energy, "armadillo", double), timing=True)
    assert "PCGStep1_Graph" in t and t["PCGStep1"][0] == 1, t.keys()


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_trajectory_on_the_armadillo(oracle_lib, grid_path_check, energy, double, kind):
    """3 x 12, three workgroups.  cotangent in float under Gauss-Newton is held to 1 x 12: on this input the CPU oracle's own legal summation orders
    (set_reduction(1, seed), seeds 1-3, against its exact-order run) are 8.3e-8 apart after the first step and 1.07e-5, 1.08e-5 and 6.9e-6 apart after the second -- the
    reference's own spread there is the float bar of 1e-5 itself (the cost rises in that step), so no implementation can be held to it; under LM the spread stays below
    1.7e-7 over all three steps (tests/test_onchip_graph_grid_horizon_cpu.py asserts both)."""
    grid_path_check(3)
    nsteps = 1 if (energy == "cotangent" and not double and kind == "gaussNewtonGPU") else 3
    _beside(oracle_lib, gs._base(energy, "armadillo", double), kind, nsteps, 12, hip=grid(3), **_bars(double))


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
def test_the_shuffled_raptor(oracle_lib, kind):
    P = gc.reorder(gs._base("embedded", "raptor", True), "shuffle", seed=1)
    t = gs._check_trajectory(oracle_lib, P, kind, 3, 12, timing=True, **grid(16))
    assert "PCGSolveOnChip" in t and not any(k in t for k in OLD_NAMES), t.keys()


@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
def test_head_gn(oracle_lib, grid_path_check, double):
    """The horizons test_onchip_graph_gpu.py holds head.ply to (its _head says why)."""
    grid_path_check(8)
    _beside(oracle_lib, og._head(double), "gaussNewtonGPU", 2, 6, hip=grid(8), **_bars(double))


def test_head_lm_double(oracle_lib, grid_path_check):
    grid_path_check(8)
    _beside(oracle_lib, og._head(True), "LMGPU", 5, 25, hip=grid(8), **_bars(True))


@pytest.mark.parametrize("shape", ["hub", "isolated", "tail_only", "duplicates", "open_patch"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_graph_shapes(oracle_lib, energy, shape):
    """Three workgroups; the hub (degree 70) is held by every workgroup, the isolated vertex has an empty incidence list, the open patch's cotangent hyperedges repeat a vertex."""
    P = og._shape(shape, energy, True)
    g = hip_solver(P, "gaussNewtonGPU", nIterations=1, lIterations=2, **grid(3))
    dev = api.to_device(P)
    g.init(dev); g.step(dev)
    d = g.describe()
    g.close()
    assert d["path"] == "on-chip" and d["workgroups"] == "3", d
    t = gs._check_trajectory(oracle_lib, P, "gaussNewtonGPU", 2, 8, timing=True, **grid(3))
    assert t["PCGSolveOnChip"][0] == 2 and not any(k in t for k in OLD_NAMES), t.keys()


@pytest.mark.parametrize("shape", ["hub", "isolated", "tail_only", "duplicates", "open_patch"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_graph_shapes_lm_with_a_reset(oracle_lib, grid_path_check, energy, shape):
    """Levenberg-Marquardt 2 x 8 with a residual reset every third iteration, three workgroups: the hub's delta and A delta cross every workgroup in the reset's own phase."""
    grid_path_check(3)
    _beside(oracle_lib, og._shape(shape, energy, True), "LMGPU", 2, 8, hip=grid(3), residual_reset_period=3, **_bars(True))


@pytest.mark.parametrize("shape", ["hub", "isolated", "tail_only", "duplicates", "open_patch"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_graph_shapes_float_stages(oracle_lib, monkeypatch, energy, shape):
    monkeypatch.setattr(gs, "hip_solver", lambda P, *a, **k: hip_solver(P, *a, **k, **grid(3)))
    gs._check_stages(oracle_lib, og._shape(shape, energy, False))


# ---- Levenberg-Marquardt -----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_reset_inside_the_solve(oracle_lib, grid_path_check, energy, double):
    grid_path_check(3)
    _beside(oracle_lib, gs._base(energy, "armadillo", double), "LMGPU", 3, 10, hip=grid(3), residual_reset_period=3, **_bars(double))


@pytest.mark.parametrize("period,qtol,liters", og.LM_GRID)
@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_inner_controls_double(oracle_lib, grid_path_check, energy, period, qtol, liters):
    """The cases the level-6 tests run (test_onchip_graph_gpu.py::test_lm_inner_controls_double): early-outs before, on and after a reset, decided inside the kernel."""
    grid_path_check(3)
    _beside(oracle_lib, te.CASES[energy](True), "LMGPU", 4, liters, 1e-10, 1e-9, 1e-8, hip=grid(3), **og._controls(period, qtol))


GRID_PATHS = {"cotangent": dataclasses.replace(og.ONCHIP_PATHS["cotangent"], hip=grid(3))}


@pytest.mark.parametrize("base,name", lc.cases(list(GRID_PATHS)))
def test_lm_outer_controls_double(oracle_lib, base, name):
    p = GRID_PATHS[base]
    sc = lc.scenario(oracle_lib, base, name)
    P = lc.problem(base, True)
    g = hip_solver(P, "LMGPU", timing=True, **lc.all_controls(base, sc), **p.hip)
    lmo._run(base, sc, P, g, lc.oracle_run(oracle_lib, base, name, double=True))
    t, d = g.kernel_timings(), g.describe()
    assert all(k in t for k in p.kernels) and not any(k in t for k in p.absent), t.keys()
    assert d["path"] == "on-chip" and d["workgroups"] == "3", d
    g.close()


# ---- the time-out path ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fail_at", [0, 3, 9], ids=["first", "3", "last"])
@pytest.mark.parametrize("kind", ["GN", "LM"])
def test_timeout_redoes_the_step_with_the_bits_of_the_path_off(monkeypatch, kind, fail_at):
    """Workgroup 0 raises `bad` in iteration fail_at as a timed-out wait would: every workgroup leaves at that iteration's sum, nothing is applied, the solver redoes the
    linear solve on the four-launch loop and the plan is off the chip (status 2)."""
    P = gs._base("embedded", "armadillo", True)
    off = _run(P, KINDS[kind], 1, 10, amd_onchip=1)
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", str(fail_at))
    costs, x, t, d, _, status = _run(P, KINDS[kind], 1, 10, **grid(3))
    assert "PCGSolveOnChip" in t and "PCGStep1_Graph" in t and status == 2, (t.keys(), status)
    assert costs == off[0] and np.array_equal(x, off[1])
    assert d["onchip_fallbacks"] == "1" and "a wait timed out earlier" in d["why_not_on_chip"], d


@pytest.mark.parametrize("kind", ["GN", "LM"])
def test_the_plan_returns_to_the_chip_after_its_back_off(monkeypatch, kind):
    """The first on-chip launch fails; the plan stays on the loop for its back-off of eight steps (the redone step is the first of them; the eighth rearms the path and
    reports status 0), then every step is on the chip again."""
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", "2"); monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_LAUNCH", "0")
    P = gs._base("robust", "armadillo", True)
    g = hip_solver(P, KINDS[kind], timing=True, nIterations=12, lIterations=6, function_tolerance=0.0, **grid(3))
    dev = api.to_device(P)
    g.init(dev)
    status = []
    while g.step(dev):
        status.append(g.on_chip_status())
    status.append(g.on_chip_status())
    t = g.kernel_timings()
    g.close()
    assert status[:8] == [2] * 7 + [0] and len(status) >= 11 and all(s == 1 for s in status[8:]), status
    assert t["PCGSolveOnChip"][0] >= 4, (t["PCGSolveOnChip"], status)      # the failed launch and the steps behind the back-off


# ---- determinism, re-binding, Opt_ProblemSolve -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,double", [("GN", False), ("LM", True)])
@pytest.mark.parametrize("energy", ENERGIES)
def test_two_fresh_plans_give_the_same_bits(energy, kind, double):
    P = gs._base(energy, "armadillo", double)
    a, b = (_run(P, KINDS[kind], 3, 12, timing=False, residual_reset_period=5, **grid(3)) for _ in range(2))
    assert a[5] == b[5] == 1 and a[3]["workgroups"] == "3"
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("energy", ENERGIES)
def test_rebinding_another_graph_rebuilds_the_partition(energy):
    """One plan bound to the armadillo, to its hub variant (other hyperedges, another partition) and to the armadillo again gives the bits of fresh plans."""
    P = gs._base(energy, "armadillo", False)
    H = gc.with_hub(P, 70)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **gs.KW, **grid(3))
    runs = []
    for X in (P, H, P):
        runs.append(gs._solve(g, X))
        d = g.describe()
        assert d["workgroups"] == "3" and d["hyperedges"] == str(X.meta["n_edges"]) and int(d["evaluated_hyperedges"]) >= X.meta["n_edges"], d
    assert g.on_chip_status() == 1
    g.close()
    small, large = gs._fresh(P, **grid(3)), gs._fresh(H, **grid(3))
    gs._same_bits(runs[0], small); gs._same_bits(runs[1], large); gs._same_bits(runs[2], small)


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_solve_gives_the_costs_of_init_and_steps(energy, kind):
    P = gs._base(energy, "armadillo", False)
    stepped = _run(P, KINDS[kind], 3, 12, **grid(3))
    g = hip_solver(P, KINDS[kind], timing=True, nIterations=3, lIterations=12, **grid(3))
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert "PCGSolveOnChip" in t and not any(k in t for k in OLD_NAMES) and g.on_chip_status() == 1, t.keys()
    assert g.cost() == stepped[0][-1] and np.array_equal(device_unknowns(P, dev), stepped[1])
    g.close()
