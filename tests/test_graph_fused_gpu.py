"""GPU tests (-m gpu) of the two-launch PCG iteration of the functor mesh energies (solver parameter amd_graph_fused = 1; opt_amd/csrc/graph_engine.h: ge_flatStep +
ge_gather) -- cotangent_mesh_smoothing, embedded_mesh_deformation, robust_nonrigid_alignment, Gauss-Newton and Levenberg-Marquardt, float and double.

  * the path is taken and visible (kernel names and counts, describe()), and with the parameter at 0 or under amd_reference_order = 1 nothing changes, bits included;
  * J^T J p of ge_gather equals the record path's (ge_edges + ge_vertices) bit for bit, its p . A p to 1e-12: the same terms in another order of a double sum;
  * the same iterates as the four-launch loop (trace rows at 1e-9, the bar of test_onchip_arap_gpu.py::test_same_iterates_as_the_two_kernel_loop);
  * beside the CPU oracle: stages, trajectories, LM inner controls (residual_reset_period, q_tolerance) and LM outer controls, with the bars, builders and stepping
    routines of the existing tests, imported;
  * re-binding, determinism, Opt_ProblemSolve, and the fallback in scatter mode.
Shapes: open_patch (35 vertices, one workgroup, hyperedges with v2 == v3), armadillo (130 vertices, three workgroups per pass), raptor (2000 vertices, valence 3..12).
"""
import dataclasses
import itertools

import numpy as np
import pytest

import graph_cases as gc
import lm_control_cases as lc
import test_energies_gpu as te
import test_graph_shapes_gpu as gs
import test_lm_controls_gpu as lmc
import test_lm_outer_controls_gpu as lmo
from opt_amd import api
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

FUSED = dict(amd_graph_fused=1)
ENERGIES = gc.FUNCTOR_ENERGIES
FUNCTOR = {"cotangent": "CotangentG", "embedded": "EmbeddedG", "robust": "RobustG"}
KINDS = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}
# (precision, functor, LM) of every ge_gather instantiation the library offers; tests/test_graph_fused_resources.py holds the list against the build
GATHER_VARIANTS = [(p, FUNCTOR[e], lm) for e in ENERGIES for p in ("float", "double") for lm in (False, True)]
OLD_NAMES = ("PCGStep1_Graph", "PCGStep1", "PCGStep2", "PCGStep3")


def _run(P, kind, nsteps, liters, timing=True, trace=False, **params):
    """(costs after init and every step, final unknowns, timer table, describe(), trace) of Init + Step by Step."""
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
    out = (costs, device_unknowns(P, dev), g.kernel_timings() if timing else None, g.describe(), g.trace() if trace else None)
    g.close()
    return out


# ---- the path is taken and visible ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,functor,lm", GATHER_VARIANTS, ids=lambda v: str(v))
def test_the_fused_path_is_taken_and_visible(prec, functor, lm):
    energy = {v: k for k, v in FUNCTOR.items()}[functor]
    P = gs._base(energy, "armadillo", prec == "double")
    costs, x, t, d, _ = _run(P, KINDS["LM" if lm else "GN"], 2, 6, **FUSED)
    assert "PCGStep2+PCGStep3" in t and "PCGStep1" in t, t.keys()
    assert not any(k in t for k in ("PCGStep1_Graph", "PCGStep2", "PCGStep3")), t.keys()
    if not lm:
        assert t["PCGStep2+PCGStep3"][0] == 2 * 5 and t["PCGStep1"][0] == 2 * 6, t
    else:      # (a q early-out may end a linear solve before its sixth iteration)
        assert 0 < t["PCGStep2+PCGStep3"][0] <= 2 * 5 and t["PCGStep2+PCGStep3"][0] < t["PCGStep1"][0] <= 2 * 6, t
    assert d["path"] == "launch-per-iteration" and d["launches_per_iteration"] == "2", d
    assert d["kernels"] == f"ge_flatStep+ge_gather<{prec}, {functor}, {'LM' if lm else 'GN'}>", d
    assert np.isfinite(costs).all() and costs[-1] <= costs[0]


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
@pytest.mark.parametrize("params", [dict(amd_graph_fused=0), dict(amd_graph_fused=1, amd_reference_order=1)], ids=["unset", "reference_order"])
def test_nothing_changes_without_the_parameter(energy, kind, params):
    """amd_graph_fused = 0, and amd_graph_fused = 1 under amd_reference_order = 1 (which wins): the four launches, today's describe(), and the bits of a plan that
    never heard of the parameter."""
    P = gs._base(energy, "armadillo", False)
    never = {k: v for k, v in params.items() if k != "amd_graph_fused"}
    a = _run(P, KINDS[kind], 2, 6, **params)
    b = _run(P, KINDS[kind], 2, 6, **never)
    assert all(k in a[2] for k in OLD_NAMES) and "PCGStep2+PCGStep3" not in a[2], a[2].keys()
    assert a[3] == b[3] and "launches_per_iteration" not in a[3] and "why_not_fused" not in a[3], (a[3], b[3])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert {k: c for k, (c, _) in a[2].items()} == {k: c for k, (c, _) in b[2].items()}


# ---- A p bit for bit ------------------------------------------------------------------------------------------------------------------------------------------------
def _probe_problem(energy, shape, double):
    if shape in ("open_patch", "armadillo"):
        return gs._base(energy, shape, double)
    if shape == "raptor-shuffle":
        return gc.reorder(gs._base(energy, "raptor", double), "shuffle", seed=1)
    B = gs._base(energy, "armadillo", double)
    return {"hub": lambda: gc.with_hub(B, 70), "isolated": lambda: gc.with_isolated_vertex(B), "tail_only": lambda: gc.with_tail_only_vertex(B),
            "duplicates": lambda: gc.with_duplicate_edges(B, 9)}[shape]()


PROBE_SHAPES = ("open_patch", "armadillo", "raptor-shuffle", "hub", "isolated", "tail_only", "duplicates")


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", PROBE_SHAPES)
@pytest.mark.parametrize("energy", ENERGIES)
def test_apply_jtj_bit_for_bit(energy, shape, double):
    """ge_gather against ge_edges<3> + ge_vertices<3>: `out` identical, the dot within 1e-12 in both precisions (the summed terms are the same numbers)."""
    import torch
    P = _probe_problem(energy, shape, double)
    n = sum(int(np.asarray(P.params[s]).size) for s in P.unknown_slots)
    v = torch.from_numpy(np.random.default_rng(11).standard_normal(n).astype(np.float64 if double else np.float32)).cuda()
    res = {}
    for fused in (0, 1):
        g = hip_solver(P, timing=True, amd_graph_fused=fused)
        dev = api.to_device(P)
        out, dot = g.apply_jtj(dev, v)
        t = g.kernel_timings()
        assert ("PCGStep1_Graph" in t) == (fused == 0) and t["PCGStep1"][0] == 1, t.keys()
        res[fused] = (out.clone(), dot)
        g.close()
    print("dot", res[1][1], res[0][1], abs(res[1][1] - res[0][1]) / abs(res[0][1]))
    assert torch.isfinite(res[0][0]).all() and float(res[0][0].abs().max()) > 0
    assert torch.equal(res[1][0], res[0][0]), float((res[1][0] - res[0][0]).abs().max())
    assert_close("dot", res[1][1], res[0][1], 1e-12, double=double)


# ---- the same iterates as the four-launch loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy", ENERGIES)
def test_same_iterates_as_the_four_launch_loop(energy):
    """The recipe and bar (1e-9) of test_onchip_arap_gpu.py::test_same_iterates_as_the_two_kernel_loop: double, Gauss-Newton, 1 x 10 on the armadillo, traced."""
    P = gs._base(energy, "armadillo", True)
    res = {f: _run(P, "gaussNewtonGPU", 1, 10, trace=True, amd_graph_fused=f) for f in (1, 0)}
    assert "PCGStep2+PCGStep3" in res[1][2] and "PCGStep2+PCGStep3" not in res[0][2] and "PCGStep1_Graph" in res[0][2]
    assert rel_err(res[1][1], res[0][1]) <= 1e-9
    a, b = res[1][4], res[0][4]
    assert a.shape == b.shape == (10, 6), (a.shape, b.shape)
    assert np.array_equal(a[:, :2], b[:, :2])      # (outer step, PCG iteration)
    err = np.abs(a[:, 2:5] - b[:, 2:5]) / np.maximum(np.abs(b[:, 2:5]), 1e-300)
    print("largest relative difference of a trace entry:", err.max())
    assert err.max() <= 1e-9, (err.max(), np.unravel_index(err.argmax(), err.shape))


# ---- beside the oracle ----------------------------------------------------------------------------------------------------------------------------------------------------
def _fused_solver(P, *a, **k):
    return hip_solver(P, *a, **k, **FUSED)


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh,how", [("armadillo", None), ("raptor", "shuffle")])
@pytest.mark.parametrize("energy", ENERGIES)
def test_stages_beside_the_oracle(oracle_lib, monkeypatch, energy, mesh, how, double):
    """test_graph_shapes_gpu.py's stage check (1e-11 / 3e-5 norm-wise) with every plan it makes under the parameter."""
    monkeypatch.setattr(gs, "hip_solver", _fused_solver)
    P = gs._base(energy, mesh, double)
    t = gs._check_stages(oracle_lib, gc.reorder(P, how, seed=1) if how else P, timing=True)
    assert "PCGStep1_Graph" not in t and t["PCGStep1"][0] == 1, t.keys()


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["cotangent", "embedded", "embedded_rest", "robust"])
def test_trajectory(oracle_lib, name, double, kind):
    """test_energies_gpu.py::test_trajectory's recipe on its CASES, 4 x 12: its bars (1e-10 / 1e-9 in double; 1e-5 / 2e-5 in float, or twice the frozen envelope of legal
    float runs where ENVELOPES has the case), the same accept / reject sequence, and the LM radius at 1e-8 in double.  (In float 1e-8 lies below the unit roundoff
    6e-8, so the radius takes the project's float bar, 1e-3: test_lm_controls_gpu.py, test_lm_outer_controls_gpu.py.)"""
    P = te.CASES[name](double)
    kw = dict(nIterations=4, lIterations=12)
    o = oracle_solver(oracle_lib, P, kind, **kw)
    g = hip_solver(P, kind, timing=True, **kw, **FUSED)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    ctol, xtol = (1e-10, 1e-9) if double else (1e-5, 2e-5)
    if not double:
        env = te.ENVELOPES.get(f"{name}_{kind}")
        if env is not None:
            ctol, xtol = max(ctol, 2.0 * env[0]), max(xtol, 2.0 * env[1])
    scale = max(abs(o.cost()), 1e-300)
    assert_close("cost0", g.cost(), o.cost(), 1e-12 if double else 1e-5, floor=scale, double=double)
    step = 0
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        step += 1
        print("step", step, a, b, "cost", g.cost(), o.cost(), abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-7 * scale), "radius", g.trust_region_radius(), o.trust_region_radius())
        assert a == b
        assert_close("cost", g.cost(), o.cost(), ctol, floor=1e-7 * scale, double=double, step=step)
        if kind == "LMGPU":
            assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), 1e-8 if double else 1e-3, double=double, step=step)
        if not a:
            break
    x = rel_err(device_unknowns(P, dev), flat_unknowns(Pref))
    print("x", x, xtol)
    assert_close("x", x, 0.0, xtol, absolute=True, double=double)
    t = g.kernel_timings()
    assert "PCGStep2+PCGStep3" in t and "PCGStep1_Graph" not in t and "PCGStep3" not in t, t.keys()
    g.close(); o.close()


def test_raptor_trajectory_double(oracle_lib):
    """test_graph_shapes_gpu.py::_check_trajectory's bars on the shuffled raptor: embedded, Gauss-Newton 3 x 12."""
    P = gc.reorder(gs._base("embedded", "raptor", True), "shuffle", seed=1)
    t = gs._check_trajectory(oracle_lib, P, "gaussNewtonGPU", 3, 12, timing=True, **FUSED)
    assert t["PCGStep2+PCGStep3"][0] == 3 * 11 and t["PCGStep1"][0] == 3 * 12 and "PCGStep1_Graph" not in t, t


# ---- LM inner controls ----------------------------------------------------------------------------------------------------------------------------------------------------
def _arap_grid():
    """(period, qtol, liters) of test_lm_controls_gpu.py::test_arap_two_kernel_lm_iteration_controls"""
    for m in lmc.test_arap_two_kernel_lm_iteration_controls.pytestmark:
        if m.name == "parametrize" and m.args[0] == "period,qtol,liters":
            return list(m.args[1])
    raise AssertionError("the grid of test_arap_two_kernel_lm_iteration_controls has moved")


# its q_tolerance values (None: the default 1e-4; 0: never; 0.05 / 0.5 / 5: early-outs on, next to and between resets) against the reset periods, at lIterations = 12
QTOLS = sorted({q for _, q, _ in _arap_grid()}, key=lambda q: -1.0 if q is None else q)
PERIODS = (1, 3, 5, 10)
LM_CASES = {"cotangent": "cotangent", "embedded": "embedded", "robust": "robust"}      # test_energies_gpu.CASES: cotangent 19 x 13, embedded 17 x 11, robust 15 x 12


def _controls(period, qtol):
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    return kw


@pytest.mark.parametrize("period,qtol", list(itertools.product(PERIODS, QTOLS)))
@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_inner_controls_double(oracle_lib, energy, period, qtol):
    """Step for step beside the oracle at 1e-10 (cost) / 1e-9 (unknowns) / 1e-8 (radius), and the fused loop is the one that ran -- with the split residual reset on
    ge_gather (computeAdelta) where a reset falls inside the solve."""
    P = te.CASES[LM_CASES[energy]](True)
    lmc._side_by_side(oracle_lib, P, 4, 12, 1e-10, 1e-9, 1e-8, hip_only=FUSED, **_controls(period, qtol))
    _, _, t, _, _ = _run(P, "LMGPU", 1, 12, **FUSED, **_controls(period, qtol))
    assert "PCGStep1" in t and not any(k in t for k in ("PCGStep1_Graph", "PCGStep2", "PCGStep3")), t.keys()
    if period < 12 and qtol == 0.0:      # (no early-out: the reset before the last iteration is reached)
        assert "PCGStep2_2ndHalf" in t, t.keys()


@pytest.mark.parametrize("energy", ENERGIES)
def test_lm_inner_controls_float(oracle_lib, energy):
    """One float run per energy: 1e-5 on the first step's cost (radius: the project's float bar 1e-3)."""
    P = te.CASES[LM_CASES[energy]](False)
    lmc._side_by_side(oracle_lib, P, 1, 12, 1e-5, None, 1e-3, hip_only=FUSED, residual_reset_period=5)


# ---- LM outer controls ----------------------------------------------------------------------------------------------------------------------------------------------------
FUSED_PATHS = {base: dataclasses.replace(lc.PATHS[base], hip=dict(FUSED), kernels=("PCGStep2+PCGStep3", "PCGStep1"), absent=("PCGStep1_Graph", "PCGStep3"))
               for base in ("cotangent", "embedded")}


def _assert_path(p, g):
    """test_lm_outer_controls_gpu.py::_assert_path for a Path that lm_control_cases.PATHS does not hold"""
    t = g.kernel_timings()
    assert "PCGSolveOnChip" not in t and g.on_chip_status() == 0, t.keys()
    assert all(k in t for k in p.kernels) and not any(k in t for k in p.absent), t.keys()
    assert g.describe()["launches_per_iteration"] == "2"


def _outer(oracle_lib, base, name, double):
    """The oracle side of a fused path is its base path's (the same problem and controls): lm_control_cases.oracle_run, proved by tests/test_lm_control_cases_cpu.py."""
    p = FUSED_PATHS[base]
    sc = lc.scenario(oracle_lib, base, name)
    P = lc.problem(base, double)
    g = hip_solver(P, "LMGPU", timing=True, **lc.all_controls(base, sc), **p.hip)
    lmo._run(base, sc, P, g, lc.oracle_run(oracle_lib, base, name, double=double))
    _assert_path(p, g)
    g.close()


@pytest.mark.parametrize("base,name", lc.cases(list(FUSED_PATHS)))
def test_lm_outer_controls_double(oracle_lib, base, name):
    _outer(oracle_lib, base, name, True)


@pytest.mark.parametrize("base,name", [(p, s) for p, s in lc.cases(list(FUSED_PATHS)) if lc.PATHS[p].float_too])
def test_lm_outer_controls_float(oracle_lib, base, name):
    _outer(oracle_lib, base, name, False)


# ---- re-binding and determinism ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy,double", [pytest.param(e, d, id=f"{e}-{'f64' if d else 'f32'}") for e in ENERGIES for d in (False, True)])
def test_rebind_shuffled_and_back(energy, double):
    """One plan bound to the armadillo, to its shuffled order and to the armadillo again gives the bits of fresh plans."""
    P = gs._base(energy, "armadillo", double)
    Q = gc.reorder(P, "shuffle", seed=1)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, **gs.KW, **FUSED)
    runs = [gs._solve(g, X) for X in (P, Q, P)]
    assert "PCGStep2+PCGStep3" in g.kernel_timings()
    g.close()
    ordered, shuffled = gs._fresh(P, **FUSED), gs._fresh(Q, **FUSED)
    gs._same_bits(runs[0], ordered); gs._same_bits(runs[1], shuffled); gs._same_bits(runs[2], ordered)


@pytest.mark.parametrize("double", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_two_fresh_plans_give_the_same_bits(energy, kind, double):
    P = gs._base(energy, "armadillo", double)
    a, b = (_run(P, KINDS[kind], 3, 12, timing=False, **FUSED) for _ in range(2))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_solve_gives_the_costs_of_init_and_steps(energy, kind):
    """Opt_ProblemSolve is Opt_ProblemInit + Opt_ProblemStep until 0 on the same kernels: the same final cost and unknowns, bit for bit."""
    P = gs._base(energy, "armadillo", False)
    stepped = _run(P, KINDS[kind], 3, 12, **FUSED)
    g = hip_solver(P, KINDS[kind], timing=True, nIterations=3, lIterations=12, **FUSED)
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert "PCGStep2+PCGStep3" in t and "PCGStep1_Graph" not in t, t.keys()
    assert g.cost() == stepped[0][-1] and np.array_equal(device_unknowns(P, dev), stepped[1])
    g.close()


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["GN", "LM"])
@pytest.mark.parametrize("energy", ENERGIES)
def test_scatter_mode_keeps_the_four_launches(monkeypatch, energy, kind):
    monkeypatch.setenv("OPT_AMD_GRAPH_GATHER", "0")
    P = gs._base(energy, "armadillo", True)
    costs, x, t, d, _ = _run(P, KINDS[kind], 2, 6, **FUSED)
    assert all(k in t for k in OLD_NAMES) and "PCGStep2+PCGStep3" not in t, t.keys()
    assert "launches_per_iteration" not in d and "scatter mode" in d["why_not_fused"], d
