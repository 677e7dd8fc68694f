"""GPU parity tests (-m gpu) of the Levenberg-Marquardt OUTER-loop controls on every LM path of the library: function_tolerance, min_trust_region_radius,
max_trust_region_radius, radius_decrease_factor, min_lm_diagonal and max_lm_diagonal (tests/test_lm_controls_gpu.py covers the inner loop's residual_reset_period and
q_tolerance).

The accept / reject / exit logic (solverGPUGaussNewton.t:1119-1157, PcgSolver::lmDecision) and the clamp of PCGFinalizeDiagonal (:631-664; five hand-written copies:
k_finalizeDiagonal, image_warping's LMINIT march, the flag-byte table of its launch-per-iteration loop, its on-chip table, shape_from_shading's fused init -- the other
on-chip LM kernels read the CtC those produce) run at their defaults in every other test, where no exit is taken and no unknown is clamped.  Here, per path
(tests/lm_control_cases.py: PATHS) and scenario (SCENARIOS), the library is stepped beside the oracle's recorded run of the same case:
  * the same return value at every step, so the same exit step; cost, trust-region radius and final unknowns within the project's bars -- double 1e-10 (cost, relative
    to the initial cost where costs approach 0) / 1e-8 (radius) / 1e-9 (unknowns); float 1e-5 at the first step, 1e-3 later and on the radius;
  * at a function-tolerance exit the unknowns are the updated ones, cost() still reports the previous cost, and an independent cost pass over the final unknowns gives
    the oracle's new cost;
  * parameters captured at Opt_ProblemInit change nothing when set mid-solve (the same bits as the run that sets nothing), the others act on the next step;
  * a second Opt_ProblemInit on a used plan gives the bits of a fresh plan: radius, decrease factor and SSq re-seeded;
  * Opt_ProblemSolve ends where Init + Step by Step ends;
  * the path the case names is the one that ran (kernel names, on_chip_status(), describe()).
tests/test_lm_control_cases_cpu.py proves on the oracle alone that every case reaches its branch, that the clamp binds on at least 10 % of the unknowns per class, and
that no decision is a close call.
"""
import numpy as np
import pytest

import lm_control_cases as lc
from opt_amd import api
from helpers import assert_close, device_unknowns, hip_solver, rel_err

pytestmark = pytest.mark.gpu


def _plan(path, sc, double=True):
    P = lc.problem(path, double)
    return hip_solver(P, "LMGPU", timing=True, **lc.all_controls(path, sc), **lc.PATHS[path].hip)


def _assert_path(path, g):
    p = lc.PATHS[path]
    t = g.kernel_timings()
    assert ("PCGSolveOnChip" in t) == p.onchip and g.on_chip_status() == (1 if p.onchip else 0), (path, t.keys(), g.on_chip_status())
    assert all(k in t for k in p.kernels) and not any(k in t for k in p.absent), (path, t.keys())
    d = g.describe()
    assert all(sub in d[key] for key, sub in p.describe), (path, d)


def _run(path, sc, P, g, ref=None):
    """Init + Step by Step on plan g with the scenario's mid-solve changes; beside the oracle's run `ref` where given.  Returns the library's own record."""
    for k, v in lc.all_controls(path, sc).items():
        g.set_parameter(k, v)
    dev = api.to_device(P)
    g.init(dev)
    rec = lc.Run([], [g.cost()], [], None)
    dbl = P.double
    if ref:
        scale = max(abs(ref.cost[0]), 1e-300)
        assert_close("cost0", g.cost(), ref.cost[0], 1e-12 if dbl else 1e-5, double=dbl)
    for k in range(1, sc.nsteps + 2):
        b = g.step(dev)
        rec.ret.append(b); rec.cost.append(g.cost()); rec.radius.append(g.trust_region_radius())
        if ref:
            print("step", k, "ret", b, ref.ret[k - 1], "cost", g.cost(), ref.cost[k], "radius", g.trust_region_radius(), ref.radius[k - 1])
            assert b == ref.ret[k - 1], (k, rec.ret, ref.ret, rec.cost, ref.cost)
            if dbl:
                assert_close("cost", g.cost(), ref.cost[k], 1e-10, floor=1e-7 * scale, double=True, step=k)
                assert_close("radius", g.trust_region_radius(), ref.radius[k - 1], 1e-8, double=True, step=k)
            else:
                assert_close("cost" if k == 1 else "cost_later", g.cost(), ref.cost[k], 1e-5 if k == 1 else 1e-3, floor=1e-7 * scale, double=False, step=k)
                assert_close("radius", g.trust_region_radius(), ref.radius[k - 1], 1e-3, double=False, step=k)
        if not b:
            break
        for name, v in sc.changes.get(k, {}).items():
            g.set_parameter(name, v)
    rec.x = device_unknowns(P, dev)
    if ref:
        if dbl:
            assert_close("x", rel_err(rec.x, ref.x), 0.0, 1e-9, absolute=True, double=True)
        last = ref.decisions[-1]
        if len(ref.ret) <= sc.nsteps and last["accepted"]:      # a function-tolerance exit: updated unknowns, the previous cost reported, the new cost where the unknowns are
            assert rec.cost[-1] == rec.cost[-2]
            h = hip_solver(P)
            assert_close("cost_at_exit", h.eval_cost(dev), last["new"], 1e-10 if dbl else 1e-3, floor=1e-7 * scale, double=dbl)
            h.close()
    return rec


def _same_bits(a, b):
    return a.ret == b.ret and a.cost == b.cost and a.radius == b.radius and np.array_equal(a.x, b.x)


@pytest.mark.parametrize("path,name", lc.cases())
def test_double(oracle_lib, path, name):
    sc = lc.scenario(oracle_lib, path, name)
    g = _plan(path, sc)
    _run(path, sc, lc.problem(path), g, lc.oracle_run(oracle_lib, path, name))
    _assert_path(path, g)
    g.close()


@pytest.mark.parametrize("path,name", lc.float_cases())
def test_float(oracle_lib, path, name):
    sc = lc.scenario(oracle_lib, path, name)
    g = _plan(path, sc, double=False)
    _run(path, sc, lc.problem(path, False), g, lc.oracle_run(oracle_lib, path, name, double=False))
    _assert_path(path, g)
    g.close()


@pytest.mark.parametrize("path", list(lc.PATHS))
def test_parameters_captured_at_init_change_nothing_mid_solve(oracle_lib, path):
    """trust_region_radius, radius_decrease_factor, min_lm_diagonal and max_lm_diagonal set after step 2 (solver.t:996-1001 reads them in Opt_ProblemInit only): the bits
    of the run that sets nothing, through two rejected steps -- which divide by the decrease factor in force, 2 then 4 -- and two accepted ones."""
    recs = []
    for name in ("late_captured", "late_nothing"):
        sc = lc.scenario(oracle_lib, path, name)
        g = _plan(path, sc)
        recs.append(_run(path, sc, lc.problem(path), g))
        g.close()
    assert _same_bits(*recs), (recs[0].cost, recs[1].cost, recs[0].radius, recs[1].radius)


@pytest.mark.parametrize("name", lc.REINIT_AFTER)
@pytest.mark.parametrize("path", list(lc.PATHS))
def test_second_init_on_a_used_plan_equals_a_fresh_plan(oracle_lib, path, name):
    """After an exit (or five clamped steps) the plan holds a moved radius, a grown decrease factor, an SSq of other unknowns: Opt_ProblemInit re-seeds all three."""
    sc = lc.scenario(oracle_lib, path, name)
    P2 = lc.perturbed(lc.problem(path))
    ref = lc.run_oracle(oracle_lib, path, sc, P=P2)
    used = _plan(path, sc)
    _run(path, sc, lc.problem(path), used)
    again = _run(path, sc, P2, used, ref)
    _assert_path(path, used)
    used.close()
    fresh = _plan(path, sc)
    first = _run(path, sc, P2, fresh)
    fresh.close()
    assert _same_bits(again, first), (again.ret, first.ret, again.cost, first.cost, again.radius, first.radius)


@pytest.mark.parametrize("name", lc.SOLVE)
@pytest.mark.parametrize("path", lc.SOLVE_PATHS)
def test_solve_ends_where_init_and_steps_end(oracle_lib, path, name):
    """Opt_ProblemSolve is Opt_ProblemInit + Opt_ProblemStep until 0 (o.t:2548-2551) on the same kernels: the same bits."""
    sc = lc.scenario(oracle_lib, path, name)
    g = _plan(path, sc)
    stepped = _run(path, sc, lc.problem(path), g)
    g.close()
    P = lc.problem(path)
    g = _plan(path, sc)
    dev = api.to_device(P)
    g.solve(dev)
    x = device_unknowns(P, dev)
    print("cost", g.cost(), stepped.cost[-1], "radius", g.trust_region_radius(), stepped.radius[-1], "x", rel_err(x, stepped.x))
    assert g.cost() == stepped.cost[-1] and g.trust_region_radius() == stepped.radius[-1] and np.array_equal(x, stepped.x)
    _assert_path(path, g)
    g.close()
