"""GPU parity tests (-m gpu) of the on-chip linear solve for a general UrShape (opt_amd/csrc/iw_onchip.h, iw_onchipPcgGeneral): image_warping, Gauss-Newton and
Levenberg-Marquardt, solver parameter amd_onchip = 4.

image_warping.t:4 declares UrShape as an ordinary input array; by default only the unit pixel lattice takes the on-chip solve (tests/test_onchip_gpu.py,
tests/test_onchip_lm_gpu.py) and any other rest shape streams (one launch per PCG iteration).  With amd_onchip = 4 a general UrShape keeps the solve on chip too: the same
protocol, with U_c - U_n read per pixel and the Angle channel of the Jacobi preconditioner (LM: and of CtC) read once from the solver's vectors instead of a table.
Everything here runs on a jittered UrShape (workloads.image_warping(jitter_urshape=0.2)) against the CPU oracle, which evaluates a general UrShape already:
  * the opt-in gate (level 4 on chip, the default streams);
  * every general variant (GENERAL_VARIANTS, forced with OPT_AMD_ONCHIP_ROWS) on small and ragged images with masks, the iteration counts / reset periods of the lattice tests;
  * the same iterates as the streaming general loop; a lattice input at level 4 = level 1, bitwise;
  * UrShape leaving the lattice and coming back between steps (lattice kernel, general kernel, lattice kernel);
  * rejected LM steps, the q early-out, the tag counter over many steps, tree and flat grid sums;
  * the time-out path, also among the deferred steps of Opt_ProblemSolve;
  * the reference's own input sizes on the natural variant, and an image that is too large.
Bars (the project's: tests/test_onchip_gpu.py, tests/test_onchip_lm_gpu.py, BASELINE.json north star): double 1e-10 on costs / 1e-8 on the LM radius / 1e-9 on the unknowns;
float 1e-5 on the cost of the first outer step, 2e-5 on the unknowns (Gauss-Newton), 1e-3 on LM outer steps after the first (hand-over of the loop state).
"""
import os

import numpy as np
import pytest

from opt_amd import api, workloads as wl
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

THREADS = max(1, min(os.cpu_count() or 1, 64))
JIT = 0.2

# (precision, rows per lane, Levenberg-Marquardt) of every kernel iw_onchipPcgGeneral<T, ROWS, LMV> the library offers: the variant tests force each one
# (tests/test_onchip_general_resources.py checks that this is exactly the set instantiated)
GENERAL_VARIANTS = [("float", 2, False), ("float", 4, False), ("float", 2, True), ("float", 4, True), ("double", 2, False), ("double", 2, True)]


def _rows(prec, lmv):
    return [r for p, r, l in GENERAL_VARIANTS if p == prec and l == lmv]


def _ran_onchip(g):
    return "PCGSolveOnChip" in g.kernel_timings()


def _pair(oracle_lib, P, nsteps, liters, cost_tol, x_tol, expect_onchip=True, level=4):
    """Gauss-Newton, step by step beside the oracle (tests/test_onchip_gpu.py::_pair with the plan opted in)."""
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", nIterations=nsteps, lIterations=liters)
    o.set_threads(THREADS if P.params[0].size > 200_000 else 1)
    kw = {} if level is None else {"amd_onchip": level}
    g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=nsteps, lIterations=liters, **kw)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        assert_close("cost", g.cost(), o.cost(), cost_tol, floor=1e-12 * scale, double=P.double)
        if not a:
            break
    t = g.kernel_timings()
    assert _ran_onchip(g) == expect_onchip, t.keys()
    assert ("PCGIteration" in t) == (not expect_onchip), t.keys()
    assert g.on_chip_status() == (1 if expect_onchip else 0)
    if x_tol is not None:
        assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, x_tol, absolute=True, double=P.double)
    g.close(); o.close()


def _side_by_side(oracle_lib, P, nsteps, liters, cost_tol, x_tol, radius_tol, expect_onchip=True, threads=1, later_tol=None, level=4, **controls):
    """Levenberg-Marquardt, step by step beside the oracle (tests/test_onchip_lm_gpu.py::_side_by_side with the plan opted in)."""
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=nsteps, lIterations=liters, **controls)
    o.set_threads(threads)
    kw = dict(controls) if level is None else dict(controls, amd_onchip=level)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=nsteps, lIterations=liters, **kw)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    costs = [(o.cost(), g.cost())]
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b, (a, b, costs)
        costs.append((o.cost(), g.cost()))
        tol = cost_tol if (later_tol is None or len(costs) <= 2) else later_tol      # later_tol: outer steps after the first (float runs, see test_variants_lm_float)
        assert_close("cost" if len(costs) <= 2 else "cost_later", g.cost(), o.cost(), tol, floor=1e-12 * scale, double=P.double, step=len(costs) - 1)
        if later_tol is None or len(costs) <= 2:
            assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), radius_tol, double=P.double)
        if not a:
            break
    t = g.kernel_timings()
    assert _ran_onchip(g) == expect_onchip, t.keys()
    assert ("PCGIteration" in t) == (not expect_onchip), t.keys()
    assert g.on_chip_status() == (1 if expect_onchip else 0)
    if x_tol is not None:
        assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, x_tol, absolute=True, double=P.double)
    g.close(); o.close()
    return costs


# ---- the opt-in gate -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm", [False, True])
def test_level_4_keeps_a_general_urshape_on_chip(oracle_lib, lm):
    P = wl.image_warping(300, 100, double=True, random_state=2, perturb=0.3, jitter_urshape=JIT)
    if lm:
        _side_by_side(oracle_lib, P, 2, 6, 1e-10, 1e-9, 1e-8)
    else:
        _pair(oracle_lib, P, 2, 4, 1e-10, 1e-9)


@pytest.mark.parametrize("lm", [False, True])
def test_the_default_level_streams_a_general_urshape(oracle_lib, lm):
    P = wl.image_warping(300, 100, double=True, random_state=2, perturb=0.3, jitter_urshape=JIT)
    if lm:
        _side_by_side(oracle_lib, P, 2, 6, 1e-10, 1e-9, 1e-8, expect_onchip=False, level=None)
    else:
        _pair(oracle_lib, P, 2, 4, 1e-10, 1e-9, expect_onchip=False, level=None)


# ---- every variant ------------------------------------------------------------------------------------------------------------------------------------------------------------
# one tile; tiles across (x) with a partial last tile; tiles down; both; a single pixel column; fewer rows than one wave holds
SHAPES = [(96, 64), (300, 40), (517, 33), (64, 300), (260, 131), (1, 70), (700, 3), (257, 9)]


def _problem(W, H, double, perturb):
    return wl.image_warping(W, H, double=double, random_state=W * 7 + H, mask_fraction=0.1, perturb=perturb, jitter_urshape=JIT)


@pytest.mark.parametrize("liters", [1, 2, 3, 7, 8])
@pytest.mark.parametrize("rows", _rows("double", False))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_gn_double(oracle_lib, monkeypatch, W, H, rows, liters):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows))
    _pair(oracle_lib, _problem(W, H, True, 0.3), 2, liters, 1e-10, 1e-9)


@pytest.mark.parametrize("liters", [3, 8, 20])
@pytest.mark.parametrize("rows", _rows("float", False))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_gn_float(oracle_lib, monkeypatch, W, H, rows, liters):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows))
    _pair(oracle_lib, _problem(W, H, False, 0.3), 2, liters, 1e-5, 2e-5)


@pytest.mark.parametrize("liters,period", [(9, 10), (10, 10), (10, 3), (12, 5), (7, 1), (12, 2)])
@pytest.mark.parametrize("rows", _rows("double", True))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_lm_double(oracle_lib, monkeypatch, W, H, rows, liters, period):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows))
    _side_by_side(oracle_lib, _problem(W, H, True, 0.3), 3, liters, 1e-10, 1e-9, 1e-8, residual_reset_period=period)


@pytest.mark.parametrize("liters,period", [(10, 10), (12, 5), (25, 10), (9, 2)])
@pytest.mark.parametrize("rows", _rows("float", True))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_lm_float(oracle_lib, monkeypatch, W, H, rows, liters, period):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows))
    # q_tolerance = -1e9 (never: 0 would still break on a NEGATIVE zeta, which in float happens behind a residual reset when Q is not monotone to the last bit): in float the
    # zeta test can sit on a knife's edge (tests/test_onchip_lm_gpu.py::test_variants_float: 517 x 33, period 2, zeta = 0.996e-4 against 1e-4 at k = 6 -- the oracle breaks, every
    # HIP loop, streaming or on chip, goes on); the decisions themselves are pinned in double (test_variants_lm_double, test_q_early_out_double), the float runs pin the arithmetic.
    # The first outer step holds the float contract (1e-5); the steps after it start from unknowns that already differ in their last bits and check the hand-over of the loop
    # state between launches (phase tags, trust region), at 1e-3.
    _side_by_side(oracle_lib, _problem(W, H, False, 0.3), 3, liters, 1e-5, None, 1e-3, residual_reset_period=period, q_tolerance=-1e9, later_tol=1e-3)


# ---- against the streaming general loop, and against level 1 on a lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
def test_same_iterates_as_the_streaming_general_loop(double):
    res = []
    for level in (4, 0):
        P = wl.image_warping(600, 300, double=double, random_state=11, mask_fraction=0.05, perturb=0.3, jitter_urshape=JIT)
        g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=2, lIterations=15, amd_onchip=level)
        dev = api.to_device(P)
        g.solve(dev)
        assert _ran_onchip(g) == (level == 4)
        res.append((g.cost(), device_unknowns(P, dev)))
        g.close()
    tol = 1e-11 if double else 2e-5
    assert abs(res[0][0] - res[1][0]) <= tol * abs(res[1][0]), (res[0][0], res[1][0])
    assert rel_err(res[0][1], res[1][1]) < (1e-10 if double else 2e-5)


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
def test_a_lattice_input_at_level_4_is_level_1_bitwise(kind):
    res = []
    for level in (4, 1):
        P = wl.image_warping(300, 120, random_state=6, mask_fraction=0.05, perturb=0.3)
        g = hip_solver(P, kind, timing=True, nIterations=3, lIterations=9, amd_onchip=level)
        dev = api.to_device(P)
        g.solve(dev)
        assert _ran_onchip(g) and "PCGIteration" not in g.kernel_timings()
        res.append((g.cost(), device_unknowns(P, dev)))
        g.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1])


def test_urshape_leaves_the_lattice_and_comes_back_all_on_chip(oracle_lib):
    """tests/test_image_warping_gpu.py::test_urshape_leaves_the_lattice_between_two_steps at level 4: step 1 on the lattice kernel, step 2 -- UrShape moved off the lattice in
    place, PCGInit1 redone as the general march, which also leaves M_a -- on the general kernel, step 3 back on the lattice kernel; each against the oracle."""
    import torch
    P = wl.image_warping(150, 97, double=True, random_state=21, mask_fraction=0.05, perturb=0.3)
    o = oracle_solver(oracle_lib, P, nIterations=3, lIterations=9)
    g = hip_solver(P, timing=True, nIterations=3, lIterations=9, amd_onchip=4)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    assert o.step(Pref.params) and g.step(dev)
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert g.on_chip_status() == 1
    rng = np.random.default_rng(5)
    lattice = np.array(Pref.params[2], copy=True)
    jit = 0.03 * rng.standard_normal(Pref.params[2].shape)
    Pref.params[2][...] = lattice + jit                               # UrShape (binding index 2), in place on both sides
    dev[2].copy_(torch.from_numpy(lattice + jit).cuda())
    assert o.step(Pref.params) and g.step(dev)
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert g.on_chip_status() == 1
    Pref.params[2][...] = lattice
    dev[2].copy_(torch.from_numpy(lattice).cuda())
    o.step(Pref.params); g.step(dev)
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert g.on_chip_status() == 1
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    t = g.kernel_timings()
    assert t["PCGSolveOnChip"][0] == 3 and "PCGIteration" not in t, t
    g.close(); o.close()


# ---- controls (double) ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rejected_steps_shrink_the_radius_and_restore_the_unknowns(oracle_lib):
    for radius in (1e-2, 1e12):
        P = wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.6, jitter_urshape=JIT)
        _side_by_side(oracle_lib, P, 6, 12, 1e-10, 1e-9, 1e-8, trust_region_radius=radius)


@pytest.mark.parametrize("qtol", [None, 0.0, 0.05, 0.5, 5.0])
@pytest.mark.parametrize("period", [1, 2, 3, 10])
def test_q_early_out_double(oracle_lib, period, qtol):
    P = wl.image_warping(300, 77, double=True, random_state=7 + period, mask_fraction=0.05, perturb=0.4, jitter_urshape=JIT)
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    _side_by_side(oracle_lib, P, 4, 30, 1e-10, 1e-9, 1e-8, **kw)


def test_many_steps_tag_counter_runs_on(oracle_lib):
    """9 x 5 launches on one plan: tags never repeat, the double buffers alternate whatever the parity of the counts.
    The input: nine under-converged Gauss-Newton steps amplify last-bit differences about tenfold per step, by an amount that depends on the seed.  The oracle under the
    reference's own summation order (set_reduction(1, seed), seeds 1-3) against its exact-order run, relative cost after step 9 on 260 x 131, jitter 0.2: random_state 21 (the
    lattice test's) 4.0e-10 -- the reference does not reproduce itself to the 1e-10 bar there, so nothing can be held to it --, 22: 7.9e-12, 23: 4.8e-12.  Seed 23 leaves the
    bar 20 x the reference's own spread."""
    P = wl.image_warping(260, 131, double=True, random_state=23, mask_fraction=0.05, perturb=0.3, jitter_urshape=JIT)
    _pair(oracle_lib, P, 9, 5, 1e-10, 1e-9)


@pytest.mark.parametrize("flat", [0, 1000])
def test_grid_sum_tree_and_flat(oracle_lib, monkeypatch, flat):
    """520 x 200 at 2 rows per lane: 3 x 50 = 150 workgroups, ten groups of 16 (the last one partial); the tree (OPT_AMD_ONCHIP_FLAT=0) and the flat sum add in the same order."""
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", "2")
    monkeypatch.setenv("OPT_AMD_ONCHIP_FLAT", str(flat))
    P = wl.image_warping(520, 200, double=True, random_state=722, mask_fraction=0.05, perturb=0.3, jitter_urshape=JIT)
    _pair(oracle_lib, P, 2, 9, 1e-10, 1e-9)


# ---- the time-out path --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("fail_at", [0, 3])
def test_a_timed_out_wait_leaves_the_unknowns_alone_and_the_step_is_redone(oracle_lib, monkeypatch, capfd, fail_at, kind):
    """OPT_AMD_ONCHIP_FAIL_AT: workgroup 0 raises the failure flag in that iteration as a timed-out wait would; nothing is applied, the streaming general loop redoes the step."""
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", str(fail_at))
    P = wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.3, jitter_urshape=JIT)
    o = oracle_solver(oracle_lib, P, kind, nIterations=3, lIterations=8)
    Pref = P.clone()
    o.solve(Pref.params)
    g = hip_solver(P, kind, timing=True, nIterations=3, lIterations=8, amd_onchip=4)
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert 1 <= t["PCGSolveOnChip"][0] <= 3 and "PCGIteration" in t, t
    assert g.on_chip_status() == 2
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    assert "timed out" in capfd.readouterr().err
    g.close(); o.close()


def test_a_time_out_among_deferred_steps_sends_the_solve_back_to_that_step(oracle_lib, monkeypatch, capfd):
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", "3")
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_LAUNCH", "2")
    P = wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.3, jitter_urshape=JIT)
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", nIterations=6, lIterations=8)
    Pref = P.clone()
    o.solve(Pref.params)
    g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=6, lIterations=8, amd_onchip=4)
    dev = api.to_device(P)
    g.solve(dev)
    t = g.kernel_timings()
    assert "PCGIteration" in t and "PCGSolveOnChip" in t, t.keys()
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    assert "timed out" in capfd.readouterr().err
    g.close(); o.close()


# ---- the sizes the path exists for ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(512, 512), (640, 480)])
def test_natural_variant_gn_float(oracle_lib, W, H):
    P = wl.image_warping(W, H, random_state=W + H, mask_fraction=0.02, perturb=0.3, jitter_urshape=JIT)
    _pair(oracle_lib, P, 2, 10, 1e-5, 2e-5)


@pytest.mark.parametrize("W,H", [(512, 512), (640, 480)])
def test_natural_variant_lm_float(oracle_lib, W, H):
    P = wl.image_warping(W, H, random_state=W + H, mask_fraction=0.02, perturb=0.3, jitter_urshape=JIT)
    _side_by_side(oracle_lib, P, 2, 10, 1e-5, None, 1e-3, threads=THREADS, later_tol=1e-3, q_tolerance=-1e9)


def test_natural_variant_gn_double_512(oracle_lib):
    P = wl.image_warping(512, 512, double=True, random_state=9, mask_fraction=0.02, perturb=0.3, jitter_urshape=JIT)
    _pair(oracle_lib, P, 2, 10, 1e-10, 1e-9)


def test_too_large_an_image_streams_and_describe_says_why(oracle_lib):
    P = wl.image_warping(2048, 1100, random_state=1, perturb=0.3, jitter_urshape=JIT)      # 2.25 M pixels: no general variant holds it
    g = hip_solver(P, "gaussNewtonGPU", nIterations=1, lIterations=4, amd_onchip=4)
    d = g.describe()
    assert d["general_urshape"].startswith("one launch per PCG iteration") and "no general-UrShape variant fits" in d["why_not_on_chip_general"], d
    g.close()
    _pair(oracle_lib, P, 1, 4, 1e-5, 2e-5, expect_onchip=False)


def test_describe_names_both_kernels_at_level_4_and_is_unchanged_below():
    P = wl.image_warping(300, 100, random_state=1, jitter_urshape=JIT)
    texts = {}
    for level in (1, 3, 4):
        g = hip_solver(P, "gaussNewtonGPU", nIterations=1, lIterations=4, amd_onchip=level)
        texts[level] = g.describe()
        g.close()
    assert texts[1]["path"].startswith("on-chip (if UrShape is the unit lattice") and "general_urshape" not in texts[1]
    assert texts[3]["path"] == texts[1]["path"] and "general_urshape" not in texts[3]
    assert "iw_onchipPcgGeneral" in texts[4]["path"] and texts[4]["general_urshape"].startswith("on-chip (iw_onchipPcgGeneral)"), texts[4]
