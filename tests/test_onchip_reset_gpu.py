"""GPU parity tests (-m gpu) of the on-chip Levenberg-Marquardt linear solve WITH the split residual reset inside the solve (opt_amd/csrc/stencil_onchip.h:
march_onchipPcg<.., 2>, taken with the solver parameter amd_onchip = 2 when lIterations > residual_reset_period) on the 5-point-stencil energies:
poisson_image_editing, the tests/minimal laplacian, optical_flow, intrinsic_image_decomposition.

An iteration k with (k + 1) % residual_reset_period == 0 and k + 1 < lIterations ends with the reference's split step (solverGPUGaussNewton.t:1077-1086): delta += alpha p,
then r = b - (J^T J + CtC) delta from a second stencil pass, z = r, beta and Q from a second grid-wide wait.  Side by side with the CPU oracle, step by step:
  * the solve really ran on chip (kernel name, on_chip_status) and every outer step of the oracle ran more PCG iterations than the period -- no case passes without a reset;
  * the same accept / reject decisions, cost, trust-region radius and unknowns within the bars the on-chip LM tests of tests/test_onchip_stencil_gpu.py carry for the
    same inputs: double 1e-10 (cost) / 1e-9 (unknowns) / 1e-8 (radius); float 1e-5 at the first step, 1e-3 later and on the radius;
  * where no LM on-chip bar exists (intrinsic_image_decomposition, the long horizons of the reference's own callers: 50 and 100 linear iterations) the yardstick is measured
    in the test: the same case with amd_onchip = 1 -- the launch-per-iteration loop -- against the oracle, bar = max(contract, 10 x that error), the project's margin between
    two legal summation orders of the same arithmetic (tools/make_parity_bars.py);
  * every offered (operator, precision, rows, waves) variant, forced with OPT_AMD_ONCHIP_ROWS / _WAVES: MODE2_VARIANTS is compared with the compiler's resource remarks by
    tests/test_onchip_reset_resources.py, so no offered variant goes untested;
  * early-outs between resets, right behind one and on one, the "breaking at iteration" message, the time-out path, and what amd_onchip = 2 does NOT change.
"""
import json
import os
import re

import numpy as np
import pytest

from opt_amd import api, workloads as wl
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

# every march_onchipPcg<T, Op, rows, waves, 2> the library offers: (operator, precision, rows a wave owns, waves per workgroup)
MODE2_VARIANTS = (
    [("poisson", "double", r, w) for (r, w) in [(2, 4), (4, 4), (8, 4), (2, 8)]]
    + [("poisson", "float", r, w) for (r, w) in [(2, 4), (4, 4), (8, 4), (2, 8), (4, 8)]]
    + [("laplacian", "float", r, w) for r in (2, 4, 8, 16) for w in (4, 8)]
    + [("optical_flow", "double", r, w) for (r, w) in [(2, 4), (4, 4), (8, 4), (2, 8), (4, 8)]]
    + [("optical_flow", "float", r, w) for (r, w) in [(2, 4), (4, 4), (8, 4), (16, 4), (2, 8), (4, 8), (8, 8)]]
    + [("intrinsic", "double", r, w) for (r, w) in [(2, 4), (4, 4)]]
    + [("intrinsic", "float", r, w) for (r, w) in [(2, 4), (4, 4), (8, 4), (2, 8), (4, 8)]]
)
SHAPES = [(61, 5), (62, 3), (63, 9), (300, 40), (64, 300), (517, 33)]
FLOAT_SHAPES = [(61, 5), (300, 40), (64, 300), (517, 33)]
DOUBLE_BARS = (1e-10, 1e-9, 1e-8)      # cost, unknowns, radius


def _variants(op, prec):
    return [(r, w) for (o, p, r, w) in MODE2_VARIANTS if o == op and p == prec]


def _poisson(W, H, double, seed, mask):
    P = wl.poisson_image_editing(W, H, double=double, seed=seed)
    rng = np.random.default_rng(seed + 100)
    M = P.params[2]
    if mask == "random":
        M[...] = np.where(rng.random(M.shape) < 0.3, 255.0, 0.0)
    elif mask == "none":
        M[...] = 0.0
    return P


def _force(monkeypatch, rows, waves):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows)); monkeypatch.setenv("OPT_AMD_ONCHIP_WAVES", str(waves))


def _log(kind, step, err):
    """(the yardstick runs: measured, not asserted -- same record as helpers.assert_close writes)"""
    log = os.environ.get("OPT_PARITY_LOG")
    if log:
        node = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        fn, _, par = node.partition("[")
        with open(log, "a") as f:
            f.write(json.dumps({"test": fn, "params": ("[" + par) if par else "", "prec": "double", "kind": kind, "step": step, "err": err, "default": None}) + "\n")


def _run(oracle_lib, P, nsteps, liters, period, onchip, **controls):
    """The oracle and the library step by step on the same input (the shape of tests/test_onchip_stencil_gpu.py::_lm_side_by_side); returns what was measured."""
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=nsteps, lIterations=liters, residual_reset_period=period, **controls)
    o.set_threads(4)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=nsteps, lIterations=liters, residual_reset_period=period, amd_onchip=onchip, **controls)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    m = {"nsteps": nsteps, "ret": [], "cost": [], "radius": [], "costs": [(o.cost(), g.cost())]}
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        m["ret"].append((a, b))
        m["costs"].append((o.cost(), g.cost()))
        m["cost"].append(abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-9 * scale, 1e-300))
        m["radius"].append(abs(g.trust_region_radius() - o.trust_region_radius()) / max(abs(o.trust_region_radius()), 1e-300))
        if not a or not b:
            break
    m["kernels"] = set(g.kernel_timings().keys())
    m["status"] = g.on_chip_status()
    m["x"] = rel_err(device_unknowns(P, dev), flat_unknowns(Pref))
    tr = o.trace()
    m["iters"] = [int(c) for c in np.bincount(tr[:, 0].astype(int))] if len(tr) else []
    g.close(); o.close()
    return m


def _check(m, P, period, cost_tol, x_tol, radius_tol, later_tol=None, status=1):
    """cost_tol / radius_tol: one bar, or one per step.  later_tol (float): the bar of the cost from the second step on; the radius is then compared at the first step only."""
    assert "PCGSolveOnChip" in m["kernels"] and m["status"] == status, (m["kernels"], m["status"])
    assert all(a == b for a, b in m["ret"]), (m["ret"], m["costs"])
    assert len(m["iters"]) == m["nsteps"] and all(n > period for n in m["iters"]), (m["iters"], period)      # every outer step ran, and passed a reset
    per = lambda t, i: t[i] if isinstance(t, (list, tuple)) else t
    for i, e in enumerate(m["cost"]):
        tol = per(cost_tol, i) if (later_tol is None or i == 0) else later_tol
        assert_close("cost" if i == 0 else "cost_later", e, 0.0, tol, absolute=True, double=P.double, step=i + 1)
        if later_tol is None or i == 0:
            assert_close("radius", m["radius"][i], 0.0, per(radius_tol, i), absolute=True, double=P.double, step=i + 1)
    if x_tol is not None:
        assert_close("x", m["x"], 0.0, x_tol, absolute=True, double=P.double)


def _against_parent_path(oracle_lib, make, nsteps, liters, period, contract, **controls):
    """Bars measured in the test: the same case on the launch-per-iteration loop (amd_onchip = 1, which must NOT be on chip) against the oracle; bar = max(contract,
    10 x that error) per step for cost and radius, and for the unknowns."""
    y = _run(oracle_lib, make(), nsteps, liters, period, 1, **controls)
    assert "PCGSolveOnChip" not in y["kernels"], y["kernels"]
    m = _run(oracle_lib, make(), nsteps, liters, period, 2, **controls)
    for i, e in enumerate(y["cost"]):
        _log("cost_parent_path", i + 1, e); _log("radius_parent_path", i + 1, y["radius"][i])
    _log("x_parent_path", None, y["x"])
    print("parent path (cost per step, radius per step, x):", y["cost"], y["radius"], y["x"], "| on chip:", m["cost"], m["radius"], m["x"])
    n = len(m["cost"])
    bar = lambda errs, c: [max(c, 10.0 * (errs[i] if i < len(errs) else 0.0)) for i in range(n)]
    _check(m, make(), period, bar(y["cost"], contract[0]), max(contract[1], 10.0 * y["x"]), bar(y["radius"], contract[2]))


# ---- 1. the controls: resets at every iteration, at odd periods, an early-out between resets (25, 10), right behind one (12, 5), a solve that ends on one (20, 10) ----------
@pytest.mark.parametrize("liters,period", [(12, 5), (10, 3), (6, 1), (8, 7), (21, 10), (20, 10), (25, 10)])
@pytest.mark.parametrize("energy", ["poisson", "optical_flow"])
def test_controls(oracle_lib, energy, liters, period):
    P = _poisson(120, 70, True, 9, "random") if energy == "poisson" else wl.optical_flow(120, 70, double=True, seed=9, init_flow=1.2)
    _check(_run(oracle_lib, P, 3, liters, period, 2), P, period, *DOUBLE_BARS)


# ---- 2. every variant ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,waves", _variants("poisson", "double"))
@pytest.mark.parametrize("mask", ["random", "none"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_poisson_double(oracle_lib, monkeypatch, W, H, mask, rows, waves):
    _force(monkeypatch, rows, waves)
    P = _poisson(W, H, True, W * 3 + H, mask)
    _check(_run(oracle_lib, P, 3, 12, 5, 2), P, 5, *DOUBLE_BARS)


@pytest.mark.parametrize("rows,waves", _variants("optical_flow", "double"))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_optical_flow_double(oracle_lib, monkeypatch, W, H, rows, waves):
    _force(monkeypatch, rows, waves)
    P = wl.optical_flow(W, H, double=True, seed=W + H, init_flow=1.2)
    _check(_run(oracle_lib, P, 3, 12, 5, 2), P, 5, *DOUBLE_BARS)


@pytest.mark.parametrize("rows,waves", _variants("poisson", "float"))
@pytest.mark.parametrize("W,H", FLOAT_SHAPES)
def test_variants_poisson_float(oracle_lib, monkeypatch, W, H, rows, waves):
    _force(monkeypatch, rows, waves)
    P = _poisson(W, H, False, W * 5 + H, "random")
    _check(_run(oracle_lib, P, 2, 12, 5, 2, q_tolerance=-1e9), P, 5, 1e-5, None, 1e-3, later_tol=1e-3)


@pytest.mark.parametrize("rows,waves", _variants("laplacian", "float"))
@pytest.mark.parametrize("W,H", FLOAT_SHAPES)
def test_variants_laplacian_float(oracle_lib, monkeypatch, W, H, rows, waves):
    _force(monkeypatch, rows, waves)
    P = wl.laplacian(W, H, seed=W + H)
    _check(_run(oracle_lib, P, 2, 12, 5, 2, q_tolerance=-1e9), P, 5, 1e-5, None, 1e-3, later_tol=1e-3)


@pytest.mark.parametrize("rows,waves", _variants("optical_flow", "float"))
@pytest.mark.parametrize("W,H", FLOAT_SHAPES)
def test_variants_optical_flow_float(oracle_lib, monkeypatch, W, H, rows, waves):
    """(the float bars of the poisson and laplacian LM on-chip tests: the float contract at the first step, 1e-3 later and on the radius)"""
    _force(monkeypatch, rows, waves)
    P = wl.optical_flow(W, H, double=False, seed=W + H, init_flow=1.2)
    _check(_run(oracle_lib, P, 2, 12, 5, 2, q_tolerance=-1e9), P, 5, 1e-5, None, 1e-3, later_tol=1e-3)


@pytest.mark.parametrize("rows,waves", _variants("intrinsic", "float"))
def test_variants_intrinsic_float_against_the_generic_kernels(monkeypatch, rows, waves):
    """float: the trajectory of this energy is outside the 1e-5 contract for any two implementations (tests/golden/float_envelopes.json).  As
    tests/test_onchip_stencil_gpu.py::test_intrinsic_float_variants_against_the_marching_kernels does for Gauss-Newton, the variants are pinned against the other legal
    implementation on the same input -- the launch-per-iteration loop (amd_onchip = 1) -- after one LM step of 12 iterations with resets at 5 and 10, with that test's bars."""
    _force(monkeypatch, rows, waves)
    res = {}
    for onchip in (2, 1):
        P = wl.intrinsic_image_decomposition(200, 120, double=False, seed=4)
        g = hip_solver(P, "LMGPU", timing=True, nIterations=1, lIterations=12, residual_reset_period=5, q_tolerance=-1e9, amd_onchip=onchip)
        dev = api.to_device(P)
        g.init(dev); g.step(dev)
        assert ("PCGSolveOnChip" in g.kernel_timings()) == (onchip == 2) and g.on_chip_status() == (1 if onchip == 2 else 0)
        res[onchip] = (g.cost(), device_unknowns(P, dev))
        g.close()
    assert abs(res[2][0] - res[1][0]) <= 2e-4 * abs(res[1][0]), (res[2][0], res[1][0])
    assert rel_err(res[2][1], res[1][1]) < 1e-4


# ---- 3. intrinsic_image_decomposition, double: ill-conditioned, no LM on-chip bar of its own -- measured against the launch-per-iteration loop's own error ------------------
@pytest.mark.parametrize("rows,waves", _variants("intrinsic", "double"))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_intrinsic_double(oracle_lib, monkeypatch, W, H, rows, waves):
    """bar = max(1e-10, 10 x the error of the same case on the launch-per-iteration loop) for the cost, likewise from 1e-9 for the unknowns and from 1e-8 for the radius
    (the double contract of the other energies, widened only by what the parent's path itself needs on this ill-conditioned system)"""
    _force(monkeypatch, rows, waves)
    _against_parent_path(oracle_lib, lambda: wl.intrinsic_image_decomposition(W, H, double=True, seed=W + H), 3, 12, 5, DOUBLE_BARS)


# ---- 4. the horizons of the reference's own callers (poisson_image_editing: 100 linear iterations, optical_flow: 50) ------------------------------------------------------
@pytest.mark.parametrize("case", ["optical_flow-50", "optical_flow-100", "poisson-100", "intrinsic-50"])
def test_example_horizons(oracle_lib, case):
    """bar per step = max(double contract, 10 x the launch-per-iteration loop's own error against the oracle on the same case)"""
    make, liters = {"optical_flow-50": (lambda: wl.optical_flow(300, 90, double=True, seed=7, init_flow=1.2), 50),
                    "optical_flow-100": (lambda: wl.optical_flow(300, 90, double=True, seed=7, init_flow=1.2), 100),
                    "poisson-100": (lambda: _poisson(300, 90, True, 5, "random"), 100),
                    "intrinsic-50": (lambda: wl.intrinsic_image_decomposition(200, 60, double=True, seed=5), 50)}[case]
    _against_parent_path(oracle_lib, make, 3, liters, 10, DOUBLE_BARS)


# ---- 5. the early-out message of a verbose caller ---------------------------------------------------------------------------------------------------------------------------
def test_breaking_message_names_the_oracles_iterations(oracle_lib, capfd):
    """(precedent: tests/test_lm_controls_gpu.py::test_verbose_run_takes_the_same_path_as_the_silent_one)  poisson 120 x 70, 25 iterations, period 10: the oracle's linear
    solves end after 11, 17 and 17 iterations -- one early-out right behind the reset at 10, two between the resets."""
    P = _poisson(120, 70, True, 9, "random")
    m = _run(oracle_lib, P, 3, 25, 10, 2)
    _check(m, P, 10, *DOUBLE_BARS)
    assert m["iters"] == [11, 17, 17], m["iters"]
    capfd.readouterr()
    g = hip_solver(P, "LMGPU", verbosity=1, nIterations=3, lIterations=25, residual_reset_period=10, amd_onchip=2)
    dev = api.to_device(P)
    g.init(dev)
    while g.step(dev):
        pass
    assert g.on_chip_status() == 1
    g.close()
    import ctypes
    ctypes.CDLL(None).fflush(None)      # the library prints through C stdio
    out = capfd.readouterr().out
    assert [int(n) for n in re.findall(r"breaking at iteration: (\d+)", out)] == [11, 17, 17], out[-2000:]


# ---- 6. the time-out path: the flag a timed-out wait raises, in iteration 0 and in iteration 7 (behind the first reset) ------------------------------------------------------
@pytest.mark.parametrize("fail_at", [0, 7])
def test_timeout_path_redoes_the_step_on_the_generic_kernels(oracle_lib, monkeypatch, fail_at):
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", str(fail_at))
    P = _poisson(130, 70, True, 3, "random")
    m = _run(oracle_lib, P, 3, 12, 5, 2, q_tolerance=-1e9)
    _check(m, P, 5, *DOUBLE_BARS, status=2)
    assert "PCGStep2_2ndHalf" in m["kernels"], m["kernels"]      # the step was redone by the launch-per-iteration loop, resets included


# ---- 7. what amd_onchip = 2 does not change ---------------------------------------------------------------------------------------------------------------------------------
def test_default_keeps_a_reset_inside_the_solve_on_the_generic_kernels(oracle_lib):
    m = _run(oracle_lib, _poisson(120, 70, True, 9, "random"), 3, 12, 5, 1)
    assert "PCGSolveOnChip" not in m["kernels"] and m["status"] == 0, (m["kernels"], m["status"])


def test_shape_from_shading_keeps_its_rule(oracle_lib):
    m = _run(oracle_lib, wl.shape_from_shading(72, 56, double=True, seed=2), 3, 12, 5, 2)
    assert "PCGSolveOnChip" not in m["kernels"] and m["status"] == 0, (m["kernels"], m["status"])
    assert all(a == b for a, b in m["ret"]), m["ret"]


def test_describe_matches_the_step():
    P = _poisson(120, 70, True, 9, "random")
    g = hip_solver(P, "LMGPU", nIterations=3, lIterations=12, residual_reset_period=5, amd_onchip=2)
    d = g.describe()
    g.close()
    assert "on-chip" in d["path"] and d["amd_onchip"] == "2", d
    g = hip_solver(P, "LMGPU", nIterations=3, lIterations=12, residual_reset_period=5)
    d = g.describe()
    g.close()
    assert "on-chip" not in d["path"] and "reset" in d["why_not_on_chip"] and "amd_onchip=2" in d["why_not_on_chip"], d
