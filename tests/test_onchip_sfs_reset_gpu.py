"""GPU parity tests (-m gpu) of shape_from_shading's on-chip Levenberg-Marquardt linear solve WITH the split residual reset inside the solve (opt_amd/csrc/sfs_onchip.h:
sfs_onchipPcg<T, rows, 2, waves>, taken with the solver parameter amd_onchip = 3 when lIterations > residual_reset_period).

An iteration k with (k + 1) % residual_reset_period == 0 and k + 1 < lIterations ends with the reference's split step (solverGPUGaussNewton.t:1077-1086): delta += alpha p,
then r = b - (J^T J + CtC) delta from a second march over delta, z = r, beta and Q from a second grid-wide wait.  Side by side with the CPU oracle, step by step (the shape of
tests/test_onchip_reset_gpu.py, the 5-point stencils' file):
  * the solve really ran on chip (kernel name, on_chip_status 1), the return codes are the oracle's, and every outer step of the oracle ran more PCG iterations than the
    period -- no case passes without a reset;
  * bars: a floor from tests/test_onchip_sfs_gpu.py for the same input family -- double 1e-10 on the cost of the first step, 1e-8 on later steps, 1e-7 on the unknowns, 1e-8 on
    the radius; float 1e-5 / 1e-3 / - / 1e-3 -- widened, per step, to 10 x the error the launch-per-iteration loop (amd_onchip = 1, which must NOT be on chip) shows against the
    oracle on the same case, measured in the test: the project's margin between two legal summation orders of the same arithmetic (tools/make_parity_bars.py);
  * every offered (precision, rows, waves) variant, forced with OPT_AMD_ONCHIP_ROWS / _WAVES: SFS_MODE2_VARIANTS is compared with the compiler's resource remarks by
    tests/test_onchip_sfs_reset_resources.py, so no offered variant goes untested;
  * early-outs before any reset, on one, right behind one and between two, with the "breaking at iteration" message; the reference's input size; the time-out path; on chip
    against the marching kernels; and what amd_onchip = 3 does NOT change.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from opt_amd import api, workloads as wl
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

# every sfs_onchipPcg<T, rows, 2, waves> the library offers: (precision, rows a wave owns, waves per workgroup)
SFS_MODE2_VARIANTS = [(prec, r, w) for prec in ("double", "float") for r in (4, 6, 8, 10) for w in (4, 8)]
DOUBLE_FLOORS = dict(first=1e-10, later=1e-8, x=1e-7, radius=1e-8)
FLOAT_FLOORS = dict(first=1e-5, later=1e-3, x=None, radius=1e-3)
SHAPES = [(40, 32), (61, 9), (130, 37), (5, 70), (123, 4), (200, 150)]      # ((3, 3) of the model file is left out: its linear solves end after 2 iterations)
FLOAT_SHAPES = [(40, 32), (130, 37), (200, 150)]


def _sfs(W=130, H=90, double=True, seed=11):
    return wl.shape_from_shading(W, H, double=double, seed=seed, holes=True, noise=2e-3)


def _force(monkeypatch, rows, waves):
    monkeypatch.setenv("OPT_AMD_ONCHIP_ROWS", str(rows)); monkeypatch.setenv("OPT_AMD_ONCHIP_WAVES", str(waves))


def _log(P, kind, step, err):
    """(the yardstick runs: measured, not asserted -- same record as helpers.assert_close writes)"""
    log = os.environ.get("OPT_PARITY_LOG")
    if log:
        node = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        fn, _, par = node.partition("[")
        with open(log, "a") as f:
            f.write(json.dumps({"test": fn, "params": ("[" + par) if par else "", "prec": "double" if P.double else "float", "kind": kind, "step": step, "err": err, "default": None}) + "\n")


def _run(oracle_lib, P, nsteps, liters, period, onchip, **controls):
    """The oracle and the library step by step on the same input; returns what was measured."""
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=nsteps, lIterations=liters, residual_reset_period=period, **controls)
    o.set_threads(4)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=nsteps, lIterations=liters, residual_reset_period=period, amd_onchip=onchip, **controls)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    m = {"nsteps": nsteps, "ret": [], "cost": [], "radius": [], "costs": [(o.cost(), g.cost())], "describe": g.describe()}
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        m["ret"].append((a, b))
        m["costs"].append((o.cost(), g.cost()))
        m["cost"].append(abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-12 * scale, 1e-300))
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


def _against_parent_path(oracle_lib, make, nsteps, liters, period, status=1, min_iters=None, **controls):
    """Every case: the launch-per-iteration loop (amd_onchip = 1, which must NOT be on chip) against the oracle gives the yardstick, then the same case with amd_onchip = 3.
    Bar per step = max(floor, 10 x the yardstick's error at that step), likewise for the unknowns.  min_iters: what every outer step's iteration count must exceed (the
    period: every step passes a reset); None for the early-out cases, which pin the counts themselves."""
    P = make()
    fl = DOUBLE_FLOORS if P.double else FLOAT_FLOORS
    y = _run(oracle_lib, make(), nsteps, liters, period, 1, **controls)
    assert "PCGSolveOnChip" not in y["kernels"] and y["status"] == 0, (y["kernels"], y["status"])
    m = _run(oracle_lib, make(), nsteps, liters, period, 3, **controls)
    for i, e in enumerate(y["cost"]):
        _log(P, "cost_parent_path", i + 1, e); _log(P, "radius_parent_path", i + 1, y["radius"][i])
    _log(P, "x_parent_path", None, y["x"])
    print("parent path (cost per step, radius per step, x):", y["cost"], y["radius"], y["x"], "| on chip:", m["cost"], m["radius"], m["x"], "| iterations:", m["iters"])
    assert "PCGSolveOnChip" in m["kernels"] and m["status"] == status, (m["kernels"], m["status"])
    assert all(a == b for a, b in m["ret"]), (m["ret"], m["costs"])
    assert len(m["iters"]) == nsteps, (m["iters"], nsteps)      # every outer step ran
    if min_iters is not None:
        assert all(n > min_iters for n in m["iters"]), (m["iters"], min_iters)      # ... and passed a reset
    yerr = lambda errs, i: errs[i] if i < len(errs) else 0.0
    for i, e in enumerate(m["cost"]):
        floor = fl["first"] if i == 0 else fl["later"]
        assert_close("cost" if i == 0 else "cost_later", e, 0.0, max(floor, 10.0 * yerr(y["cost"], i)), absolute=True, double=P.double, step=i + 1)
        assert_close("radius", m["radius"][i], 0.0, max(fl["radius"], 10.0 * yerr(y["radius"], i)), absolute=True, double=P.double, step=i + 1)
    if fl["x"] is not None:
        assert_close("x", m["x"], 0.0, max(fl["x"], 10.0 * y["x"]), absolute=True, double=P.double)
    return m


# ---- 1. the controls: resets at every iteration, at odd periods, solves that end on a reset iteration (20, 10) and right behind one (21, 10), the long horizon (50, 10) -------
@pytest.mark.parametrize("liters,period", [(12, 5), (10, 3), (6, 1), (8, 7), (21, 10), (20, 10), (25, 10), (50, 10)])
def test_controls(oracle_lib, liters, period):
    _against_parent_path(oracle_lib, _sfs, 3, liters, period, min_iters=period)


# ---- 2. every variant -----------------------------------------------------------------------------------------------------------------------------------------------------
def _variants(prec):
    return [(r, w) for (p, r, w) in SFS_MODE2_VARIANTS if p == prec]


@pytest.mark.parametrize("rows,waves", _variants("double"))
@pytest.mark.parametrize("W,H", SHAPES)
def test_variants_double(oracle_lib, monkeypatch, W, H, rows, waves):
    _force(monkeypatch, rows, waves)
    m = _against_parent_path(oracle_lib, lambda: _sfs(W, H, True, W + 3 * H + rows), 3, 12, 5, min_iters=5)
    assert m["describe"]["onchip_rows_per_wave"] == str(rows) and m["describe"]["waves_per_workgroup"] == str(waves), m["describe"]


@pytest.mark.parametrize("rows,waves", _variants("float"))
@pytest.mark.parametrize("W,H", FLOAT_SHAPES)
def test_variants_float(oracle_lib, monkeypatch, W, H, rows, waves):
    """float: the reset's r = b - A delta cancels, so the kernel forms A delta in double from the float operands (sfs_onchip.h SPLIT); with a float A delta one of these inputs
    (130 x 37, seed 249) sits 5 % over its first-step bar in every variant -- figures in profiles/onchip_sfs_reset.md"""
    _force(monkeypatch, rows, waves)
    _against_parent_path(oracle_lib, lambda: _sfs(W, H, False, W + 3 * H + rows), 3, 12, 5, min_iters=5, q_tolerance=-1e9)


# ---- 3. early-outs around resets ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("liters,period,qtol,expect", [
    (25, 10, 0.1, [5, 11, 21, 25]),       # before any reset, right behind the reset at 10, right behind the one at 20, none
    (25, 10, 0.05, [10, 19, 25, 25]),     # on the reset iteration itself, between resets
    (25, 10, 0.2, [2, 7, 11, 16]),
    (12, 5, 0.05, [10, 12, 12, 12]),
])
def test_early_outs_around_resets(oracle_lib, capfd, liters, period, qtol, expect):
    """(expected iteration counts: the CPU oracle's; precedent for the message: tests/test_onchip_reset_gpu.py::test_breaking_message_names_the_oracles_iterations)"""
    m = _against_parent_path(oracle_lib, _sfs, 4, liters, period, q_tolerance=qtol)
    assert m["iters"] == expect, m["iters"]
    capfd.readouterr()
    P = _sfs()
    g = hip_solver(P, "LMGPU", verbosity=1, nIterations=4, lIterations=liters, residual_reset_period=period, q_tolerance=qtol, amd_onchip=3)
    dev = api.to_device(P)
    g.init(dev)
    while g.step(dev):
        pass
    assert g.on_chip_status() == 1
    g.close()
    ctypes.CDLL(None).fflush(None)      # the library prints through C stdio
    out = capfd.readouterr().out
    # (a solve that ran all its iterations prints nothing: the test behind the last iteration is dead, solver.hip does not reproduce its message for any on-chip kernel)
    assert [int(n) for n in re.findall(r"breaking at iteration: (\d+)", out)] == [n for n in expect if n < liters], out[-2000:]


# ---- 4. the reference's own input size (640 x 480, examples/shape_from_shading/src/main.cpp:27-38) -----------------------------------------------------------------------------
def test_reference_input_size_double(oracle_lib):
    m = _against_parent_path(oracle_lib, lambda: wl.shape_from_shading(640, 480, double=True, seed=1, holes=True), 2, 25, 10, min_iters=10)
    d = m["describe"]
    assert "on-chip" in d["path"] and "residual resets inside the solve" in d["path"], d
    # the variant that ran is the one the selection rule picks from the offered list (onchip_launch.h: among those whose workgroups fit one per CU, the fewest marching
    # trips per SIMD and iteration -- a second wave per SIMD counts 1.36), worked out here from the device's CU count, not from describe()
    import torch
    cus = min(torch.cuda.get_device_properties(0).multi_processor_count, 256)
    grid = lambda r, w: -(-(-(-640 // 60) * -(-480 // r)) // w)
    cost, rows, waves = min(((100 if w == 4 else 136) * (r + 4), r, w) for (p, r, w) in SFS_MODE2_VARIANTS if p == "double" and grid(r, w) <= cus)
    assert (d["onchip_rows_per_wave"], d["waves_per_workgroup"]) == (str(rows), str(waves)), (d, rows, waves)
    assert d["workgroups"].startswith(f"{grid(rows, waves)} of "), (d, rows, waves)


# ---- 5. the time-out path: the flag a timed-out wait raises, in iteration 0 and in iteration 7 (behind the first reset) --------------------------------------------------------
@pytest.mark.parametrize("fail_at", [0, 7])
def test_timeout_path_redoes_the_step_on_the_marching_kernels(oracle_lib, monkeypatch, fail_at):
    """(the orderly give-up flag of tests/test_onchip_sfs_gpu.py: nothing is written, the step is redone by sfs_pcgMarch, resets included)"""
    monkeypatch.setenv("OPT_AMD_ONCHIP_FAIL_AT", str(fail_at))
    m = _against_parent_path(oracle_lib, lambda: _sfs(130, 70, True, 3), 3, 12, 5, status=2, min_iters=5, q_tolerance=-1e9)
    assert "PCGIteration" in m["kernels"], m["kernels"]


# ---- 6. on chip against the marching kernels ----------------------------------------------------------------------------------------------------------------------------------
def test_onchip_against_marching_kernels():
    """One LM step of 25 iterations (resets at 10 and 20) under amd_onchip = 3 and 1 on the controls' input: the costs agree to 1e-12, the bar
    tests/test_onchip_sfs_gpu.py::test_onchip_against_marching_kernels holds without resets (the distance is printed)."""
    res = {}
    for onchip in (3, 1):
        P = _sfs()
        g = hip_solver(P, "LMGPU", timing=True, nIterations=2, lIterations=25, residual_reset_period=10, amd_onchip=onchip)
        dev = api.to_device(P)
        g.init(dev); g.step(dev)
        assert ("PCGSolveOnChip" in g.kernel_timings()) == (onchip == 3) and g.on_chip_status() == (1 if onchip == 3 else 0)
        res[onchip] = g.cost()
        g.close()
    dist = abs(res[3] - res[1]) / abs(res[1])
    print("on chip vs marching kernels:", dist)
    assert dist <= 1e-12, (res, dist)


# ---- 7. what amd_onchip = 3 does and does not change --------------------------------------------------------------------------------------------------------------------------
def test_three_implies_two_for_the_stencil_family(oracle_lib):
    P = wl.poisson_image_editing(120, 70, double=True, seed=9)
    m = _run(oracle_lib, P, 3, 12, 5, 3)
    assert "PCGSolveOnChip" in m["kernels"] and m["status"] == 1, (m["kernels"], m["status"])
    assert all(a == b for a, b in m["ret"]) and all(n > 5 for n in m["iters"]), (m["ret"], m["iters"])
    assert m["cost"][0] <= 1e-10, m["cost"]


@pytest.mark.parametrize("onchip", [1, 2])
def test_lower_settings_keep_the_marching_kernels(oracle_lib, onchip):
    m = _run(oracle_lib, _sfs(), 3, 12, 5, onchip)
    assert "PCGSolveOnChip" not in m["kernels"] and m["status"] == 0, (m["kernels"], m["status"])
    assert all(a == b for a, b in m["ret"]), m["ret"]


def test_no_reset_inside_the_solve_takes_the_same_kernel_as_the_default():
    """lIterations <= residual_reset_period: amd_onchip = 3 and 1 run the same mode-1 kernel -- the same bits"""
    res = {}
    for onchip in (3, 1):
        P = _sfs()
        g = hip_solver(P, "LMGPU", timing=True, nIterations=3, lIterations=10, residual_reset_period=10, amd_onchip=onchip)
        dev = api.to_device(P)
        g.init(dev)
        c = [g.cost()]
        while g.step(dev):
            c.append(g.cost())
        c.append(g.cost())
        assert "PCGSolveOnChip" in g.kernel_timings() and g.on_chip_status() == 1
        assert "no residual reset inside the solve" in g.describe()["path"]
        res[onchip] = c
        g.close()
    assert res[3] == res[1], res


def test_describe_matches_the_step():
    P = _sfs()
    g = hip_solver(P, "LMGPU", nIterations=3, lIterations=12, residual_reset_period=5, amd_onchip=3)
    d = g.describe()
    g.close()
    assert "on-chip" in d["path"] and "residual resets inside the solve" in d["path"] and d["amd_onchip"] == "3", d
    for onchip in (1, 2):
        g = hip_solver(P, "LMGPU", nIterations=3, lIterations=12, residual_reset_period=5, amd_onchip=onchip)
        d = g.describe()
        g.close()
        assert "on-chip" not in d["path"] and "reset" in d["why_not_on_chip"] and "amd_onchip=3" in d["why_not_on_chip"], d
