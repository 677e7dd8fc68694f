"""GPU parity tests (-m gpu) of shape_from_shading's row-marching kernels at many rows per workgroup (opt_amd/csrc/energy_sfs.hip: sfs_pcgMarch<T, LM>, the launch-per-
iteration PCG kernel; sfs_pcgMarch<T, false, true>, PCGInit1 with LM's PCGFinalizeDiagonal; sfs_costMarch<T, MODEL>; sfs_applyTiled<T, LM>).

These are the kernels a plan runs when the on-chip solve times out, is refused, is traced or does not fit, and PCGInit1 and the cost marches run on every path.  Their grid
is sized to the co-resident workgroup count, so every small image elsewhere in the suite gives a workgroup ONE row; here OPT_AMD_SFS_MARCH_GRID (read when the plan is
made) forces the regimes of tests/sfs_march_cases.py -- one workgroup marching the whole image, odd and even rows per group, last groups of one and two rows, several row
groups per XCD range with and without idle tails, a second and third column strip -- and tests/test_sfs_march_cases_cpu.py proves each case is in its regime.
  (a) probes: J^T F and diag(J^T J) (the JTF march: no sums) are bit-identical under the forced and the natural grid and match the oracle; the cost (sums in another order)
      matches both;
  (b) Gauss-Newton (lIterations 1 / 2 / 3 / 9 / 10) and Levenberg-Marquardt (residual resets every 5th iteration, the default period, a radius of 1e12, the q early-out)
      beside the oracle, double.  The only rejected step of these runs is the third of 7 x 400 (every LM run but the early-out one; proved by the CPU file): the steps of the
      1e12 run are accepted on these images;
  (c) the same in float on four rows of the table;
  (d) every case of (b) and (c) also on the natural grid, same plan parameters, no override: a forced case that misses a bar its twin holds is a kernel error;
  (e) OPT_AMD_SFS_ONEKERNEL=0, the three-kernel control, against the oracle; the timer table shows which loop ran (with the switch at 1 an LM solve still shows PCGStep1
      launches: the computeAdelta of its residual resets, two per outer step at period 5 -- never one per iteration);
  (f) sfs_applyTiled's tile loop: 1050 x 500 has more tiles (2079) than the tiled grid can have workgroups, so some workgroups take a second tile with the prefetch.
The 227 sub-cases (28 probes, 100 + 72 trajectories, 16 float, 8 three-kernel, 3 tile loop) take tens of milliseconds each and are grouped into 13 tests -- the probes, one
test per image, one per section: every sub-case of a test runs and every miss is reported under its own label (_every).
Bars: double cost 1e-10 on the first outer step and 1e-8 after it, radius 1e-8, unknowns 1e-7 (tests/test_onchip_sfs_gpu.py, test_lm_controls_gpu.py::
test_sfs_double_controls); float 1e-5 / 1e-3; probes 1e-11 / 3e-5, costs 1e-12 / 1e-5 (test_energies_gpu.py::test_cost_jtf_diag_jtjp).
"""
import numpy as np
import pytest

import sfs_march_cases as sc
from opt_amd import api
from helpers import assert_close, active_mask, device_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _marching_kernels_under_test(monkeypatch):
    """Images of these sizes would otherwise take the on-chip linear solve (sfs_onchip.h, tests/test_onchip_sfs_gpu.py)."""
    monkeypatch.setenv("OPT_AMD_ONCHIP", "0")
    monkeypatch.delenv("OPT_AMD_SFS_MARCH_GRID", raising=False)
    monkeypatch.delenv("OPT_AMD_SFS_ONEKERNEL", raising=False)


def _solver(monkeypatch, P, g, kind="gaussNewtonGPU", **params):
    """A plan whose marching launches have `g` workgroups as their target (None: the natural grid).  The switch is read when the plan is made: set before."""
    if g is None:
        monkeypatch.delenv("OPT_AMD_SFS_MARCH_GRID", raising=False)
    else:
        monkeypatch.setenv("OPT_AMD_SFS_MARCH_GRID", str(g))
    return hip_solver(P, kind, timing=True, **params)


def _beside(oracle_lib, monkeypatch, W, H, g, double, kind, nsteps, liters, first_tol, later_tol, radius_tol, x_tol, **controls):
    """Step the plan beside the oracle's run of the same image (sc.oracle_run: computed once per image and parameter set): equal return values, the cost after every step,
    the trust-region radius for LM, the unknowns at the end."""
    ref = sc.oracle_run(oracle_lib, W, H, double, kind, nsteps, liters, **controls)
    P = sc.problem(W, H, double)
    s = _solver(monkeypatch, P, g, kind, nIterations=nsteps, lIterations=liters, **controls)
    dev = api.to_device(P)
    s.init(dev)
    scale = max(abs(ref.cost0), 1e-300)
    assert_close("cost0", s.cost(), ref.cost0, 1e-12 if double else 1e-5, floor=scale, double=double)
    for i, ret in enumerate(ref.ret):
        got = s.step(dev)
        print(f"step {i + 1}: returned {got} ({ret}), cost {s.cost()!r} ({ref.cost[i]!r}, {abs(s.cost() - ref.cost[i]) / max(abs(ref.cost[i]), 1e-12 * scale):.2e}), "
              f"radius {s.trust_region_radius()!r} ({ref.radius[i]!r})")
        assert got == ret, (i, got, ret)
        assert_close("cost" if i == 0 else "cost_later", s.cost(), ref.cost[i], first_tol if i == 0 else later_tol, floor=1e-12 * scale, double=double, step=i + 1)
        if radius_tol is not None:
            assert_close("radius", s.trust_region_radius(), ref.radius[i], radius_tol, double=double, step=i + 1)
    kt = s.kernel_timings()
    print({k: v[0] for k, v in kt.items()})
    assert s.on_chip_status() == 0 and "PCGSolveOnChip" not in kt, kt.keys()
    if x_tol is not None:
        act = active_mask(P)      # (the excluded pixels keep their -10000: left in, they would take four digits off the relative error)
        xerr = rel_err(device_unknowns(P, dev)[act], ref.x[act])
        print(f"unknowns {xerr:.2e}")
        assert_close("x", xerr, 0.0, x_tol, absolute=True, double=double)
    s.close()
    return kt


def _every(subcases, fn):
    """fn(*args), or args[0](*args[1:]) where fn is None, for every (label, args) of a test's sub-cases: all of them run, and every one that misses is reported, not only the first.  (The sub-cases of one image
    or one kind share a test, tens of milliseconds each: the suite's case count grows by 13 instead of 227.  Only a failed assertion is collected; any other error ends
    the test.)"""
    failed = []
    for label, args in subcases:
        print(f"---- {label}")
        try:
            fn(*args) if fn else args[0](*args[1:])
        except AssertionError as e:
            failed.append(f"{label}: {e}")
    assert not failed, f"{len(failed)} of {len(subcases)} sub-cases:\n" + "\n".join(failed)


def _grid_label(W, H, g):
    return f"{W}x{H}-" + ("natural" if g is None else f"g{g}")


def _grids_of(W, H, cases):
    """The forced grids that `cases` has for an image, then the natural grid: their twin.  Nothing if the image is in none of them."""
    forced = [c.g for c in cases if (c.W, c.H) == (W, H)]
    return forced + [None] if forced else []


# ---- (a) probes that must not depend on the grid ---------------------------------------------------------------------------------------------------------------------
def _probes(oracle_lib, monkeypatch, c, double):
    P = sc.problem(c.W, c.H, double)
    act = active_mask(P)
    o = oracle_solver(oracle_lib, P)
    c_ref = o.eval_cost(P.params)
    f_ref, d_ref = o.eval_jtf(P.params)
    o.close()
    out = {}
    for g in (None, c.g):
        s = _solver(monkeypatch, P, g)
        dev = api.to_device(P)
        cost = s.eval_cost(dev)
        f, d = s.eval_jtf(dev)
        out[g] = (cost, f.cpu().numpy(), d.cpu().numpy())
        s.close()
    tol, ctol = (1e-11, 1e-12) if double else (3e-5, 1e-5)
    for g, (cost, f, d) in out.items():
        print(f"grid {g}: cost {abs(cost - c_ref) / abs(c_ref):.2e}, J^T F {rel_err(f[act], f_ref[act]):.2e}, diag {rel_err(d[act], d_ref[act]):.2e}")
    assert np.array_equal(out[c.g][1], out[None][1]) and np.array_equal(out[c.g][2], out[None][2])      # per element the same expressions, whichever workgroup owns the row
    assert_close("cost0", out[c.g][0], out[None][0], ctol, double=double)                                   # the sums are added in another order
    for g, (cost, f, d) in out.items():
        assert_close("cost0", cost, c_ref, ctol, double=double)
        assert_close("jtf", rel_err(f[act], f_ref[act]), 0.0, tol, absolute=True, double=double)
        assert_close("diag", rel_err(d[act], d_ref[act]), 0.0, tol, absolute=True, double=double)


def test_probes_do_not_depend_on_the_grid(oracle_lib, monkeypatch):
    """Every row of the table, double and float."""
    _every([(f"{sc.case_id(c)}-{'f64' if double else 'f32'}", (oracle_lib, monkeypatch, c, double)) for c in sc.TABLE for double in (True, False)], _probes)


# ---- (b) + (d) Gauss-Newton and Levenberg-Marquardt beside the oracle, double: forced grids and their natural-grid twins ------------------------------------------------
def _gauss_newton(oracle_lib, monkeypatch, W, H, g, liters):
    # 5 x 70: Gauss-Newton on an image a few pixels thin is an undamped, ill-conditioned normal matrix; the first step gets the 1e-8 tests/test_onchip_sfs_gpu.py gives it
    kt = _beside(oracle_lib, monkeypatch, W, H, g, True, "gaussNewtonGPU", 2, liters, 1e-8 if (W, H) == (5, 70) else 1e-10, 1e-8, None, 1e-7)
    assert kt["PCGIteration"][0] == 2 * liters and "PCGStep1" not in kt, kt


def _levenberg_marquardt(oracle_lib, monkeypatch, W, H, g, run):
    nsteps, liters, controls = sc.LM_RUNS[run]
    kt = _beside(oracle_lib, monkeypatch, W, H, g, True, "LMGPU", nsteps, liters, 1e-10, 1e-8, 1e-8, 1e-7, **controls)
    assert "PCGIteration" in kt and "PCGInit1" in kt and "PCGFinalizeDiagonal" not in kt, kt      # PCGInit1 is the march that also finalises the diagonal
    if run == "early_out":
        assert kt["PCGIteration"][0] < nsteps * liters, kt
    else:      # PCGStep1 is the computeAdelta of the residual resets (sfs_applyTiled<T, true>): after iterations 5 and 10 of a linear solve, or after the 10th
        assert kt["PCGIteration"][0] == nsteps * liters and kt["PCGStep1"][0] == nsteps * (liters // controls.get("residual_reset_period", 10)), kt


@pytest.mark.parametrize("W,H", sc.shapes(sc.TRAJECTORY))
def test_trajectories_double(oracle_lib, monkeypatch, W, H):
    """One image of the table: each of its forced grids and the natural grid, Gauss-Newton at every lIterations of the list and the four LM runs."""
    gn = [(f"{_grid_label(W, H, g)}-GN-{liters}", (_gauss_newton, oracle_lib, monkeypatch, W, H, g, liters)) for g in _grids_of(W, H, [c for c in sc.TRAJECTORY if c.gn]) for liters in sc.GN_LITERS]
    lm = [(f"{_grid_label(W, H, g)}-LM-{run}", (_levenberg_marquardt, oracle_lib, monkeypatch, W, H, g, run)) for g in _grids_of(W, H, [c for c in sc.TRAJECTORY if c.lm]) for run in sc.LM_RUNS]
    assert len(gn) >= 2 * len(sc.GN_LITERS) and len(lm) == (0 if (W, H) == (5, 70) else len(gn) // len(sc.GN_LITERS) * len(sc.LM_RUNS))
    _every(gn + lm, None)


# ---- (c) + (d) float ----------------------------------------------------------------------------------------------------------------------------------------------------
def _float(oracle_lib, monkeypatch, W, H, g, kind):
    lm = kind == "LMGPU"      # q_tolerance: a float Q near the threshold can end a linear solve one iteration apart (tests/test_onchip_sfs_gpu.py::test_variants_float)
    _beside(oracle_lib, monkeypatch, W, H, g, False, kind, 2, 10, 1e-5, 1e-3, 1e-3 if lm else None, None, **({"q_tolerance": -1e9} if lm else {}))


def test_float(oracle_lib, monkeypatch):
    rows = [sc.case(*r) for r in sc.FLOAT_ROWS]
    grids = [(c.W, c.H, c.g) for c in rows] + [(W, H, None) for W, H in sc.shapes(rows)]
    _every([(f"{_grid_label(W, H, g)}-{kind}", (oracle_lib, monkeypatch, W, H, g, kind)) for W, H, g in grids for kind in ("gaussNewtonGPU", "LMGPU")], _float)


# ---- (e) the three-kernel control ---------------------------------------------------------------------------------------------------------------------------------------
def _three_kernel(oracle_lib, monkeypatch, W, H, kind, one_kernel):
    monkeypatch.setenv("OPT_AMD_SFS_ONEKERNEL", one_kernel)
    lm = kind == "LMGPU"
    nsteps, liters, controls = (3, 12, {"residual_reset_period": 5}) if lm else (2, 10, {})
    kt = _beside(oracle_lib, monkeypatch, W, H, None, True, kind, nsteps, liters, 1e-10, 1e-8, 1e-8 if lm else None, 1e-7, **controls)
    if one_kernel == "0":
        assert "PCGStep1" in kt and "PCGIteration" not in kt and kt["PCGStep1"][0] >= nsteps * liters, kt
    else:      # (LM: what is left of PCGStep1 is the computeAdelta of the resets after iterations 5 and 10 of a step)
        assert "PCGIteration" in kt and kt.get("PCGStep1", (0, 0.0))[0] <= (2 * nsteps if lm else 0), kt


def test_three_kernel_control(oracle_lib, monkeypatch):
    _every([(f"{W}x{H}-{kind}-onekernel{k}", (oracle_lib, monkeypatch, W, H, kind, k)) for W, H in sc.THREE_KERNEL_SHAPES for kind in ("gaussNewtonGPU", "LMGPU") for k in ("0", "1")],
           _three_kernel)


# ---- (f) sfs_applyTiled's tile loop ---------------------------------------------------------------------------------------------------------------------------------------
def _tile_loop_apply_jtj(oracle_lib, monkeypatch, double):
    import torch
    W, H = sc.TILE_LOOP_SHAPE
    P = sc.problem(W, H, double)
    o = oracle_solver(oracle_lib, P)
    o.set_threads(4)
    v = (np.random.default_rng(5).standard_normal(o.n) * active_mask(P)).astype(o.dtype)
    Av_ref = o.apply_jtj(P.params, v)
    o.close()
    s = _solver(monkeypatch, P, None)
    Av, dot = s.apply_jtj(api.to_device(P), torch.from_numpy(v).cuda())
    s.close()
    tol = 1e-11 if double else 3e-5
    err = rel_err(Av.cpu().numpy(), Av_ref)
    dot_ref = float(v.astype(np.float64) @ Av_ref.astype(np.float64))
    print(f"J^T J v {err:.2e}, v . J^T J v {abs(dot - dot_ref) / abs(dot_ref):.2e}")
    assert_close("jtjp", err, 0.0, tol, absolute=True, double=double)
    assert_close("dot", dot, dot_ref, 10 * tol, double=double)      # the bar test_energies_gpu.py::test_cost_jtf_diag_jtjp gives the sum over the workgroups' partials


def test_tile_loop_apply_jtj(oracle_lib, monkeypatch):
    _every([("f64", (oracle_lib, monkeypatch, True)), ("f32", (oracle_lib, monkeypatch, False))], _tile_loop_apply_jtj)


def test_tile_loop_lm_step_with_resets(oracle_lib, monkeypatch):
    """sfs_applyTiled<T, true> through the loop: one LM step of 6 iterations with a residual reset after the 3rd and the 6th."""
    W, H = sc.TILE_LOOP_SHAPE
    kt = _beside(oracle_lib, monkeypatch, W, H, None, True, "LMGPU", 1, 6, 1e-10, 1e-8, 1e-8, 1e-7, residual_reset_period=3)
    assert "PCGStep1" in kt and "PCGIteration" in kt, kt
