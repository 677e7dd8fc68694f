"""GPU tests (-m gpu) of an energy that a plug-in brings: examples/plugins/spring_mesh_deformation.{t,hip}, loaded by path or by OPT_AMD_ENERGY_PLUGINS and solved
through the unmodified Opt_* API on every path the built-in functor mesh energies reach (four launches per PCG iteration, amd_graph_fused = 1, amd_onchip = 6,
amd_onchip = 7 with amd_onchip_workgroups), Gauss-Newton and Levenberg-Marquardt, float and double.

The CPU oracle knows the built-in energies only, so the reference is restated here in numpy (float64): the residual vector, the analytic dense Jacobian
(d|d|/dX = +-d/|d|) and the reference's Gauss-Newton / Jacobi-PCG loop -- PCGInit1 (+ _Finish), PCGStep1-3 and PCGLinearUpdate of solverGPUGaussNewton.t:361-560 with
the CERES guarded inverse 1 / (1 + sqrt(d))^2 (:323-332).  Bars are the README's parity contracts: probes 1e-12 (double) / 1e-5 (float), trajectories 1e-10 (double) /
1e-5 (float).  LM is not restated: its outer logic is energy-independent (tests/test_lm_*_gpu.py); what is energy-specific in it -- diag J^T J, J^T J p with CtC -- is
what the probes and the path comparisons check.

No plug-in is loaded in the pytest process (the registry is process-global): every test runs tests/plugin_energy_driver.py in a fresh child, one at a time, and no
child is started after one that ended abnormally."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plugin_energy_driver as drv
from helpers import rel_err
from opt_amd import build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "plugin_energy_driver.py")
STEM = "spring_mesh_deformation"
_abnormal = []


def child(case, args, env=None, timeout=180):
    if _abnormal:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % _abnormal[0])
    e = dict(os.environ)
    e.pop("OPT_AMD_ENERGY_PLUGINS", None)
    e.update(env or {})
    try:
        r = subprocess.run([sys.executable, DRIVER, case, json.dumps(args)], capture_output=True, text=True, timeout=timeout, env=e)
    except subprocess.TimeoutExpired:
        _abnormal.append(case + ": time limit")
        raise
    if r.returncode != 0:
        _abnormal.append("%s: exit status %d" % (case, r.returncode))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def sample():
    p = build.plugin_path(STEM)
    if not os.path.exists(p):
        build.build_plugin(build.SAMPLE_PLUGIN)
    return p


# ---- the energy in numpy ---------------------------------------------------------------------------------------------------------------------------------------------
def _inputs(P):
    f = np.float64
    return (np.asarray(P.params[1], f), np.asarray(P.params[2], f), float(P.params[3]), float(P.params[4]), np.asarray(P.params[6]), np.asarray(P.params[7]))


def residuals_and_jacobian(P, X):
    """F (3 N vertex residuals, then one per half-edge) and the dense J (rows of F, columns 3 v + c) at X [N, 3]."""
    U, C, wf, wr, v0, v1 = _inputs(P)
    N, E = len(X), len(v0)
    valid = C[:, 0] >= -999999.9
    F = np.zeros(3 * N + E); J = np.zeros((3 * N + E, 3 * N))
    F[:3 * N] = np.where(valid[:, None], wf * (X - np.where(valid[:, None], C, 0.0)), 0.0).reshape(-1)
    for v in np.flatnonzero(valid):
        for c in range(3):
            J[3 * v + c, 3 * v + c] = wf
    d = X[v1] - X[v0]
    ln = np.linalg.norm(d, axis=1)
    u = U[v1] - U[v0]
    F[3 * N:] = wr * (ln - np.linalg.norm(u, axis=1))
    for e in range(E):
        g = wr * d[e] / ln[e]
        J[3 * N + e, 3 * v1[e]:3 * v1[e] + 3] += g
        J[3 * N + e, 3 * v0[e]:3 * v0[e] + 3] -= g
    return F, J


def cost_of(P, X):
    F, _ = residuals_and_jacobian(P, X)
    return 0.5 * float(F @ F)


def gauss_newton(P, nsteps, liters):
    """(costs after init and every step, final X): the reference's loop, in float64 on the problem's own (possibly float32-rounded) inputs."""
    X = np.asarray(P.params[0], np.float64).copy()
    costs = [cost_of(P, X)]
    for _ in range(nsteps):
        F, J = residuals_and_jacobian(P, X)
        r = -(J.T @ F)                                        # PCGInit1
        M = 1.0 / (1.0 + np.sqrt((J * J).sum(0))) ** 2       # guardedInvert (CERES), PCGInit1_Finish
        p = M * r
        delta = np.zeros_like(r)
        a_num = float(r @ p)
        for _ in range(liters):
            Ap = J.T @ (J @ p); a_den = float(p @ Ap)        # PCGStep1
            alpha = a_num / a_den if a_den > 0 else 0.0      # PCGStep2
            delta += alpha * p; r = r - alpha * Ap
            z = M * r; b_num = float(z @ r)
            beta = b_num / a_num if a_num > 0 else 0.0       # PCGStep3
            p = z + beta * p
            a_num = b_num
        X = X + delta.reshape(-1, 3)                          # PCGLinearUpdate
        costs.append(cost_of(P, X))
    return costs, X.reshape(-1)


def _close(name, got, ref, tol):
    err = abs(got - ref) / max(abs(ref), 1e-300)
    print(name, got, ref, "rel", err)
    assert err <= tol, (name, got, ref, err, tol)


def _probes(sample, double, tol):
    out = child("probes", {"plugin": sample, "double": double})
    for mesh in drv.MESHES:
        P, g = drv.problem(mesh, double), out[mesh]
        X = np.asarray(P.params[0], np.float64)
        F, J = residuals_and_jacobian(P, X)
        v = drv.probe_direction(3 * len(X)).astype(np.float64 if double else np.float32).astype(np.float64)
        assert g["n"] == 3 * len(X)
        _close(mesh + " cost", g["cost"], 0.5 * float(F @ F), tol)
        # (OptAmd_EvalJTF hands out J^T F itself; the solver's r is its negative)
        for name, got, ref in (("r", g["r"], J.T @ F), ("diag", g["diag"], (J * J).sum(0)), ("out fused=0", g["out0"], J.T @ (J @ v)), ("out fused=1", g["out1"], J.T @ (J @ v))):
            err = rel_err(got, ref)
            print(mesh, name, "rel", err)
            assert err <= tol, (mesh, name, err, tol)
        Jv = J @ v
        _close(mesh + " dot fused=0", g["dot0"], float(Jv @ Jv), tol)
        _close(mesh + " dot fused=1", g["dot1"], float(Jv @ Jv), tol)
        # the two J^T J p formulations: the same bits in `out` (the engine's guarantee, test_graph_fused_gpu.py::test_apply_jtj_bit_for_bit), the returned p . A p --
        # a sum of the same terms over another grid -- at the probes' own bar
        assert g["out0"] == g["out1"], rel_err(g["out1"], g["out0"])
        _close(mesh + " dot fused=1 vs 0", g["dot1"], g["dot0"], 1e-12)
        if mesh == "grid_shapes":      # the isolated vertex: no residual touches it
            assert g["r"][-3:] == [0.0] * 3 and g["diag"][-3:] == [0.0] * 3 and g["out0"][-3:] == [0.0] * 3


def test_probes_double(sample):
    _probes(sample, True, 1e-12)


def test_probes_float(sample):
    _probes(sample, False, 1e-5)


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------------------------------------
def _run(name, mesh, kind, nsteps, liters, double=True, **params):
    return dict(name=name, mesh=mesh, double=double, kind=kind, nsteps=nsteps, liters=liters, params=params)


@pytest.fixture(scope="module")
def gn_default(sample):
    """GN 3 x 10, double, the 35-vertex grid, default path, plug-in loaded by path."""
    return child("solves", {"plugin": sample, "runs": [_run("gn", "grid", "GN", 3, 10)]})["gn"]


def test_gauss_newton_trajectory_double(gn_default):
    P = drv.problem("grid", True)
    costs, x = gauss_newton(P, 3, 10)
    g = gn_default
    assert g["ret"] == [1, 1, 1, 0] and len(g["cost"]) == 5 and g["cost"][4] == g["cost"][3], g      # (the call that ends the solve takes no step)
    for k in range(4):
        _close("cost after step %d" % k, g["cost"][k], costs[k], 1e-10)
    err = rel_err(g["x"], x)
    print("x rel", err)
    assert err <= 1e-10
    assert all(b < a for a, b in zip(g["cost"][:4], g["cost"][1:4])), g["cost"]
    assert g["status"] == 0 and g["describe"]["path"] == "launch-per-iteration" and "launches_per_iteration" not in g["describe"], g["describe"]


def _accepts(rec):
    return [b < a for a, b in zip(rec["cost"], rec["cost"][1:])]


def _same_trajectory(name, got, want, lm):
    assert got["ret"] == want["ret"] and len(got["cost"]) == len(want["cost"]), (name, got["ret"], want["ret"])
    for k, (a, b) in enumerate(zip(got["cost"], want["cost"])):
        _close("%s cost %d" % (name, k), a, b, 1e-10)
    if lm:
        assert _accepts(got) == _accepts(want), (name, got["cost"], want["cost"])
        for k, (a, b) in enumerate(zip(got["radius"], want["radius"])):
            _close("%s radius %d" % (name, k), a, b, 1e-10)
    print(name, "x rel", rel_err(got["x"], want["x"]))      # (reported; the bars of the paths are on costs and radius)
    assert np.isfinite(got["x"]).all()


def _strip(d):
    return {k: v for k, v in d.items() if k != "amd_onchip"}


PATHS = [("fused", "grid", dict(amd_graph_fused=1)), ("onchip6", "grid", dict(amd_onchip=6)), ("grid4", "armadillo", dict(amd_onchip=7, amd_onchip_workgroups=4)),
         ("seven_auto", "grid", dict(amd_onchip=7, amd_onchip_workgroups=0))]


@pytest.mark.parametrize("kind,controls", [("GN", {}), ("LM", dict(residual_reset_period=4)), ("LM", dict(residual_reset_period=10))], ids=["GN", "LM-reset-inside", "LM-no-reset"])
def test_every_path_of_the_functor_energies(sample, kind, controls):
    """3 x 10 in double on every path, beside the default path on the same mesh: the path is taken and visible, per-step costs at 1e-10, LM's return values, accept /
    reject sequence and radius (1e-10).  LM: lIterations = 10 once above residual_reset_period (a reset inside the linear solve) and once at it."""
    lm = kind == "LM"
    runs = [_run("default_grid", "grid", kind, 3, 10, **controls), _run("default_armadillo", "armadillo", kind, 3, 10, **controls)]
    runs += [_run(n, mesh, kind, 3, 10, **controls, **p) for n, mesh, p in PATHS]
    out = child("solves", {"plugin": sample, "runs": runs})
    assert out["names"][-1] == STEM and len(out["names"]) == 13
    for mesh in ("grid", "armadillo"):
        d = out["default_" + mesh]
        assert d["status"] == 0 and d["describe"]["path"] == "launch-per-iteration" and d["describe"]["solver"] == kind, d["describe"]
        assert np.isfinite(d["cost"]).all() and d["cost"][-1] < d["cost"][0]
    prec, sol = "double", kind
    d = out["fused"]["describe"]
    assert d["path"] == "launch-per-iteration" and d["launches_per_iteration"] == "2" and d["kernels"] == "ge_flatStep+ge_gather<%s, SpringG, %s>" % (prec, sol), d
    assert out["fused"]["status"] == 0
    d = out["onchip6"]["describe"]
    assert d["path"] == "on-chip" and d["workgroups"] == "1" and d["vertices"] == "35" and d["variant"] == "ge_onchipPcg<%s, SpringG, 1, %s>" % (prec, sol), d
    assert out["onchip6"]["status"] == 1
    d = out["grid4"]["describe"]
    assert d["path"] == "on-chip" and d["workgroups"] == "4" and d["vertices"] == "130" and d["variant"] == "ge_onchipPcgGrid<%s, SpringG, %s>" % (prec, sol), d
    assert out["grid4"]["status"] == 1
    # amd_onchip = 7 without a workgroup count: the defaults base names no automatic choice, so level 6's behaviour, and PlanDescribe says so
    assert _strip(out["seven_auto"]["describe"]) == _strip(out["onchip6"]["describe"]) and out["seven_auto"]["describe"]["amd_onchip"] == "7", out["seven_auto"]["describe"]
    assert out["seven_auto"]["status"] == 1 and out["seven_auto"]["cost"] == out["onchip6"]["cost"] and out["seven_auto"]["x"] == out["onchip6"]["x"]
    for name, mesh, _ in PATHS:
        _same_trajectory(name, out[name], out["default_" + mesh], lm)


def test_float(sample):
    """GN 2 x 8 in float on the 35-vertex grid, default path and amd_onchip = 6: the cost after step 1 within 1e-5 of the numpy loop."""
    out = child("solves", {"plugin": sample, "runs": [_run("default", "grid", "GN", 2, 8, double=False), _run("onchip6", "grid", "GN", 2, 8, double=False, amd_onchip=6)]})
    costs, _ = gauss_newton(drv.problem("grid", False), 2, 8)
    for name in ("default", "onchip6"):
        _close(name + " cost 0", out[name]["cost"][0], costs[0], 1e-5)
        _close(name + " cost after step 1", out[name]["cost"][1], costs[1], 1e-5)
    d = out["onchip6"]["describe"]
    assert d["path"] == "on-chip" and d["variant"] == "ge_onchipPcg<float, SpringG, 1, GN>" and out["onchip6"]["status"] == 1, d
    assert out["default"]["status"] == 0


def test_environment_route_end_to_end(sample, gn_default):
    """OPT_AMD_ENERGY_PLUGINS in the child's environment, no load call: the solve of test_gauss_newton_trajectory_double, the same bits."""
    out = child("solves", {"runs": [_run("gn", "grid", "GN", 3, 10)]}, env={"OPT_AMD_ENERGY_PLUGINS": sample})
    assert out["names"][-1] == STEM
    assert out["gn"]["cost"] == gn_default["cost"] and out["gn"]["x"] == gn_default["x"] and out["gn"]["cost"][-1] == gn_default["cost"][-1]


def test_built_ins_next_to_a_plugin(sample):
    """embedded_mesh_deformation on the 7 x 5 patch, GN 2 x 8 in double: bit-identical costs and unknowns with and without a loaded plug-in."""
    run = dict(_run("emb", "grid", "GN", 2, 8), energy="embedded")
    with_plugin = child("solves", {"plugin": sample, "runs": [run]})
    without = child("solves", {"runs": [run]})
    assert len(with_plugin["names"]) == 13 and len(without["names"]) == 12 and with_plugin["names"][:12] == without["names"]
    assert with_plugin["emb"]["cost"] == without["emb"]["cost"] and with_plugin["emb"]["x"] == without["emb"]["x"]
    assert without["emb"]["ret"] == [1, 1, 0] and without["emb"]["cost"][2] < without["emb"]["cost"][0]
