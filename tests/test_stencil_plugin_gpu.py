"""GPU tests (-m gpu) of image-domain energy plug-ins and of the two-launch PCG iteration of the functor stencil engine (solver parameter amd_stencil_fused = 1:
ge_flatStep / ge_flatStepNoPre + se_gatherIter, opt_amd/csrc/stencil_engine.h).

The sample examples/plugins/vector_tv_denoising.{t,hip} is loaded by path or by OPT_AMD_ENERGY_PLUGINS and solved through the unmodified Opt_* API; its reference is
the numpy restatement of tests/stencil_plugin_cases.py (float64), whose cases tests/test_stencil_plugin_cases_cpu.py has shown fit for the float bars.  Bars are the
README's parity contracts: probes 1e-12 (double) / 1e-5 (float), trajectories 1e-10 (double) / 1e-5 (float).  The built-in functor stencil energies run under the
parameter against the CPU oracle with the bars tests/test_energies_gpu.py::test_trajectory holds them to (tests/golden/parity_bars.json, float_envelopes.json).

No plug-in is loaded in the pytest process (the registry is process-global): every test runs tests/stencil_plugin_driver.py in a fresh child, one at a time, with a
time limit, and no child is started after one that ended abnormally."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_plugin_cases as sc
import stencil_plugin_driver as drv
from helpers import flat_unknowns, oracle_solver, rel_err
from opt_amd import build
from test_energies_gpu import ENVELOPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "stencil_plugin_driver.py")
STEM = "vector_tv_denoising"
NAMES = [c["name"] for c in sc.CASES]
_abnormal = []


def child(case, args, env=None, timeout=240):
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
        build.build_plugin(build.SAMPLE_STENCIL_PLUGIN)
    return p


def _close(name, got, ref, tol):
    err = abs(got - ref) / max(abs(ref), 1e-300)
    print(name, got, ref, "rel", err)
    assert err <= tol, (name, got, ref, err, tol)


# ---- probes ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
def test_probes(sample, double):
    """EvalCost, EvalJTF with the diagonal and ApplyJTJ of the sample against numpy on every case."""
    tol = sc.BARS["probe"][double]
    out = child("probes", {"plugin": sample, "double": double, "cases": NAMES})
    for name in NAMES:
        P, g = sc.problem(sc.case(name), double), out[name]
        m = sc.Model(P)
        v = sc.probe_direction(m.X.size).astype(np.float64 if double else np.float32).astype(np.float64)
        assert g["n"] == m.X.size
        _close(name + " cost", g["cost"], m.cost(), tol)
        Av = m.jtj(v)
        for what, got, ref in (("r", g["r"], m.jtf()), ("diag", g["diag"], m.diag()), ("out", g["out"], Av)):      # (OptAmd_EvalJTF hands out J^T F itself)
            err = rel_err(got, ref)
            print(name, what, "rel", err)
            assert err <= tol, (name, what, err, tol)
        _close(name + " dot", g["dot"], float(v @ Av), tol)
        ex = np.repeat(m.ex.reshape(-1), 2)      # rows of excluded unknowns are exactly 0
        assert not np.asarray(g["r"])[ex].any() and not np.asarray(g["diag"])[ex].any() and not np.asarray(g["out"])[ex].any()


# ---- Gauss-Newton trajectories -----------------------------------------------------------------------------------------------------------------------------------------
def _run(name, case=None, kind="GN", nsteps=sc.GN_STEPS, liters=sc.GN_LITERS, double=True, energy="tv", trace=False, **params):
    return dict(name=name, case=case, energy=energy, double=double, kind=kind, nsteps=nsteps, liters=liters, params=params, trace=trace)


@pytest.fixture(scope="module")
def gn(sample):
    """GN 3 x 10 on every case under amd_stencil_fused = 0 and 1, plug-in loaded by path: {double: child output}."""
    return {double: child("solves", {"plugin": sample, "runs": [_run("%s|%d" % (n, f), n, double=double, amd_stencil_fused=f) for n in NAMES for f in (0, 1)]}) for double in (True, False)}


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
def test_gauss_newton_trajectory(gn, double, fused):
    """The costs after every step and the unknowns against the numpy loop, on the three-launch loop and on the two-launch one."""
    tol = sc.BARS["trajectory"][double]
    out = gn[double]
    assert out["names"][-1] == STEM and len(out["names"]) == 13
    for name in NAMES:
        g = out["%s|%d" % (name, fused)]
        costs, x = sc.gauss_newton(sc.problem(sc.case(name), double))
        assert g["ret"] == [1, 1, 1, 0] and len(g["cost"]) == 5 and g["cost"][4] == g["cost"][3], g["ret"]      # (the call that ends the solve takes no step)
        for k in range(4):
            _close("%s fused=%d cost after step %d" % (name, fused, k), g["cost"][k], costs[k], tol)
        err = rel_err(g["x"], x)
        print(name, "x rel", err)
        assert err <= tol, (name, err)
        d = g["describe"]
        assert g["status"] == 0 and d["path"] == "launch-per-iteration" and d["solver"] == "GN", d
        if fused:
            assert d["launches_per_iteration"] == "2" and d["kernels"] == "ge_flatStep+se_gatherIter<%s, VectorTvE, GN>" % ("double" if double else "float"), d
        else:
            assert "launches_per_iteration" not in d and d["why_not_fused"] == "amd_stencil_fused=1 was not set", d


def test_environment_route_end_to_end(sample, gn):
    """OPT_AMD_ENERGY_PLUGINS in the child's environment, no load call: the solves of the by-path child, the same bits, on both loops."""
    runs = [_run("%s|%d" % (n, f), n, amd_stencil_fused=f) for n in ("13x9-block", "130x37-border") for f in (0, 1)]
    out = child("solves", {"runs": runs}, env={"OPT_AMD_ENERGY_PLUGINS": sample})
    assert out["names"][-1] == STEM
    for r in runs:
        assert out[r["name"]]["cost"] == gn[True][r["name"]]["cost"] and out[r["name"]]["x"] == gn[True][r["name"]]["x"], r["name"]


# ---- Levenberg-Marquardt: the same outer decisions on both loops ---------------------------------------------------------------------------------------------------------
# 1 x 7 with an excluded block: the residuals centred on the excluded pixel count in J^T F of its neighbours but not in the cost, so near the minimum a model step can
# raise the cost -- and LM must reject it.  lIterations = 10 above residual_reset_period = 4: resets fall inside the linear solve, the restart launch runs.
LM_CASE, LM_STEPS, LM_CONTROLS = "1x7-block", 8, dict(residual_reset_period=4)


def _accepts(rec):
    return [b < a for a, b in zip(rec["cost"], rec["cost"][1:])]


@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
def test_levenberg_marquardt_same_decisions_on_both_loops(sample, double):
    tol = sc.BARS["trajectory"][double]
    runs = [_run("lm|%d" % f, LM_CASE, "LM", LM_STEPS, 10, double=double, amd_stencil_fused=f, **LM_CONTROLS) for f in (0, 1)]
    runs += [_run("big|%d" % f, "130x37-block", "LM", 3, 10, double=double, amd_stencil_fused=f, **LM_CONTROLS) for f in (0, 1)]
    out = child("solves", {"plugin": sample, "runs": runs})
    for tag in ("lm", "big"):
        a, b = out[tag + "|0"], out[tag + "|1"]
        print(tag, "costs", a["cost"], b["cost"], "radius", a["radius"], b["radius"])
        assert a["ret"] == b["ret"] and len(a["cost"]) == len(b["cost"]), (a["ret"], b["ret"])
        assert _accepts(a) == _accepts(b), (a["cost"], b["cost"])
        for k, (x, y) in enumerate(zip(b["cost"], a["cost"])):
            _close("%s cost %d" % (tag, k), x, y, tol)
        for k, (x, y) in enumerate(zip(b["radius"], a["radius"])):
            _close("%s radius %d" % (tag, k), x, y, tol)
        d = b["describe"]
        assert d["launches_per_iteration"] == "2" and d["kernels"] == "ge_flatStep+se_gatherIter<%s, VectorTvE, LM>" % ("double" if double else "float") and d["solver"] == "LM", d
        assert "launches_per_iteration" not in a["describe"]
        assert np.isfinite(b["x"]).all() and b["cost"][-1] < b["cost"][0]
    steps = _accepts(out["lm|0"])[:len(out["lm|0"]["ret"]) - 1]
    assert not all(steps) and any(steps), out["lm|0"]["cost"]      # at least one step rejected (and one accepted)


# ---- J^T J p of a two-launch iteration: the bits of the probe -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
def test_apply_jtj_bit_for_bit(sample, double):
    """Under amd_stencil_fused = 1 the A p the last two-launch iteration of a step wrote (se_gatherIter) equals OptAmd_ApplyJTJ (se_gather) of the same p, bit for bit."""
    out = child("apply_bits", {"plugin": sample, "double": double, "cases": NAMES, "liters": 3})
    for name in NAMES:
        g = out[name]
        assert g["describe"]["launches_per_iteration"] == "2", g["describe"]
        assert np.any(np.asarray(g["p"]) != 0) and np.any(np.asarray(g["Ap"]) != 0), name
        assert g["Ap"] == g["probe"], (name, rel_err(g["Ap"], g["probe"]))


def test_trace_rows_agree_with_the_three_launch_loop(sample):
    """The PCG trace rows (alphaNumerator, alphaDenominator, betaNumerator) of a 10-iteration double Gauss-Newton solve under 0 and 1 at 1e-9: the bar of the same
    comparison between the mesh engine's loops (tests/test_onchip_graph_gpu.py)."""
    runs = [_run("%s|%d" % (n, f), n, nsteps=1, liters=10, trace=True, amd_stencil_fused=f) for n in ("13x9-block", "130x37-nomask") for f in (0, 1)]
    out = child("solves", {"plugin": sample, "runs": runs})
    for n in ("13x9-block", "130x37-nomask"):
        a, b = np.asarray(out[n + "|0"]["trace"]), np.asarray(out[n + "|1"]["trace"])
        assert a.shape == b.shape == (10, 6), (a.shape, b.shape)
        assert (a[:, :2] == b[:, :2]).all()
        for col, what in ((2, "alphaNumerator"), (3, "alphaDenominator"), (4, "betaNumerator")):
            err = float(np.max(np.abs(a[:, col] - b[:, col]) / np.abs(a[:, col])))
            print(n, what, "max rel", err)
            assert err <= 1e-9, (n, what, err)


def test_describe_says_why_not(sample):
    """amd_reference_order = 1 wins over the parameter, and 0 is 0: both keep the three launches and say why."""
    runs = [_run("ref", "13x9-block", nsteps=1, liters=4, amd_stencil_fused=1, amd_reference_order=1), _run("off", "13x9-block", nsteps=1, liters=4, amd_stencil_fused=0),
            _run("on", "13x9-block", nsteps=1, liters=4, amd_stencil_fused=1)]
    out = child("solves", {"plugin": sample, "runs": runs})
    for key in ("describe_before", "describe"):
        d = out["ref"][key]
        assert d["path"].startswith("reference-order") and d["amd_reference_order"] == "1" and "amd_reference_order" in d["why_not_fused"] and "launches_per_iteration" not in d, d
        d = out["off"][key]
        assert d["path"] == "launch-per-iteration" and d["why_not_fused"] == "amd_stencil_fused=1 was not set" and "launches_per_iteration" not in d, d
        d = out["on"][key]
        assert d["path"] == "launch-per-iteration" and d["launches_per_iteration"] == "2" and "why_not_fused" not in d, d
    assert out["ref"]["cost"] == out["off"]["cost"] and out["ref"]["x"] == out["off"]["x"]      # (both ran the reference-order loop: the same bits)


# ---- the built-in functor stencil energies under the parameter, against the CPU oracle -------------------------------------------------------------------------------------
BUILTIN_RUNS = [      # (driver's builder, test_energies_gpu's case name for the bars, solver, plan parameters, environment)
    ("flow_13x9", "flow", "LM", dict(amd_onchip=0), {}),            # unpreconditioned: the p_0 = M_0 r_0 start of ge_flatStepNoPre
    ("flow_130x37", "flow", "LM", dict(amd_onchip=0), {}),
    ("intrinsic_29x23", "intrinsic", "LM", dict(amd_onchip=0), {}),  # ComputedArrays, two unknown images
    ("volumetric_5x4x3", "volumetric", "LM", {}, {"OPT_AMD_VOLUMETRIC_ARAP": "0"}),      # 3-D, preconditioned
    ("volumetric_5x4x3", "volumetric", "GN", {}, {"OPT_AMD_VOLUMETRIC_ARAP": "0"}),
]
NSTEPS, LITERS = 4, 12      # test_energies_gpu.py::test_trajectory's recipe, whose bars these are


def _bars(name, kind, double):
    """(cost bar, unknowns bar) of tests/test_energies_gpu.py::test_trajectory for this energy: tests/golden/parity_bars.json in double, the contract or twice the
    diameter of the frozen legal oracle runs (tests/golden/float_envelopes.json) in float."""
    if double:
        pb = json.load(open(os.path.join(HERE, "golden", "parity_bars.json")))
        kd = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}[kind]
        own = "tests/test_energies_gpu.py::test_trajectory[%s-f64-%s]|double|" % (name, kd)
        gen = "tests/test_energies_gpu.py::test_trajectory|double|"
        return pb.get(own + "cost", pb[gen + "cost"])["bar"], pb.get(own + "x", pb[gen + "x"])["bar"]
    ctol, xtol = 1e-5, 2e-5
    env = ENVELOPES.get("%s_%s" % (name, {"GN": "gaussNewtonGPU", "LM": "LMGPU"}[kind]))
    if env is not None:
        ctol, xtol = max(ctol, 2.0 * env[0]), max(xtol, 2.0 * env[1])
    return ctol, xtol


@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
@pytest.mark.parametrize("builder,bars_of,kind,params,env", BUILTIN_RUNS, ids=["%s-%s" % (b[0], b[2]) for b in BUILTIN_RUNS])
def test_built_ins_under_the_parameter(oracle_lib, sample, builder, bars_of, kind, params, env, double):
    """4 x 12 under amd_stencil_fused = 0 beside 1, each against the CPU oracle; the plug-in is loaded and solved in the same process."""
    ctol, xtol = _bars(bars_of, kind, double)
    P = drv.BUILTINS[builder](double)
    o = oracle_solver(oracle_lib, P, drv.KINDS[kind], nIterations=NSTEPS, lIterations=LITERS)
    Pref = P.clone()
    o.init(Pref.params)
    costs, rets = [o.cost()], []
    while True:
        more = o.step(Pref.params)
        rets.append(int(more)); costs.append(o.cost())
        if not more:
            break
    o.close()
    runs = [_run("b|%d" % f, None, kind, NSTEPS, LITERS, double=double, energy=builder, amd_stencil_fused=f, **params) for f in (0, 1)]
    runs.append(_run("tv", "13x9-block", double=double, amd_stencil_fused=1))
    out = child("solves", {"plugin": sample, "runs": runs}, env=env)
    assert len(out["names"]) == 13 and out["tv"]["describe"]["launches_per_iteration"] == "2" and out["tv"]["cost"][3] < out["tv"]["cost"][0]
    scale = max(abs(costs[0]), 1e-300)
    for f in (0, 1):
        g = out["b|%d" % f]
        d = g["describe"]
        print(builder, kind, "fused", f, d)
        assert g["status"] == 0 and d["solver"] == kind and "on-chip" not in d["path"], d
        if f:
            flat = "ge_flatStep" if bars_of == "volumetric" else "ge_flatStepNoPre"
            assert d["launches_per_iteration"] == "2" and d["kernels"].startswith(flat + "+se_gatherIter<%s, " % ("double" if double else "float")) and d["kernels"].endswith(", %s>" % kind), d
        else:
            assert "launches_per_iteration" not in d, d
        assert g["ret"] == rets, (g["ret"], rets)
        _close("cost0", g["cost"][0], costs[0], 1e-12 if double else 1e-5)
        for k in range(1, len(costs)):      # relative to the initial cost, as test_trajectory compares
            err = abs(g["cost"][k] - costs[k]) / max(abs(costs[k]), 1e-7 * scale)
            print("fused", f, "cost", k, g["cost"][k], costs[k], "rel", err)
            assert err <= ctol, (f, k, err, ctol)
        err = rel_err(g["x"], flat_unknowns(Pref))
        print("fused", f, "x rel", err)
        assert err <= xtol, (f, err, xtol)
