"""GPU tests (-m gpu) of energies generated from .t files (opt_amd/tgen.py): six generated plug-ins beside their comparators on the same arrays.

Comparators: for vector_tv_denoising and spring_mesh_deformation the hand-written plug-in of examples/plugins/, loaded in a child of its own (one process cannot
register one name twice); for the gen_ copies of image_warping, arap_mesh_deformation, embedded_mesh_deformation and cotangent_mesh_smoothing the built-in kernel
set, in the same child.  Bars: the README's parity contracts -- probes 1e-12 of the vector's max-abs in double, 1e-5 in float; per-step costs 1e-10 in double, 1e-5
in float.  A probe case whose hand-written comparator orders an expression differently is listed with its reason in tests/golden/tgen_bars.json; its bar is twice
the distance between the comparator and the CPU oracle's probe on the same input (neither is code under test), never above 1e-9.

No plug-in is loaded in the pytest process: every case runs tests/tgen_driver.py in a fresh child, one at a time, and no child is started after one that ended
abnormally."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tgen_cases as tc
from opt_amd import build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "tgen_driver.py")
_abnormal = []
EXTRA_BARS = json.load(open(os.path.join(HERE, "golden", "tgen_bars.json")))["bars"]


def child(case, args, timeout=240):
    if _abnormal:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % _abnormal[0])
    e = dict(os.environ)
    e.pop("OPT_AMD_ENERGY_PLUGINS", None)
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
def libs(tmp_path_factory):
    """{name: (library, .t)} of the six, built with force=False, at most four compilers at once; the hand-written samples are built if they are missing."""
    tmp = tmp_path_factory.mktemp("tgen")
    for stem, src in (("spring_mesh_deformation", build.SAMPLE_PLUGIN), ("vector_tv_denoising", build.SAMPLE_STENCIL_PLUGIN)):
        if not os.path.exists(build.plugin_path(stem)):
            build.build_plugin(src)
    built = tc.build_all(tmp, jobs=4, force=False)
    return {n: (built[n], tc.t_file(n, tmp)) for n in tc.SIX}


def sides_of(name, libs):
    """[(child arguments, {side name: .t})]: one child with both sides for a gen_ copy, two children for a sample."""
    lib, t = libs[name]
    if name in tc.SAMPLES:
        return [({"plugins": [lib]}, {"gen": t}), ({"plugins": [build.plugin_path(name)]}, {"ref": t})]
    from opt_amd import api
    return [({"plugins": [lib]}, {"gen": t, "ref": api.energy_file(tc.builtin_of(name))})]


def max_abs_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300)) if got.size else 0.0


def rel(got, ref):
    return abs(got - ref) / max(abs(ref), 1e-300)


# ---- probes ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
@pytest.mark.parametrize("name", tc.SIX)
def test_probes(libs, name, double):
    """OptAmd_EvalCost, EvalJTF (J^T F and the diagonal) and ApplyJTJ (the vector and the returned scalar) of the generated energy against its comparator on every
    input of the energy: images 5 x 3, 13 x 9 and 67 x 5 with masks none / block / border, meshes grid, grid_shapes and armadillo."""
    inputs = tc.inputs_of(name)
    out = {}
    for args, sides in sides_of(name, libs):
        got = child("probes", dict(args, energy=name, double=double, inputs=inputs, sides=[{"name": k, "t": t} for k, t in sides.items()]))
        for inp in inputs:
            out.setdefault(inp, {}).update(got[inp])
    worst = {}
    for inp in inputs:
        g, r = out[inp]["gen"], out[inp]["ref"]
        assert g["n"] == r["n"] > 0
        for key in ("cost", "dot"):
            bar = tc.BARS["probe"][double]
            case = "%s/%s/%s/%s" % (name, "double" if double else "float", inp, key)
            if double and case in EXTRA_BARS:
                bar = EXTRA_BARS[case]["bar"]
                assert tc.BARS["probe"][True] < bar <= 1e-9 and EXTRA_BARS[case]["reason"], case
            err = rel(g[key], r[key])
            print(case, g[key], r[key], "rel", err, "bar", bar)
            worst[case] = (err, bar)
        for key in ("r", "diag", "out"):
            bar = tc.BARS["probe"][double]
            case = "%s/%s/%s/%s" % (name, "double" if double else "float", inp, key)
            if double and case in EXTRA_BARS:
                bar = EXTRA_BARS[case]["bar"]
                assert tc.BARS["probe"][True] < bar <= 1e-9 and EXTRA_BARS[case]["reason"], case
            err = max_abs_err(g[key], r[key])
            print(case, "max-abs rel", err, "bar", bar)
            worst[case] = (err, bar)
        assert r["cost"] > 0 and np.max(np.abs(r["r"])) > 0 and np.max(np.abs(r["out"])) > 0      # (the input exercises the energy)
    failed = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not failed, failed


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------------------------------
def trajectory_input(name):
    return "13x9-block" if name in tc.IMAGE_ENERGIES else "grid"


def run_sides(libs, name, runs):
    """Every run on the generated side and on the comparator's: {run name: {"gen": record, "ref": record}}."""
    out = {}
    for args, sides in sides_of(name, libs):
        rs = [dict(r, name=r["name"] + "/" + s, side=s, energy=name) for r in runs for s in sides]
        got = child("solves", dict(args, sides=sides, runs=rs))
        for r in runs:
            for s in sides:
                out.setdefault(r["name"], {})[s] = got[r["name"] + "/" + s]
    return out


def accepts(rec):
    return [b < a for a, b in zip(rec["cost"], rec["cost"][1:])]


def same_trajectory(case, got, want, double, lm):
    bar = tc.BARS["trajectory"][double]
    assert got["ret"] == want["ret"] and len(got["cost"]) == len(want["cost"]), (case, got["ret"], want["ret"])
    assert np.isfinite(got["cost"]).all() and np.isfinite(got["x"]).all()
    for k, (a, b) in enumerate(zip(got["cost"], want["cost"])):
        err = rel(a, b)
        print(case, "cost", k, a, b, "rel", err)
        assert err <= bar, (case, k, a, b, err, bar)
    if lm:
        assert accepts(got) == accepts(want), (case, got["cost"], want["cost"])


@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
@pytest.mark.parametrize("name", tc.SIX)
def test_trajectories(libs, name, double):
    """GN 3 x 10 and LM 3 x 10: every step's cost beside the comparator's; LM's return values and accept / reject decisions identical."""
    inp = trajectory_input(name)
    runs = [dict(name=k, input=inp, double=double, kind=k, nsteps=3, liters=10, params={}) for k in ("GN", "LM")]
    out = run_sides(libs, name, runs)
    for k in ("GN", "LM"):
        g = out[k]["gen"]
        assert g["ret"] == [1, 1, 1, 0] and g["cost"][3] < g["cost"][0], (k, g["ret"], g["cost"])
        same_trajectory("%s/%s/%s" % (name, "double" if double else "float", k), g, out[k]["ref"], double, k == "LM")


# ---- paths -------------------------------------------------------------------------------------------------------------------------------------------------------
PATHS = [
    ("vector_tv_denoising", dict(amd_stencil_fused=1), {"path": "launch-per-iteration", "launches_per_iteration": "2"}),
    ("gen_image_warping", dict(amd_stencil_fused=1), {"path": "launch-per-iteration", "launches_per_iteration": "2"}),
    ("spring_mesh_deformation", dict(amd_graph_fused=1), {"path": "launch-per-iteration", "launches_per_iteration": "2"}),
    ("gen_embedded_mesh_deformation", dict(amd_graph_fused=1), {"path": "launch-per-iteration", "launches_per_iteration": "2"}),
    ("spring_mesh_deformation", dict(amd_onchip=6), {"path": "on-chip", "workgroups": "1"}),
    ("gen_arap_mesh_deformation", dict(amd_onchip=6), {"path": "on-chip", "workgroups": "1"}),
]


@pytest.mark.parametrize("name,params,says", PATHS, ids=["%s-%s" % (n, "-".join("%s=%s" % kv for kv in p.items())) for n, p, _ in PATHS])
def test_paths(libs, name, params, says):
    """The path is asserted from OptAmd_PlanDescribe -- a why_not_... answer fails the case, so a refusal cannot pass as agreement -- and on it GN 3 x 10 and
    LM 3 x 10 in double agree with the comparator under the same setting, step by step."""
    inp = trajectory_input(name)
    runs = [dict(name=k, input=inp, double=True, kind=k, nsteps=3, liters=10, params=params) for k in ("GN", "LM")]
    out = run_sides(libs, name, runs)
    for k in ("GN", "LM"):
        g = out[k]["gen"]
        for d in (g["describe_before"], g["describe"]):
            assert not [key for key in d if key.startswith("why_not")], d
            for key, v in says.items():
                assert d.get(key) == v, (key, d)
            assert "Gen_" + name in d.get("kernels", d.get("variant", "")), d
        assert g["status"] == (1 if says["path"] == "on-chip" else 0), (g["status"], g["describe"])
        same_trajectory("%s/%s/%s" % (name, "-".join(params), k), g, out[k]["ref"], True, k == "LM")


# ---- the round trip ----------------------------------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_unmodified_api(libs, tmp_path):
    """api.compile_and_load_energy on an energy nobody wrote a functor for (spring_mesh_deformation plus a smoothness term, written for this test); its probes
    against the numpy restatement of tests/tgen_cases.py at the double bar; Opt_ProblemSolve lowers the cost."""
    from opt_amd import tgen
    t = str(tmp_path / (tc.ROUND_TRIP_STEM + ".t"))
    open(t, "w").write(tc.ROUND_TRIP_T)
    tgen.compile_energy(t, force=False)      # (the child then finds the library up to date)
    out = child("round_trip", {"t": t})
    assert tc.ROUND_TRIP_STEM not in out["before"] and out["names"] == out["before"] + [tc.ROUND_TRIP_STEM]
    assert out["check"] == [True, "ok: " + tc.ROUND_TRIP_STEM], out["check"]
    P = tc.round_trip_problem(True)
    X = np.asarray(P.params[0], np.float64)
    F, J = tc.round_trip_residuals_and_jacobian(P, X)
    v = tc.probe_direction(3 * len(X))
    g = out["probe"]
    assert g["n"] == 3 * len(X)
    Jv = J @ v
    for key, got, ref in (("cost", g["cost"], 0.5 * float(F @ F)), ("dot", g["dot"], float(Jv @ Jv))):
        print(key, got, ref, "rel", rel(got, ref))
        assert rel(got, ref) <= 1e-12, (key, got, ref)
    for key, ref in (("r", J.T @ F), ("diag", (J * J).sum(0)), ("out", J.T @ Jv)):
        err = max_abs_err(g[key], ref)
        print(key, "max-abs rel", err)
        assert err <= 1e-12, (key, err)
    assert abs(out["cost_before"] - g["cost"]) <= 1e-12 * g["cost"]
    assert out["cost_after"] < out["cost_before"], (out["cost_before"], out["cost_after"])
    assert out["describe"]["path"] == "launch-per-iteration" and np.isfinite(out["x"]).all()
