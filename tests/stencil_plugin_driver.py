"""Child-process body of the image-domain plug-in tests (test_stencil_plugin_cpu.py, test_stencil_plugin_gpu.py).

The kernel registry of libOpt.so is process-global and other tests enumerate it, so nothing loads a plug-in inside the pytest process: every case runs here,
    python tests/stencil_plugin_driver.py <case> '<json arguments>'
and prints ONE line of JSON (floats by repr: they round-trip bit for bit).  The inputs come from tests/stencil_plugin_cases.py, which parent and child both import;
importing this module loads nothing."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import stencil_plugin_cases as sc      # noqa: E402
from opt_amd import workloads as wl      # noqa: E402

TV_T = wl.VECTOR_TV_T
KINDS = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}
# the built-in functor stencil energies on the grids of the GPU tests ("the p_0 = r_0 / 4 start": optical_flow and intrinsic do not precondition)
BUILTINS = {
    "flow_13x9": lambda double: wl.optical_flow(13, 9, double=double, seed=2, init_flow=1.2),
    "flow_130x37": lambda double: wl.optical_flow(130, 37, double=double, seed=2, init_flow=1.2),
    "intrinsic_29x23": lambda double: wl.intrinsic_image_decomposition(29, 23, double=double, seed=4),
    "volumetric_5x4x3": lambda double: wl.volumetric_mesh_deformation(5, 4, 3, double=double, seed=5, perturb=0.05),
}


def _api():
    from opt_amd import api
    return api


# ---- host-only case ----------------------------------------------------------------------------------------------------------------------------------------------
def case_load(a):
    api = _api()
    before = api.registered_energies()
    refused = api.check_problem_file(TV_T)
    n = api.load_energy_plugin(a["plugin"])
    out = {"n": n, "before": before, "names": api.registered_energies(), "refused_before": refused, "hash": "%016x" % api.problem_file_hash(TV_T), "own": api.check_problem_file(TV_T)}
    src = open(TV_T).read()
    moved = src.replace('Array("A", opt_float2, {W,H}, 1)', 'Array("A", opt_float2, {W,H}, 4)')
    retyped = src.replace('Array("Mask", opt_float, {W,H}, 2)', 'Array("Mask", opt_float2, {W,H}, 2)')
    nopre = src.replace("UsePreconditioner(true)", "UsePreconditioner(false)")
    assert moved != src and retyped != src and nopre != src
    for key, text in (("moved_index", moved), ("retyped", retyped), ("no_preconditioner", nopre)):
        d = os.path.join(a["tmp"], key); os.makedirs(d, exist_ok=True)
        p = os.path.join(d, "vector_tv_denoising.t"); open(p, "w").write(text)
        out[key] = api.check_problem_file(p)
    return out


# ---- GPU cases -----------------------------------------------------------------------------------------------------------------------------------------------------
def _load(a):
    if a.get("plugin"):
        _api().load_energy_plugin(a["plugin"])      # (else: OPT_AMD_ENERGY_PLUGINS, or nothing)


def _solver(P, t_file, kind, params):
    g = _api().Solver(t_file, KINDS[kind], P.dims, double=P.double)
    for k, v in params.items():
        g.set_parameter(k, v)
    return g


def _np(t):
    return t.cpu().numpy().astype(np.float64).tolist()


def case_probes(a):
    """EvalCost, EvalJTF with the diagonal and ApplyJTJ of the sample on every named case."""
    import torch
    _load(a)
    out = {}
    for name in a["cases"]:
        P = sc.problem(sc.case(name), a["double"])
        dev = _api().to_device(P)
        g = _solver(P, TV_T, "GN", {})
        v = torch.from_numpy(sc.probe_direction(g.n).astype(np.float64 if P.double else np.float32)).cuda()
        r, diag = g.eval_jtf(dev)
        o, dot = g.apply_jtj(dev, v)
        out[name] = {"n": g.n, "cost": g.eval_cost(dev), "r": _np(r), "diag": _np(diag), "out": _np(o), "dot": dot}
        g.close()
    return out


def _problem(r):
    if r.get("energy", "tv") == "tv":
        return sc.problem(sc.case(r["case"]), r["double"]), TV_T
    P = BUILTINS[r["energy"]](r["double"])
    return P, _api().energy_file(P.energy)


def _run(r):
    """Init + Step by Step: return values, costs (after init and every step), the LM radius after every step, describe() before and after, the status, the unknowns,
    and the PCG trace rows if asked for."""
    api = _api()
    P, t = _problem(r)
    kind = r["kind"]
    g = _solver(P, t, kind, dict(nIterations=r["nsteps"], lIterations=r["liters"], **r.get("params", {})))
    if r.get("trace"):
        g.enable_trace(True)
    dev = api.to_device(P)
    g.init(dev)
    rec = {"ret": [], "cost": [g.cost()], "radius": [], "describe_before": g.describe()}
    while True:
        more = g.step(dev)
        rec["ret"].append(int(more)); rec["cost"].append(g.cost()); rec["radius"].append(g.trust_region_radius() if kind == "LM" else 0.0)
        if not more:
            break
    rec["describe"] = g.describe(); rec["status"] = g.on_chip_status()
    if r.get("trace"):
        rec["trace"] = g.trace().tolist()
    rec["x"] = np.concatenate([dev[i].reshape(-1).cpu().numpy().astype(np.float64) for i in P.unknown_slots]).tolist()
    g.close()
    return rec


def case_solves(a):
    """a["runs"]: [{name, energy, case, double, kind, nsteps, liters, params, trace}] run one after the other in this process."""
    _load(a)
    out = {r["name"]: _run(r) for r in a["runs"]}
    out["names"] = _api().registered_energies()
    return out


def case_apply_bits(a):
    """One Gauss-Newton step of a["liters"] iterations under amd_stencil_fused = 1 on every named case; then the vectors p and A p the LAST two-launch iteration left in
    the solver's buffers, and OptAmd_ApplyJTJ of that very p on a fresh upload of the inputs (the step has moved the unknowns; the probe must linearise where the
    step did)."""
    _load(a)
    api = _api()
    out = {}
    for name in a["cases"]:
        P = sc.problem(sc.case(name), a["double"])
        g = _solver(P, TV_T, "GN", dict(nIterations=1, lIterations=a["liters"], amd_stencil_fused=1))
        dev = api.to_device(P)
        g.init(dev)
        d = g.describe()
        g.step(dev)
        p, Ap = g.vector("p"), g.vector("Ap_X")
        o, _ = g.apply_jtj(api.to_device(P), p.clone())
        out[name] = {"describe": d, "p": _np(p), "Ap": _np(Ap), "probe": _np(o)}
        g.close()
    return out


if __name__ == "__main__":
    case, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    result = globals()["case_" + case](args)
    sys.stdout.flush()
    print(json.dumps(result))
