"""Child-process body of the tests of generated energies (test_tgen_cpu.py, test_tgen_gpu.py).

The kernel registry of libOpt.so is process-global and other tests enumerate it, so nothing loads a plug-in inside the pytest process: every case runs here,
    python tests/tgen_driver.py <case> '<json arguments>'
and prints ONE line of JSON (floats by repr: they round-trip bit for bit).  The inputs come from tests/tgen_cases.py, which parent and child both import.

A `side` is {"name", "t"}: the .t file a solver is planned from.  The generated energy and a built-in comparator are two sides of one child (gen_<energy>.t resolves
to the plug-in, <energy>.t to the built-in kernel set); a hand-written plug-in of the same name as the generated one is the one side of a child of its own."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import tgen_cases as tc      # noqa: E402

KINDS = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}


def _api():
    from opt_amd import api
    return api


def _load(a):
    for p in a.get("plugins", []):
        _api().load_energy_plugin(p)


# ---- host-only cases -----------------------------------------------------------------------------------------------------------------------------------------
def case_check(a):
    """Load the libraries, then OptAmd_CheckProblemFile of every file of a["files"]: {key: path}."""
    api = _api()
    before = api.registered_energies()
    n = [api.load_energy_plugin(p) for p in a.get("plugins", [])]
    return {"n": n, "before": before, "names": api.registered_energies(), "check": {k: api.check_problem_file(p) for k, p in a["files"].items()},
            "hash": {k: "%016x" % api.problem_file_hash(p) for k, p in a["files"].items()}}


# ---- GPU cases -------------------------------------------------------------------------------------------------------------------------------------------------
def _solver(P, t_file, kind, params):
    g = _api().Solver(t_file, KINDS[kind], P.dims, double=P.double)
    for k, v in params.items():
        g.set_parameter(k, v)
    return g


def _np(t):
    return t.cpu().numpy().astype(np.float64).tolist()


def _probe(P, t_file):
    import torch
    dev = _api().to_device(P)
    g = _solver(P, t_file, "GN", {})
    v = torch.from_numpy(tc.probe_direction(g.n).astype(np.float64 if P.double else np.float32)).cuda()
    r, diag = g.eval_jtf(dev)
    o, dot = g.apply_jtj(dev, v)
    rec = {"n": g.n, "cost": g.eval_cost(dev), "r": _np(r), "diag": _np(diag), "out": _np(o), "dot": dot}
    g.close()
    return rec


def case_probes(a):
    """EvalCost, EvalJTF with the diagonal and ApplyJTJ (the vector and the returned scalar) of every side on every input of the energy, on the same arrays."""
    _load(a)
    out = {}
    for inp in a["inputs"]:
        P = tc.problem(a["energy"], inp, a["double"])
        out[inp] = {s["name"]: _probe(P, s["t"]) for s in a["sides"]}
    return out


def _run(P, t_file, kind, nsteps, liters, params):
    """Init + Step by Step: return values, costs (after init and every step), the LM radius after every step, describe() before and after, the status, the unknowns."""
    api = _api()
    g = _solver(P, t_file, kind, dict(nIterations=nsteps, lIterations=liters, **params))
    dev = api.to_device(P)
    g.init(dev)
    rec = {"ret": [], "cost": [g.cost()], "radius": [], "describe_before": g.describe()}
    while True:
        more = g.step(dev)
        rec["ret"].append(int(more)); rec["cost"].append(g.cost()); rec["radius"].append(g.trust_region_radius() if kind == "LM" else 0.0)
        if not more:
            break
    rec["describe"] = g.describe(); rec["status"] = g.on_chip_status()
    rec["x"] = np.concatenate([dev[i].reshape(-1).cpu().numpy().astype(np.float64) for i in P.unknown_slots]).tolist()
    g.close()
    return rec


def case_solves(a):
    """a["runs"]: [{name, side, energy, input, double, kind, nsteps, liters, params}] one after the other in this process; a["sides"]: {side name: .t path}."""
    _load(a)
    out = {}
    for r in a["runs"]:
        P = tc.problem(r["energy"], r["input"], r["double"])
        out[r["name"]] = _run(P, a["sides"][r["side"]], r["kind"], r["nsteps"], r["liters"], r.get("params", {}))
    out["names"] = _api().registered_energies()
    return out


def case_round_trip(a):
    """api.compile_and_load_energy on a .t nobody wrote a functor for; probes in double; then Opt_ProblemSolve through the unmodified API (GN 3 x 10, double)."""
    api = _api()
    before = api.registered_energies()
    lib = api.compile_and_load_energy(a["t"], force=False)
    P = tc.round_trip_problem(True)
    out = {"lib": lib, "before": before, "names": api.registered_energies(), "check": api.check_problem_file(a["t"]), "probe": _probe(P, a["t"])}
    g = _solver(P, a["t"], "GN", dict(nIterations=3, lIterations=10))
    dev = api.to_device(P)
    out["cost_before"] = g.eval_cost(dev)
    g.solve(dev)
    out["cost_after"] = g.cost()
    out["describe"] = g.describe()
    out["x"] = _np(dev[0].reshape(-1))
    g.close()
    return out


if __name__ == "__main__":
    case, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    result = globals()["case_" + case](args)
    sys.stdout.flush()
    print(json.dumps(result))
