"""Shared helpers of the parity tests: run the same problem through the CPU oracle and the HIP library."""
import numpy as np

from opt_amd import api


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = max(np.linalg.norm(b), 1e-300)
    return float(np.linalg.norm(a - b) / den)


def flat_unknowns(problem):
    return np.concatenate([np.asarray(problem.params[i]).reshape(-1) for i in problem.unknown_slots])


def oracle_solver(oracle_lib, problem, kind="gaussNewtonGPU", **params):
    s = oracle_lib.OracleSolver(problem.energy, kind, problem.double, problem.dims)
    for k, v in params.items():
        s.set(k, v)
    return s


def hip_solver(problem, kind="gaussNewtonGPU", timing=False, verbosity=0, **params):
    s = api.Solver(api.energy_file(problem.energy), kind, problem.dims, double=problem.double, verbosity=verbosity, timing=timing)
    for k, v in params.items():
        s.set_parameter(k, v)
    return s


def device_unknowns(problem, dev_params):
    import torch
    return torch.cat([dev_params[i].reshape(-1) for i in problem.unknown_slots]).cpu().numpy()


def active_mask(P):
    """Boolean mask over the flat unknown vector: rows of non-excluded unknowns."""
    if P.energy == "image_warping":
        m = np.asarray(P.params[4]).reshape(-1) == 0
        return np.concatenate([np.repeat(m, 2), m])
    if P.energy == "poisson_image_editing":
        return np.repeat(np.asarray(P.params[2]).reshape(-1) == 0, 4)
    if P.energy == "shape_from_shading":
        return np.asarray(P.params[17]).reshape(-1) > 0
    return np.ones(flat_unknowns(P).size, dtype=bool)


# ---- per-case parity bars ----------------------------------------------------------------------------------------
# north_star: 1e-5 (float) / 1e-12 (double).  A double trajectory of k PCG iterations does not hold 1e-12 everywhere -- the iteration amplifies last-bit
# differences of the sums -- so every test FUNCTION carries its own bar per quantity in tests/golden/parity_bars.json (tools/make_parity_bars.py builds the table from a
# logged run: OPT_PARITY_LOG=<file> python -m pytest tests -m gpu).  An entry is either the contract itself or, above it, names the frozen ensemble of LEGAL oracle runs of
# the same case (tests/golden/parity_envelopes.json: plain / fma build x exact-order sums / the reference's own sum order under 16 seeds; the cases are
# tests/parity_cases.py's) and the bar in force is
#       min(bar of the table, max(contract, 2 x diameter of the legal runs))
# with the diameter taken at the same step, for the same quantity, over the same denominator and floor as the assertion, relative to the exact-order plain run -- the
# project's rule for every yardstick above the contract (tests/test_horizon_gpu.py, float_envelopes.json).  No bar is derived from what the library itself produces.
# A function without an entry keeps the default the call site passes.
import json as _json
import os as _os

CONTRACT = {"double": 1e-12, "float": 1e-5}
ENVELOPE_FACTOR = 2.0
_BARS = None
_ENVELOPES = None


def _golden(name):
    p = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", name)
    return _json.load(open(p)) if _os.path.exists(p) else {}


def _bars():
    global _BARS
    if _BARS is None:
        _BARS = _golden("parity_bars.json")
    return _BARS


def envelopes():
    """{key: envelope} of tests/golden/parity_envelopes.json"""
    global _ENVELOPES
    if _ENVELOPES is None:
        _ENVELOPES = _golden("parity_envelopes.json").get("cases", {})
    return _ENVELOPES


def envelope_diameter(env, kind, step=None, floor=0.0):
    """Diameter of the legal runs of one envelope for the quantity an assertion checks: 'x' -- the largest relative distance of two runs' final unknowns; costs / 'radius' --
    (max - min over the runs at `step`) / max(|exact-order plain run at that step|, floor)."""      # (every run: tests/golden/envelopes/parity_envelope_runs.npz)
    if kind == "x":
        return env["x_diameter"]
    q = "radius" if kind == "radius" else "costs"
    if step is None:
        raise ValueError(f"a check of '{kind}' against an envelope needs its step")
    return env[q + "_spread"][step] / max(abs(env[q][step]), floor, 1e-300)


def envelope_name(entry, fn, par):
    """the envelope an entry of parity_bars.json names for the test `fn` ('tests/test_x.py::test_name') and parametrisation `par` ('[...]'), or None (an entry at the contract).
    A function-level entry covers many cases: it names tests/parity_cases.py::ENTRY_CASES, which gives the case -- hence the envelope -- of each parametrisation."""
    if "envelope" in entry:
        return entry["envelope"]
    if entry.get("envelopes") == "ENTRY_CASES":
        import parity_cases
        return parity_cases.ENTRY_CASES[fn + par].key
    return None


def bar_in_force(entry, fn, par, prec, kind, step=None, floor=0.0):
    name = envelope_name(entry, fn, par)
    if name is None:
        return entry["bar"]
    return min(entry["bar"], max(CONTRACT[prec], ENVELOPE_FACTOR * envelope_diameter(envelopes()[name], kind, step, floor)))


def _current_test():
    """('tests/test_x.py::test_name', '[params]') of the running test (pytest sets PYTEST_CURRENT_TEST)."""
    node = _os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    fn, _, par = node.partition("[")
    return fn, ("[" + par) if par else ""


def assert_close(kind, got, ref, default_tol, floor=0.0, absolute=False, double=None, step=None):
    """|got - ref| <= bar * max(|ref|, floor)   (absolute: got <= bar).  kind: 'cost0' (before any step), 'cost', 'cost_later', 'radius', 'x'.  The bar is the test function's
    entry in tests/golden/parity_bars.json (key '<file>::<function>|<double|float>|<kind>') if there is one, else default_tol; an entry above the contract is capped by twice the
    diameter of its envelope at `step` (bar_in_force).  With OPT_PARITY_LOG set, the measured relative error is appended to that file as one JSON line per check (the input of
    tools/make_parity_bars.py)."""
    fn, par = _current_test()
    prec = "double" if double else "float" if double is not None else "any"
    err = abs(got) if absolute else abs(got - ref) / max(abs(ref), floor, 1e-300)
    e = _bars().get(f"{fn}{par}|{prec}|{kind}") or _bars().get(f"{fn}|{prec}|{kind}")      # (a per-parametrisation entry wins: tests parametrised over ENERGIES)
    tol = bar_in_force(e, fn, par, prec, kind, step, floor) if e else default_tol
    log = _os.environ.get("OPT_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(_json.dumps({"test": fn, "params": par, "prec": prec, "kind": kind, "step": step, "err": err, "default": default_tol, "floor": floor, "bar": tol}) + "\n")
    assert err <= tol, (kind, step, got, ref, err, tol, "bar from parity_bars.json" if e else "default bar")
