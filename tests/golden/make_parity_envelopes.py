#!/usr/bin/env python
"""How far apart do LEGAL runs of the reference's arithmetic end on the cases whose parity bar sits above the contract (1e-12 double, 1e-5 float)?

A bar above the contract used to be 10 x the error this library itself produced on one GPU run.  It is now a measured yardstick, like tests/test_horizon_gpu.py's and
float_envelopes.json's: twice the diameter of a frozen ensemble of legal oracle runs of the same case (tests/helpers.py::assert_close applies the rule).  The ensemble is
fixed before any HIP number is looked at and is the same for every case:

    {plain, fma build of the oracle (oracle/Makefile)} x {exact-order sums, the reference's own reduction order under seeds 1 .. 16 (set_reduction(1, seed))}  = 34 runs

each with the thread count the test gives the oracle.  The cases come from tests/parity_cases.py -- the functions the tests themselves call.

Output:
  tests/golden/parity_envelopes.json      what a bar is computed from
    meta   the ensemble's labels in run order (run 0 is exact-order plain: what a test's oracle computes), host seconds, the rule
    cases  {key: {checksum of the inputs, double, kind, costs[step] / radius[step] (LM) of run 0 (step 0 = after init), costs_spread[step] / radius_spread[step] = max - min
           over the 34 runs, x_diameter = the largest |x_p - x_q| / |x_0| of two runs' final unknowns, row}}
  tests/golden/envelopes/parity_envelope_runs.npz   every run behind it: costs_<row>[run][step], radius_<row>[run][step] as deviations from run 0, x_dist_<row>[run] = |x_run - x_0| / |x_0|
CPU only; both builds run in subprocesses (the binding loads one library per process), several at a time.

    python tests/golden/make_parity_envelopes.py [--jobs N]
"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "parity_envelopes.json")
RUNS = os.path.join(HERE, "envelopes", "parity_envelope_runs.npz")      # (a directory of its own: tests/test_golden.py takes every tests/golden/*.npz for a problem)
VARIANTS = ("plain", "fma")
SEEDS = list(range(1, 17))
LABELS = [("exact-order " if s == 0 else f"reference-order seed {s} ") + v for v in VARIANTS for s in [0] + SEEDS]
RULE = "bar in force = min(bar of the table, max(contract, 2 x diameter at the same step and quantity, over the denominator the assertion uses))"


def run_case(ob, case, seed):
    """One oracle run of a case, stepped as the tests step it: (costs per step, radii per step or None, final unknowns)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import flat_unknowns
    P = case.problem()
    o = ob.OracleSolver(P.energy, case.kind, P.double, P.dims)
    for k, v in case.settings().items():
        o.set(k, v)
    o.set_threads(case.threads)
    if seed:
        o.set_reduction(1, seed)
    lm = case.kind == "LMGPU"
    o.init(P.params)
    costs, radii = [o.cost()], [o.trust_region_radius() if lm else 0.0]
    while True:
        more = o.step(P.params)
        costs.append(o.cost()); radii.append(o.trust_region_radius() if lm else 0.0)
        if not more:
            break
    x = flat_unknowns(P)
    o.close()
    return costs, (radii if lm else None), x


def worker(tmp, shard, nshards, only=None):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle.binding as ob
    import parity_cases as pc
    variant = os.environ.get("OPT_ORACLE_VARIANT", "plain")
    cases = pc.envelope_cases()
    keys = sorted(k for k in cases if only is None or k in only)[shard::nshards]
    out = {}
    for i, key in enumerate(keys):
        case = cases[key]
        runs, xs = [], {}
        for seed in [0] + SEEDS:
            c, r, x = run_case(ob, case, seed)
            runs.append({"costs": c, "radius": r}); xs[f"s{seed}"] = x
        np.savez(os.path.join(tmp, f"x_{variant}_{shard}_{i}.npz"), **xs)
        out[key] = {"runs": runs, "x": f"x_{variant}_{shard}_{i}.npz", "checksum": case.checksum(), "double": bool(case.problem().double)}
    json.dump(out, open(os.path.join(tmp, f"part_{variant}_{shard}.json"), "w"))


def write(meta, cases, runs):
    """the summary a bar is computed from (JSON, one line per case) and every run behind it (npz: deviations from run 0 in float32)"""
    import numpy as np
    with open(OUT, "w") as f:
        f.write('{"meta": ' + json.dumps(meta, sort_keys=True) + ',\n"cases": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, sort_keys=True, separators=(",", ":")) for k, v in sorted(cases.items())))
        f.write("\n}}\n")
    os.makedirs(os.path.dirname(RUNS), exist_ok=True)
    np.savez_compressed(RUNS, **runs)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), set(json.load(open(os.path.join(sys.argv[2], "only.json")))))
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else max(1, min(8, os.cpu_count() or 1))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import parity_cases as pc
    t0 = time.time()
    for variant in VARIANTS:      # build both libraries before the workers race for them
        env = dict(os.environ, OPT_ORACLE_VARIANT=variant)
        subprocess.check_call([sys.executable, "-c", "import oracle.binding as b; b.build()"], env=env, cwd=ROOT)
    nshards = max(1, jobs)
    with tempfile.TemporaryDirectory() as tmp:
        json.dump(sorted(pc.envelope_cases()), open(os.path.join(tmp, "only.json"), "w"))
        todo = [(v, s) for s in range(nshards) for v in VARIANTS]
        running = []
        while todo or running:
            while todo and len(running) < jobs:
                v, s = todo.pop(0)
                env = dict(os.environ, OPT_ORACLE_VARIANT=v)
                running.append((v, s, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tmp, str(s), str(nshards)], env=env, cwd=os.path.join(ROOT, "tests"))))
            for item in list(running):
                rc = item[2].poll()
                if rc is not None:
                    assert rc == 0, ("worker failed", item[0], item[1], rc)
                    running.remove(item)
            time.sleep(0.2)
        parts = {v: {} for v in VARIANTS}
        for v in VARIANTS:
            for s in range(nshards):
                parts[v].update(json.load(open(os.path.join(tmp, f"part_{v}_{s}.json"))))
        cases, runs = {}, {}
        for row, (key, case) in enumerate(sorted(pc.envelope_cases().items())):
            a, b = parts["plain"][key], parts["fma"][key]
            assert a["checksum"] == b["checksum"]
            xs = []
            for part in (a, b):
                z = np.load(os.path.join(tmp, part["x"]))
                xs += [np.asarray(z[f"s{s}"], dtype=np.float64) for s in [0] + SEEDS]
                os.remove(os.path.join(tmp, part["x"]))
            nrm = max(float(np.linalg.norm(xs[0])), 1e-300)
            diam = max(float(np.linalg.norm(xs[p] - xs[q])) for p in range(len(xs)) for q in range(p)) / nrm
            e = {"checksum": a["checksum"], "double": a["double"], "kind": case.kind, "row": row, "x_diameter": float("%.4g" % diam)}
            for q in ("costs", "radius"):
                if case.kind != "LMGPU" and q == "radius":
                    continue
                v = np.array([r[q] for r in a["runs"] + b["runs"]], dtype=np.float64)      # [run][step]
                e[q] = [float(c) for c in v[0]]
                e[q + "_spread"] = [float("%.4g" % c) for c in v.max(0) - v.min(0)]
                runs[f"{q}_{row}"] = (v - v[0]).astype(np.float32)
            runs[f"x_dist_{row}"] = np.array([float(np.linalg.norm(x - xs[0])) / nrm for x in xs], dtype=np.float32)
            cases[key] = e
    secs = time.time() - t0
    write({"ensemble": LABELS, "rule": RULE, "host_seconds": round(secs, 1), "jobs": jobs, "cases": len(cases), "runs": os.path.relpath(RUNS, HERE)}, cases, runs)
    print(f"{len(cases)} cases x {len(LABELS)} runs in {secs:.0f} s of host time ({jobs} processes); {os.path.getsize(OUT)} + {os.path.getsize(RUNS)} bytes")
    for k, e in sorted(cases.items()):
        print("  ", k, "cost diameter per step", ["%.1e" % (d / max(abs(c), 1e-300)) for d, c in zip(e["costs_spread"], e["costs"])], "x %.1e" % e["x_diameter"])


if __name__ == "__main__":
    main()
