#!/usr/bin/env python
"""The functor mesh energies (cotangent_mesh_smoothing, embedded_mesh_deformation, robust_nonrigid_alignment): the reference-order loop on the record kernels
(amd_graph_fused = 0: PCGStep3, PCGStep1_Graph, PCGStep1, PCGStep2 per PCG iteration) against the two-launch iteration (amd_graph_fused = 1: ge_flatStep + ge_gather,
opt_amd/csrc/graph_engine.h).  Whole solves (Opt_ProblemSolve, inputs resident, wall time between two device synchronisations), both settings in one process,
alternating, median and minimum of --solves (5); us per PCG iteration = median solve / (steps x lIterations).  LM rows run with q_tolerance = -1e9 (no early-out: both
settings do the same number of iterations) and residual_reset_period = 10.

Workloads: the reference callers' flows on the reference-sized raptor mesh (2000 vertices, tests/fixtures/raptor2k_mesh.npz) and the armadillo's subdivision (386), and
the three 512 x 512 rows of tools/bench_configs.py.  Every case runs in a child process of its own under a time limit; the first case that fails ends the run.
"faster" holds for a row where the median under amd_graph_fused = 1 is below the minimum under amd_graph_fused = 0.  Writes profiles/graph_fused.json and .md.

    python tools/bench_graph_fused.py                 # the table
    python tools/bench_graph_fused.py --case 3        # one row, as JSON on stdout
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def mesh(energy, name):
    import graph_cases as gc
    return gc.base_problem(energy, name, False)


def grid(energy):
    from opt_amd import workloads as wl
    return {"cotangent": wl.cotangent_mesh_smoothing, "embedded": wl.embedded_mesh_deformation, "robust": wl.robust_nonrigid_alignment}[energy](512, 512)


GN, LM = "gaussNewtonGPU", "LMGPU"
# (name, problem, solver kind, steps, lIterations, time limit of the case in seconds)
WORKLOADS = [
    ("embedded, raptor (2000)", lambda: mesh("embedded", "raptor"), GN, 1, 1000, 120),
    ("embedded, raptor (2000)", lambda: mesh("embedded", "raptor"), GN, 5, 125, 120),
    ("robust, raptor (2000)", lambda: mesh("robust", "raptor"), GN, 10, 250, 120),
    ("cotangent, armadillo subdivided (386)", lambda: mesh("cotangent", "armadillo_sub"), GN, 5, 25, 120),
    ("cotangent, raptor (2000)", lambda: mesh("cotangent", "raptor"), GN, 5, 25, 120),
    ("embedded, raptor (2000)", lambda: mesh("embedded", "raptor"), LM, 5, 125, 120),
    ("robust, raptor (2000)", lambda: mesh("robust", "raptor"), LM, 10, 250, 120),
    ("cotangent, raptor (2000)", lambda: mesh("cotangent", "raptor"), LM, 5, 25, 120),
    ("cotangent, 512 x 512 torus", lambda: grid("cotangent"), GN, 5, 25, 240),
    ("embedded, 512 x 512", lambda: grid("embedded"), GN, 5, 125, 240),
    ("robust, 512 x 512", lambda: grid("robust"), GN, 5, 50, 240),
]


def plan(P, kind, steps, liters, fused):
    from opt_amd import api
    g = api.Solver(api.energy_file(P.energy), kind, P.dims, double=P.double, timing=False)
    for k, v in (("nIterations", steps), ("lIterations", liters), ("q_tolerance", -1e9), ("residual_reset_period", 10), ("amd_graph_fused", fused)):
        g.set_parameter(k, v)
    return g


def measure(P, kind, steps, liters, solves):
    import torch
    from opt_amd import api
    settings = (0, 1)
    dev = api.to_device(P)
    x0 = [dev[i].clone() for i in P.unknown_slots]
    plans = {s: plan(P, kind, steps, liters, s) for s in settings}
    times, costs = {s: [] for s in settings}, {}

    def solve(s):
        for i, x in zip(P.unknown_slots, x0):
            dev[i].copy_(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[s].solve(dev)
        torch.cuda.synchronize()
        costs[s] = plans[s].cost()
        return time.perf_counter() - t0

    for s in settings:
        solve(s)                      # warm-up (allocations, the incidence lists, first touch)
    for _ in range(solves):
        for s in settings:
            times[s].append(solve(s))
    out = {}
    for s in settings:
        t = times[s]
        d = plans[s].describe()
        out[f"amd_graph_fused={s}"] = {"launches_per_iteration": d.get("launches_per_iteration", "4"), "kernels": d.get("kernels"), "why_not_fused": d.get("why_not_fused"),
                                       "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                                       "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
        plans[s].close()
    return out


def run_case(i, solves):
    name, make, kind, steps, liters, _ = WORKLOADS[i]
    P = make()
    row = {"workload": name, "vertices": int(P.dims[0]), "precision": "double" if P.double else "float", "solver": "LM" if kind == LM else "GN", "steps": steps, "lIterations": liters}
    row.update(measure(P, kind, steps, liters, solves))
    a, b = row["amd_graph_fused=0"], row["amd_graph_fused=1"]
    row["taken"] = b["launches_per_iteration"] == "2"
    row["faster"] = bool(row["taken"] and b["median_ms"] < a["min_ms"])
    row["speedup_of_medians"] = a["median_ms"] / b["median_ms"]
    return row


def markdown(res):
    L = ["# amd_graph_fused: two launches per PCG iteration for the functor mesh energies", "",
         f"Device: {res['device']}.  Whole solves (Opt_ProblemSolve), `amd_graph_fused=0` and `=1` alternating in one process, median / minimum of {res['solves_per_setting']};",
         "us per PCG iteration = median solve / (steps x lIterations).  LM rows: q_tolerance = -1e9, residual_reset_period = 10.  Written by tools/bench_graph_fused.py.",
         "`faster`: the median under 1 is below the minimum under 0.", "",
         "| workload | vertices | solver | steps x iterations | =0 median ms (min) | =0 us / iteration | =1 median ms (min) | =1 us / iteration | medians 0 / 1 | faster |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["workloads"]:
        a, b = r["amd_graph_fused=0"], r["amd_graph_fused=1"]
        L.append(f"| {r['workload']} | {r['vertices']} | {r['precision']} {r['solver']} | {r['steps']} x {r['lIterations']} | {a['median_ms']:.2f} ({a['min_ms']:.2f}) | {a['us_per_pcg_iteration']:.1f} | "
                 f"{b['median_ms']:.2f} ({b['min_ms']:.2f}) | {b['us_per_pcg_iteration']:.1f} | {r['speedup_of_medians']:.2f} | {'yes' if r['faster'] else 'no'} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_fused"))
    a = ap.parse_args()
    if a.case is not None:
        print("ROW " + json.dumps(run_case(a.case, a.solves)), flush=True)
        return 0
    import torch
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": []}
    for i, w in enumerate(WORKLOADS):      # one child per case, each under its own time limit; nothing more is started once one has failed
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i), "--solves", str(a.solves)], capture_output=True, text=True, timeout=w[5])
        except subprocess.TimeoutExpired:
            print(f"case {i} ({w[0]}) ran into its time limit of {w[5]} s: stopping")
            return 1
        rows = [l[4:] for l in p.stdout.splitlines() if l.startswith("ROW ")]
        if p.returncode != 0 or not rows:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            print(f"case {i} ({w[0]}) ended with status {p.returncode}: stopping")
            return 1
        res["workloads"].append(json.loads(rows[0]))
        print(rows[0], flush=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(a.out + ".md", "w") as f:
        f.write(markdown(res))
    print(markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
