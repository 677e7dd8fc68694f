#!/usr/bin/env python
"""The energies on the functor stencil engine (opt_amd/csrc/stencil_engine.h): the reference's three launches per PCG iteration (amd_stencil_fused = 0: PCGStep1 by
se_gather, PCGStep2, PCGStep3) against the two-launch iteration (amd_stencil_fused = 1: ge_flatStep / ge_flatStepNoPre + se_gatherIter).  The protocol of
tools/bench_graph_fused.py: whole solves (Opt_ProblemSolve, inputs resident, wall time between two device synchronisations), both settings in one process,
alternating, median and minimum of --solves (5); us per PCG iteration = median solve / (steps x lIterations).  LM rows run with q_tolerance = -1e9 (no early-out: both
settings do the same number of iterations) and residual_reset_period = 10.

Workloads, two sizes each -- one small enough to be launch-bound, one of at least 1024 x 1024 pixels / 64^3 voxels: the sample plug-in
(examples/plugins/vector_tv_denoising, preconditioned), optical_flow under Levenberg-Marquardt kept off the chip (amd_onchip = 0: unpreconditioned, ge_flatStepNoPre) and
volumetric_mesh_deformation on the functor engine (OPT_AMD_VOLUMETRIC_ARAP=0: 3-D, preconditioned).  Every case runs in a child process of its own under a time limit;
the first case that fails ends the run.  "faster" holds for a row where the median under 1 is below the minimum under 0.  Writes <out>.json and <out>.md
(default profiles/stencil_fused).

    python tools/bench_stencil_fused.py                 # the table
    python tools/bench_stencil_fused.py --case 3        # one row, as JSON on stdout
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

GN, LM = "gaussNewtonGPU", "LMGPU"


def tv(n):
    from opt_amd import workloads as wl
    return wl.vector_tv_denoising(n, n, seed=1, mask="block")


def flow(n):
    from opt_amd import workloads as wl
    return wl.optical_flow(n, n, seed=2, init_flow=1.2)


def vol(n):
    from opt_amd import workloads as wl
    return wl.volumetric_mesh_deformation(n, n, n, seed=5, perturb=0.05)


# (name, problem, solver kind, steps, lIterations, extra plan parameters, environment of the case, time limit of the case in seconds)
WORKLOADS = [
    ("vector_tv_denoising (plug-in), 64 x 64", lambda: tv(64), GN, 5, 50, {}, {}, 120),
    ("vector_tv_denoising (plug-in), 1024 x 1024", lambda: tv(1024), GN, 3, 30, {}, {}, 240),
    ("vector_tv_denoising (plug-in), 64 x 64", lambda: tv(64), LM, 5, 50, {}, {}, 120),
    ("vector_tv_denoising (plug-in), 1024 x 1024", lambda: tv(1024), LM, 3, 30, {}, {}, 240),
    ("optical_flow, 64 x 64, amd_onchip=0", lambda: flow(64), LM, 5, 50, {"amd_onchip": 0}, {}, 120),
    ("optical_flow, 1024 x 1024, amd_onchip=0", lambda: flow(1024), LM, 3, 30, {"amd_onchip": 0}, {}, 240),
    ("volumetric_mesh_deformation, 8^3, functor engine", lambda: vol(8), GN, 5, 50, {}, {"OPT_AMD_VOLUMETRIC_ARAP": "0"}, 120),
    ("volumetric_mesh_deformation, 64^3, functor engine", lambda: vol(64), GN, 3, 30, {}, {"OPT_AMD_VOLUMETRIC_ARAP": "0"}, 240),
]


def t_file(P):
    from opt_amd import api, build, workloads as wl
    if P.energy == "vector_tv_denoising":
        lib = build.plugin_path("vector_tv_denoising")
        if not os.path.exists(lib):
            build.build_plugin(build.SAMPLE_STENCIL_PLUGIN)
        if P.energy not in api.registered_energies():
            api.load_energy_plugin(lib)
        return wl.VECTOR_TV_T
    return api.energy_file(P.energy)


def plan(P, kind, steps, liters, extra, fused):
    from opt_amd import api
    g = api.Solver(t_file(P), kind, P.dims, double=P.double, timing=False)
    for k, v in (("nIterations", steps), ("lIterations", liters), ("q_tolerance", -1e9), ("residual_reset_period", 10), ("amd_stencil_fused", fused), *extra.items()):
        g.set_parameter(k, v)
    return g


def measure(P, kind, steps, liters, extra, solves):
    import torch
    from opt_amd import api
    settings = (0, 1)
    dev = api.to_device(P)
    x0 = [dev[i].clone() for i in P.unknown_slots]
    plans = {s: plan(P, kind, steps, liters, extra, s) for s in settings}
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
        solve(s)                      # warm-up (allocations, first touch)
    for _ in range(solves):
        for s in settings:
            times[s].append(solve(s))
    out = {}
    for s in settings:
        t = times[s]
        d = plans[s].describe()
        out[f"amd_stencil_fused={s}"] = {"launches_per_iteration": d.get("launches_per_iteration", "3"), "kernels": d.get("kernels"), "why_not_fused": d.get("why_not_fused"), "path": d.get("path"),
                                         "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                                         "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
        plans[s].close()
    return out


def run_case(i, solves):
    name, make, kind, steps, liters, extra, _, _ = WORKLOADS[i]
    P = make()
    elements = 1
    for d in P.dims:
        elements *= int(d)
    row = {"workload": name, "elements": elements, "precision": "double" if P.double else "float", "solver": "LM" if kind == LM else "GN", "steps": steps, "lIterations": liters}
    row.update(measure(P, kind, steps, liters, extra, solves))
    a, b = row["amd_stencil_fused=0"], row["amd_stencil_fused=1"]
    row["taken"] = b["launches_per_iteration"] == "2" and "on-chip" not in (b["path"] or "")
    row["faster"] = bool(row["taken"] and b["median_ms"] < a["min_ms"])
    row["speedup_of_medians"] = a["median_ms"] / b["median_ms"]
    return row


def markdown(res):
    L = ["# amd_stencil_fused: two launches per PCG iteration for the functor stencil engine", "",
         f"Device: {res['device']}.  Whole solves (Opt_ProblemSolve), `amd_stencil_fused=0` and `=1` alternating in one process, median / minimum of {res['solves_per_setting']};",
         "us per PCG iteration = median solve / (steps x lIterations).  LM rows: q_tolerance = -1e9, residual_reset_period = 10.  Written by tools/bench_stencil_fused.py.",
         "`faster`: the median under 1 is below the minimum under 0.", "",
         "| workload | pixels / voxels | solver | steps x iterations | =0 median ms (min) | =0 us / iteration | =1 median ms (min) | =1 us / iteration | medians 0 / 1 | faster |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["workloads"]:
        a, b = r["amd_stencil_fused=0"], r["amd_stencil_fused=1"]
        L.append(f"| {r['workload']} | {r['elements']} | {r['precision']} {r['solver']} | {r['steps']} x {r['lIterations']} | {a['median_ms']:.2f} ({a['min_ms']:.2f}) | {a['us_per_pcg_iteration']:.1f} | "
                 f"{b['median_ms']:.2f} ({b['min_ms']:.2f}) | {b['us_per_pcg_iteration']:.1f} | {r['speedup_of_medians']:.2f} | {'yes' if r['faster'] else 'no'} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stencil_fused"))
    a = ap.parse_args()
    if a.case is not None:
        print("ROW " + json.dumps(run_case(a.case, a.solves)), flush=True)
        return 0
    import torch
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": []}
    for i, w in enumerate(WORKLOADS):      # one child per case, each under its own time limit and environment; nothing more is started once one has failed
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i), "--solves", str(a.solves)], capture_output=True, text=True, timeout=w[7], env={**os.environ, **w[6]})
        except subprocess.TimeoutExpired:
            print(f"case {i} ({w[0]}) ran into its time limit of {w[7]} s: stopping")
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
