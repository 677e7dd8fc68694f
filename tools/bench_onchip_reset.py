"""Levenberg-Marquardt solves of the 5-point-stencil energies whose linear solve passes residual resets (lIterations > residual_reset_period = 10): the launch-per-iteration
loop (amd_onchip = 1, the default) against the on-chip solve with the resets inside (amd_onchip = 2: march_onchipPcg<.., 2>, opt_amd/csrc/stencil_onchip.h) in ONE process,
inputs resident, one warm-up solve per plan, then the timed solves alternating between the two settings.  q_tolerance = -1e9: both settings run the same iterations.

    python tools/bench_onchip_reset.py [--solves 5] [--out profiles/onchip_reset.json]

Workloads: poisson_image_editing 256^2 and 512^2 float, 1 step x 100 iterations (the reference example's linearIter); optical_flow 512^2 float, 3 x 50 (likewise).
Where no variant with the reset on chip fits the asked square the largest smaller square (steps of 64) that does is taken, and the output says so.
Pass criterion (printed, and the exit status): for every workload the median under amd_onchip = 2 is below the minimum under amd_onchip = 1.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORKLOADS = [("poisson_image_editing", 256, 1, 100), ("poisson_image_editing", 512, 1, 100), ("optical_flow", 512, 3, 50)]


def make(energy, n):
    from opt_amd import workloads as wl
    return wl.poisson_image_editing(n, n, double=False, seed=1) if energy == "poisson_image_editing" else wl.optical_flow(n, n, double=False, seed=1, init_flow=1.2)


def plan(P, steps, liters, onchip):
    from opt_amd import api
    g = api.Solver(api.energy_file(P.energy), "LMGPU", P.dims, double=False, timing=False)
    for k, v in (("nIterations", steps), ("lIterations", liters), ("q_tolerance", -1e9), ("amd_onchip", onchip)):
        g.set_parameter(k, v)
    return g


def main():
    import torch
    from opt_amd import api
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "onchip_reset.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": []}
    ok = True
    for energy, asked, steps, liters in WORKLOADS:
        n = asked
        while n > 64:      # the largest square a variant with the reset on chip fits
            g = plan(make(energy, n), steps, liters, 2)
            fits = "on-chip" in g.describe()["path"]
            g.close()
            if fits:
                break
            n -= 64
        P = make(energy, n)
        dev = api.to_device(P)
        x0 = [dev[i].clone() for i in P.unknown_slots]
        plans = {s: plan(P, steps, liters, s) for s in (1, 2)}
        paths = {s: plans[s].describe()["path"] for s in (1, 2)}
        times, costs = {1: [], 2: []}, {}

        def solve(s):
            for i, x in zip(P.unknown_slots, x0):
                dev[i].copy_(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plans[s].solve(dev)
            torch.cuda.synchronize()
            costs[s] = plans[s].cost()
            return time.perf_counter() - t0

        for s in (1, 2):
            solve(s)                      # warm-up (allocations, first-touch, the coefficient buffers)
        for _ in range(a.solves):
            for s in (1, 2):
                times[s].append(solve(s))
        row = {"energy": energy, "asked": f"{asked}x{asked}", "image": f"{n}x{n}", "precision": "float", "solver": "LM", "steps": steps, "lIterations": liters, "residual_reset_period": 10,
               "note": None if n == asked else f"no variant with the reset on chip fits {asked}x{asked}; the largest square that does"}
        for s in (1, 2):
            t = times[s]
            row[f"amd_onchip={s}"] = {"path": paths[s], "on_chip_status": plans[s].on_chip_status(), "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                                      "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
            plans[s].close()
        row["pass"] = bool(row["amd_onchip=2"]["median_ms"] < row["amd_onchip=1"]["min_ms"] and "on-chip" in paths[2] and row["amd_onchip=2"]["on_chip_status"] == 1)
        ok = ok and row["pass"]
        res["workloads"].append(row)
        print(json.dumps(row), flush=True)
    res["pass"] = ok
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("PASS" if ok else "FAIL: the median under amd_onchip=2 is not below the minimum under amd_onchip=1 everywhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
