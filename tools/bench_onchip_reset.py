"""Levenberg-Marquardt solves whose linear solve passes residual resets (lIterations > residual_reset_period = 10): the launch-per-iteration loop (amd_onchip = 1, the
default) against the on-chip solve with the resets inside, in ONE process, inputs resident, one warm-up solve per plan, then the timed solves alternating between the two
settings.  q_tolerance = -1e9: both settings run the same iterations.

    python tools/bench_onchip_reset.py [--set stencil|sfs] [--solves 5] [--out profiles/<set's file>.json]

Workload sets:
  stencil  amd_onchip 1 -> 2 (march_onchipPcg<.., 2>, opt_amd/csrc/stencil_onchip.h): poisson_image_editing 256^2 and 512^2 float, 1 step x 100 iterations (the reference
           example's linearIter); optical_flow 512^2 float, 3 x 50 (likewise).  -> profiles/onchip_reset.json
  sfs      amd_onchip 1 -> 3 (sfs_onchipPcg<.., 2, ..>, opt_amd/csrc/sfs_onchip.h): shape_from_shading 640 x 480 (the reference's input) double and float, 1024^2 double, 10 x 25;
           and a control -- 640 x 480 double, 10 x 10: no reset falls inside the solve, both settings take the same kernel, so the row must show no difference (reported,
           not part of the criterion).  -> profiles/onchip_sfs_reset.json
Where no variant with the reset on chip fits the asked image the largest smaller one (both sides in steps of 64) that does is taken, and the output says so.
Pass criterion (printed, and the exit status): for every workload the median under the new setting is below the minimum under amd_onchip = 1.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# (energy, width, height, double, steps, lIterations, control)
SETS = {
    "stencil": {"settings": (1, 2), "out": "onchip_reset.json",
                "workloads": [("poisson_image_editing", 256, 256, False, 1, 100, False), ("poisson_image_editing", 512, 512, False, 1, 100, False), ("optical_flow", 512, 512, False, 3, 50, False)]},
    "sfs": {"settings": (1, 3), "out": "onchip_sfs_reset.json",
            "workloads": [("shape_from_shading", 640, 480, True, 10, 25, False), ("shape_from_shading", 640, 480, False, 10, 25, False), ("shape_from_shading", 1024, 1024, True, 10, 25, False),
                          ("shape_from_shading", 640, 480, True, 10, 10, True)]},
}


def make(energy, W, H, double):
    from opt_amd import workloads as wl
    if energy == "poisson_image_editing":
        return wl.poisson_image_editing(W, H, double=double, seed=1)
    if energy == "optical_flow":
        return wl.optical_flow(W, H, double=double, seed=1, init_flow=1.2)
    return wl.shape_from_shading(W, H, double=double, seed=1, holes=True)


def plan(P, steps, liters, onchip):
    from opt_amd import api
    g = api.Solver(api.energy_file(P.energy), "LMGPU", P.dims, double=P.double, timing=False)
    for k, v in (("nIterations", steps), ("lIterations", liters), ("q_tolerance", -1e9), ("amd_onchip", onchip)):
        g.set_parameter(k, v)
    return g


def main():
    import torch
    from opt_amd import api
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default="stencil")
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    base, new = SETS[a.set]["settings"]
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", SETS[a.set]["out"])
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": []}
    ok = True
    for energy, askedW, askedH, double, steps, liters, control in SETS[a.set]["workloads"]:
        W, H = askedW, askedH
        while not control and min(W, H) > 64:      # the largest image a variant with the reset on chip fits
            g = plan(make(energy, W, H, double), steps, liters, new)
            fits = "on-chip" in g.describe()["path"]
            g.close()
            if fits:
                break
            W -= 64; H -= 64
        P = make(energy, W, H, double)
        dev = api.to_device(P)
        x0 = [dev[i].clone() for i in P.unknown_slots]
        plans = {s: plan(P, steps, liters, s) for s in (base, new)}
        paths = {s: plans[s].describe()["path"] for s in (base, new)}
        times, costs = {base: [], new: []}, {}

        def solve(s):
            for i, x in zip(P.unknown_slots, x0):
                dev[i].copy_(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plans[s].solve(dev)
            torch.cuda.synchronize()
            costs[s] = plans[s].cost()
            return time.perf_counter() - t0

        for s in (base, new):
            solve(s)                      # warm-up (allocations, first-touch, the coefficient buffers)
        for _ in range(a.solves):
            for s in (base, new):
                times[s].append(solve(s))
        row = {"energy": energy, "asked": f"{askedW}x{askedH}", "image": f"{W}x{H}", "precision": "double" if double else "float", "solver": "LM", "steps": steps, "lIterations": liters,
               "residual_reset_period": 10, "note": None if (W, H) == (askedW, askedH) else f"no variant with the reset on chip fits {askedW}x{askedH}; the largest image that does"}
        if control:
            row["control"] = "no reset falls inside the solve: both settings take the same kernel"
        for s in (base, new):
            t = times[s]
            row[f"amd_onchip={s}"] = {"path": paths[s], "on_chip_status": plans[s].on_chip_status(), "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                                      "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
            plans[s].close()
        if not control:
            row["pass"] = bool(row[f"amd_onchip={new}"]["median_ms"] < row[f"amd_onchip={base}"]["min_ms"] and "on-chip" in paths[new] and row[f"amd_onchip={new}"]["on_chip_status"] == 1)
            ok = ok and row["pass"]
        res["workloads"].append(row)
        print(json.dumps(row), flush=True)
    res["pass"] = ok
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("PASS" if ok else f"FAIL: the median under amd_onchip={new} is not below the minimum under amd_onchip={base} everywhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
