"""Levenberg-Marquardt solves whose linear solve passes residual resets (lIterations > residual_reset_period = 10): the launch-per-iteration loop (amd_onchip = 1, the
default) against the on-chip solve with the resets inside, in ONE process, inputs resident, one warm-up solve per plan, then the timed solves alternating between the two
settings.  q_tolerance = -1e9: both settings run the same iterations.

    python tools/bench_onchip_reset.py [--set stencil|sfs|general] [--solves 5] [--out profiles/<set's file>.json]

Workload sets:
  stencil  amd_onchip 1 -> 2 (march_onchipPcg<.., 2>, opt_amd/csrc/stencil_onchip.h): poisson_image_editing 256^2 and 512^2 float, 1 step x 100 iterations (the reference
           example's linearIter); optical_flow 512^2 float, 3 x 50 (likewise).  -> profiles/onchip_reset.json
  sfs      amd_onchip 1 -> 3 (sfs_onchipPcg<.., 2, ..>, opt_amd/csrc/sfs_onchip.h): shape_from_shading 640 x 480 (the reference's input) double and float, 1024^2 double, 10 x 25;
           and a control -- 640 x 480 double, 10 x 10: no reset falls inside the solve, both settings take the same kernel, so the row must show no difference (reported,
           not part of the criterion).  -> profiles/onchip_sfs_reset.json
  general  amd_onchip 1 -> 4 (iw_onchipPcgGeneral, opt_amd/csrc/iw_onchip.h): image_warping with a UrShape that is not the unit lattice (jitter_urshape = 0.2), under 1 the
           streaming general loop, under 4 the on-chip solve: float 512^2 and 640 x 480, Gauss-Newton 8 x 400 and LM 8 x 400 (the example's shape), and 512^2 double Gauss-Newton;
           and a control -- 512^2 float Gauss-Newton on the unit lattice: both settings take the lattice on-chip kernel.  -> profiles/onchip_general.json
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

# (energy, width, height, double, steps, lIterations, control[, solver kind (default LMGPU)])
SETS = {
    "general": {"settings": (1, 4), "out": "onchip_general.json", "fits_key": "general_urshape",
                "workloads": [("image_warping", 512, 512, False, 8, 400, False, "gaussNewtonGPU"), ("image_warping", 640, 480, False, 8, 400, False, "gaussNewtonGPU"),
                              ("image_warping", 512, 512, False, 8, 400, False, "LMGPU"), ("image_warping", 640, 480, False, 8, 400, False, "LMGPU"),
                              ("image_warping", 512, 512, True, 8, 400, False, "gaussNewtonGPU"), ("image_warping", 512, 512, False, 8, 400, True, "gaussNewtonGPU")]},
    "stencil": {"settings": (1, 2), "out": "onchip_reset.json",
                "workloads": [("poisson_image_editing", 256, 256, False, 1, 100, False), ("poisson_image_editing", 512, 512, False, 1, 100, False), ("optical_flow", 512, 512, False, 3, 50, False)]},
    "sfs": {"settings": (1, 3), "out": "onchip_sfs_reset.json",
            "workloads": [("shape_from_shading", 640, 480, True, 10, 25, False), ("shape_from_shading", 640, 480, False, 10, 25, False), ("shape_from_shading", 1024, 1024, True, 10, 25, False),
                          ("shape_from_shading", 640, 480, True, 10, 10, True)]},
}


def make(energy, W, H, double, control=False):
    from opt_amd import workloads as wl
    if energy == "image_warping":      # (the control of the `general` set: the unit lattice)
        return wl.image_warping(W, H, double=double, random_state=1, mask_fraction=0.02, perturb=0.3, jitter_urshape=0.0 if control else 0.2)
    if energy == "poisson_image_editing":
        return wl.poisson_image_editing(W, H, double=double, seed=1)
    if energy == "optical_flow":
        return wl.optical_flow(W, H, double=double, seed=1, init_flow=1.2)
    return wl.shape_from_shading(W, H, double=double, seed=1, holes=True)


def plan(P, steps, liters, onchip, kind="LMGPU"):
    from opt_amd import api
    g = api.Solver(api.energy_file(P.energy), kind, P.dims, double=P.double, timing=False)
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
    fits_key = SETS[a.set].get("fits_key", "path")      # the key of describe() that says what the workload would take under the new setting
    for energy, askedW, askedH, double, steps, liters, control, *rest in SETS[a.set]["workloads"]:
        kind = rest[0] if rest else "LMGPU"
        W, H = askedW, askedH
        while not control and min(W, H) > 64:      # the largest image a variant with the reset on chip fits
            g = plan(make(energy, W, H, double), steps, liters, new, kind)
            fits = "on-chip" in g.describe().get(fits_key, "")
            g.close()
            if fits:
                break
            W -= 64; H -= 64
        P = make(energy, W, H, double, control)
        dev = api.to_device(P)
        x0 = [dev[i].clone() for i in P.unknown_slots]
        plans = {s: plan(P, steps, liters, s, kind) for s in (base, new)}
        paths = {s: plans[s].describe().get("path" if control else fits_key, plans[s].describe()["path"]) for s in (base, new)}
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
        row = {"energy": energy, "asked": f"{askedW}x{askedH}", "image": f"{W}x{H}", "precision": "double" if double else "float", "solver": "LM" if kind == "LMGPU" else "GN", "steps": steps, "lIterations": liters,
               "residual_reset_period": 10, "note": None if (W, H) == (askedW, askedH) else f"no variant with the reset on chip fits {askedW}x{askedH}; the largest image that does"}
        if control:
            row["control"] = "both settings take the same kernel" if a.set == "general" else "no reset falls inside the solve: both settings take the same kernel"
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
