#!/usr/bin/env python
"""arap_mesh_deformation on small meshes: the two-kernel PCG loop (amd_onchip = 1: arap_flatStepPlanes + arap_applyEll per iteration) against the whole linear solve in one
workgroup (amd_onchip = 5: arap_onchipPcg, opt_amd/csrc/arap_onchip.h).  Whole solves (Opt_ProblemSolve, inputs resident, wall time between two device synchronisations),
both settings in one process, alternating, median and minimum of --solves (5); us per PCG iteration = median solve / (steps x lIterations).

Workloads: the reference's shape -- float Gauss-Newton 20 x 100 (examples/arap_mesh_deformation/src/main.cpp:58-79) -- on small_armadillo (130 vertices), its sqrt(3)
subdivision (386, tests/golden/meshes/armadillo_mesh.npz), a `head`-sized grid (689) and the raptor (2000, tests/fixtures/raptor2k_mesh.npz: no variant serves it -- both settings
stream, a control); grid meshes at every variant's largest size; Levenberg-Marquardt 20 x 100 with q_tolerance = -1e9 on the 386-vertex mesh; double rows.
A row passes if the median under amd_onchip = 5 is below the minimum under amd_onchip = 1 and the plan ran on chip.  Writes profiles/onchip_arap.json.

    python tools/bench_onchip_arap.py                 # the table
    python tools/bench_onchip_arap.py --control       # amd_onchip = 1 alone on the 386-vertex mesh: run on the parent commit's library and on this one (OPT_AMD_LIB)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def armadillo(subdivided, double):
    import numpy as np
    from opt_amd import io
    m = np.load(os.path.join(ROOT, "tests", "golden", "meshes", "armadillo_mesh.npz"))
    s = "_sub" if subdivided else ""
    return io.arap_problem_from_mesh(m["vertices" + s], m["faces" + s].tolist(), m["marker_index" if subdivided else "marker_index_coarse"], m["marker_position"], double=double, alpha=0.1)


def raptor(double):
    import numpy as np
    from opt_amd import io
    m = np.load(os.path.join(ROOT, "tests", "fixtures", "raptor2k_mesh.npz"))
    return io.arap_problem_from_mesh(m["vertices"], m["faces"].tolist(), m["marker_index"], m["marker_position"], double=double, alpha=0.1)


def grid(nx, ny, double):
    from opt_amd import workloads as wl
    return wl.arap_mesh_deformation(nx, ny, double=double, perturb=0.01)


# (name, problem, double, solver kind, steps, lIterations, control: no variant serves it)
WORKLOADS = [
    ("small_armadillo (130)", lambda: armadillo(False, False), "gaussNewtonGPU", 20, 100, False),
    ("small_armadillo, one sqrt(3) subdivision (386)", lambda: armadillo(True, False), "gaussNewtonGPU", 20, 100, False),
    ("head-sized grid 53x13 (689)", lambda: grid(53, 13, False), "gaussNewtonGPU", 20, 100, False),
    ("raptor_simplify2k (2000)", lambda: raptor(False), "gaussNewtonGPU", 20, 100, True),
    ("grid 32x16 (512: largest V = 1)", lambda: grid(32, 16, False), "gaussNewtonGPU", 20, 100, False),
    ("grid 32x32 (1024: largest V = 2)", lambda: grid(32, 32, False), "gaussNewtonGPU", 20, 100, False),
    ("small_armadillo, one sqrt(3) subdivision (386)", lambda: armadillo(True, False), "LMGPU", 20, 100, False),
    ("grid 32x16 (512: largest V = 1)", lambda: grid(32, 16, False), "LMGPU", 20, 100, False),
    ("grid 32x32 (1024: largest V = 2)", lambda: grid(32, 32, False), "LMGPU", 20, 100, False),
    ("small_armadillo, one sqrt(3) subdivision (386)", lambda: armadillo(True, True), "gaussNewtonGPU", 20, 100, False),
    ("grid 32x16 (512: largest V = 1)", lambda: grid(32, 16, True), "gaussNewtonGPU", 20, 100, False),
    ("grid 32x32 (1024: largest V = 2)", lambda: grid(32, 32, True), "gaussNewtonGPU", 20, 100, False),
    ("small_armadillo, one sqrt(3) subdivision (386)", lambda: armadillo(True, True), "LMGPU", 20, 100, False),
    ("grid 32x16 (512: largest V = 1)", lambda: grid(32, 16, True), "LMGPU", 20, 100, False),
]


def plan(P, kind, steps, liters, onchip):
    from opt_amd import api
    g = api.Solver(api.energy_file(P.energy), kind, P.dims, double=P.double, timing=False)
    for k, v in (("nIterations", steps), ("lIterations", liters), ("q_tolerance", -1e9), ("amd_onchip", onchip)):
        g.set_parameter(k, v)
    return g


def measure(P, kind, steps, liters, settings, solves):
    import torch
    from opt_amd import api
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
        solve(s)                      # warm-up (allocations, the edge lists, first touch)
    for _ in range(solves):
        for s in settings:
            times[s].append(solve(s))
    out = {}
    for s in settings:
        t = times[s]
        d = plans[s].describe()
        out[f"amd_onchip={s}"] = {"path": d.get("path"), "variant": d.get("variant"), "why_not_on_chip": d.get("why_not_on_chip"), "on_chip_status": plans[s].on_chip_status(),
                                  "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                                  "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
        plans[s].close()
    return out


def main():
    import torch
    from opt_amd import api
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--control", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onchip_arap.json"))
    a = ap.parse_args()
    if a.control:
        row = {"library": api.LIB_PATH, "workload": "small_armadillo, one sqrt(3) subdivision (386)", "precision": "float", "solver": "GN", "steps": 20, "lIterations": 100}
        row.update(measure(armadillo(True, False), "gaussNewtonGPU", 20, 100, (1,), a.solves))
        print(json.dumps(row), flush=True)
        return 0
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": []}
    ok = True
    for name, make, kind, steps, liters, control in WORKLOADS:
        P = make()
        row = {"mesh": name, "vertices": int(P.dims[0]), "precision": "double" if P.double else "float", "solver": "LM" if kind == "LMGPU" else "GN", "steps": steps, "lIterations": liters}
        row.update(measure(P, kind, steps, liters, (1, 5), a.solves))
        if control:
            row["control"] = "no variant serves this mesh: both settings take the two-kernel loop"
        else:
            row["pass"] = bool(row["amd_onchip=5"]["median_ms"] < row["amd_onchip=1"]["min_ms"] and row["amd_onchip=5"]["on_chip_status"] == 1 and row["amd_onchip=1"]["on_chip_status"] == 0)
            ok = ok and row["pass"]
        res["workloads"].append(row)
        print(json.dumps(row), flush=True)
    res["pass"] = ok
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("PASS" if ok else "FAIL: the median under amd_onchip=5 is not below the minimum under amd_onchip=1 everywhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
