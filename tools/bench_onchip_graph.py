#!/usr/bin/env python
"""The functor mesh energies (cotangent_mesh_smoothing, embedded_mesh_deformation, robust_nonrigid_alignment) on small meshes: the whole linear solve in one workgroup
(amd_onchip = 6: ge_onchipPcg, opt_amd/csrc/graph_onchip.h) against both existing loops at the default level -- four launches per PCG iteration (amd_graph_fused = 0)
and two (amd_graph_fused = 1); and level 6 with the records of an iteration always in memory (OPT_AMD_ONCHIP_REC_LDS=0) beside the default placement (LDS where they fit).  Whole solves (Opt_ProblemSolve, inputs resident, wall time between two device synchronisations), all settings in one process,
alternating, median and minimum of --solves (5); us per PCG iteration = median solve / (steps x lIterations).

Workloads: cotangent float Gauss-Newton 5 x 25 (the reference's shape, examples/cotangent_mesh_smoothing) on small_armadillo (130 vertices), its sqrt(3) subdivision
(386) and head.ply (689, tests/golden/meshes/head_mesh.npz); embedded and robust float, Gauss-Newton and Levenberg-Marquardt 5 x 125 (q_tolerance = -1e9), on 130, 386,
32 x 16, 23 x 23 and 32 x 32 (the last two beyond these energies' largest variant: they stream); double rows at 130 and at a larger size per energy; the raptor (2000 vertices: no variant serves it -- every setting streams, a control).
A row counts as faster only if the median under amd_onchip = 6 is below the MINIMUM of the better existing loop and the plan ran on chip; a losing row is reported as a
loss.  Writes profiles/onchip_graph.json and profiles/onchip_graph.md (with the per-variant register / LDS table from the build's resource remarks).

    python tools/bench_onchip_graph.py
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETTINGS = {"four launches": dict(amd_graph_fused=0), "two launches": dict(amd_graph_fused=1), "on chip": dict(amd_onchip=6), "on chip, records in memory": dict(amd_onchip=6)}
ENV = {"on chip, records in memory": {"OPT_AMD_ONCHIP_REC_LDS": "0"}}      # read when the plan is made: the A/B switch of the record placement


def mesh(energy, name, double):
    import graph_cases as gc
    return gc.base_problem(energy, name, double)


def head(double):
    import numpy as np
    from opt_amd import workloads as wl
    z = np.load(os.path.join(ROOT, "tests", "golden", "meshes", "head_mesh.npz"))
    return wl.cotangent_from_mesh(z["vertices"].astype(np.float64), z["faces"].tolist(), double=double, seed=0)


def grid(energy, nx, ny, double):
    from opt_amd import workloads as wl
    make = {"embedded": wl.embedded_mesh_deformation, "robust": wl.robust_nonrigid_alignment}[energy]
    return make(nx, ny, double=double, seed=3, perturb=0.01)


def workloads():
    """(energy, mesh name, problem, solver kind, steps, lIterations, control: no variant serves it)"""
    w = [("cotangent", "small_armadillo (130)", lambda: mesh("cotangent", "armadillo", False), "gaussNewtonGPU", 5, 25, False),
         ("cotangent", "small_armadillo, one sqrt(3) subdivision (386)", lambda: mesh("cotangent", "armadillo_sub", False), "gaussNewtonGPU", 5, 25, False),
         ("cotangent", "head.ply (689)", lambda: head(False), "gaussNewtonGPU", 5, 25, False)]
    for e in ("embedded", "robust"):
        for kind in ("gaussNewtonGPU", "LMGPU"):
            w += [(e, "small_armadillo (130)", lambda e=e: mesh(e, "armadillo", False), kind, 5, 125, False),
                  (e, "small_armadillo, one sqrt(3) subdivision (386)", lambda e=e: mesh(e, "armadillo_sub", False), kind, 5, 125, False),
                  (e, "grid 32x16 (512: the largest variant)", lambda e=e: grid(e, 32, 16, False), kind, 5, 125, False),
                  (e, "grid 23x23 (529: beyond the largest variant)", lambda e=e: grid(e, 23, 23, False), kind, 5, 125, False),
                  (e, "grid 32x32 (1024: beyond the largest variant)", lambda e=e: grid(e, 32, 32, False), kind, 5, 125, False)]
    w += [(e, "small_armadillo (130)", lambda e=e: mesh(e, "armadillo", True), "gaussNewtonGPU", 5, 25 if e == "cotangent" else 125, False) for e in ("cotangent", "embedded", "robust")]
    w += [("cotangent", "head.ply (689)", lambda: head(True), "gaussNewtonGPU", 5, 25, False),
          ("embedded", "small_armadillo, one sqrt(3) subdivision (386)", lambda: mesh("embedded", "armadillo_sub", True), "gaussNewtonGPU", 5, 125, False),
          ("robust", "small_armadillo, one sqrt(3) subdivision (386)", lambda: mesh("robust", "armadillo_sub", True), "gaussNewtonGPU", 5, 125, False)]
    for e in ("cotangent", "embedded", "robust"):
        w.append((e, "raptor_simplify2k (2000)", lambda e=e: mesh(e, "raptor", False), "gaussNewtonGPU", 5, 25 if e == "cotangent" else 125, True))
    return w


def plan(P, kind, steps, liters, params, env):
    from opt_amd import api
    os.environ.update(env)
    try:
        g = api.Solver(api.energy_file(P.energy), kind, P.dims, double=P.double, timing=False)
    finally:
        for k in env:
            del os.environ[k]
    for k, v in dict(nIterations=steps, lIterations=liters, q_tolerance=-1e9, **params).items():
        g.set_parameter(k, v)
    return g


def measure(P, kind, steps, liters, solves):
    import torch
    from opt_amd import api
    dev = api.to_device(P)
    x0 = [dev[i].clone() for i in P.unknown_slots]
    plans = {s: plan(P, kind, steps, liters, p, ENV.get(s, {})) for s, p in SETTINGS.items()}
    times, costs = {s: [] for s in SETTINGS}, {}

    def solve(s):
        for i, x in zip(P.unknown_slots, x0):
            dev[i].copy_(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[s].solve(dev)
        torch.cuda.synchronize()
        costs[s] = plans[s].cost()
        return time.perf_counter() - t0

    for s in SETTINGS:
        solve(s)                      # warm-up (allocations, the incidence lists, first touch)
    for _ in range(solves):
        for s in SETTINGS:
            times[s].append(solve(s))
    out = {}
    for s in SETTINGS:
        t = times[s]
        d = plans[s].describe()
        out[s] = {"path": d.get("path"), "variant": d.get("variant"), "records": d.get("records"), "why_not_on_chip": d.get("why_not_on_chip"), "on_chip_status": plans[s].on_chip_status(),
                  "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                  "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters), "final_cost": costs[s]}
        plans[s].close()
    return out


def variant_table():
    """[(variant, VGPRs, SGPRs, static LDS, scratch)] of every ge_onchipPcg of the last build, or [] where the build's remarks are not at hand."""
    from opt_amd import build
    rows = []
    for name, r in sorted(build.kernel_resources().items()):
        m = re.match(r"^ge_onchipPcg<(.*)>$", name)
        if m:
            rows.append((re.sub(r"(\w+G)<(?:float|double)>", r"\1", m.group(1)).replace("false", "GN").replace("true", "LM"), r["vgprs"], r["sgprs"], r["lds"], r["scratch"]))
    return rows


def markdown(res):
    L = ["# The functor mesh energies on small meshes: the linear solve in one workgroup (`amd_onchip=6`)", "",
         "`tools/bench_onchip_graph.py` on one MI355X (the runtime names it \"%s\"), this commit. Whole solves (`Opt_ProblemSolve`, inputs resident, wall time between two device" % res["device"],
         "synchronisations): the default level with four launches per PCG iteration (`amd_graph_fused=0`) and with two (`amd_graph_fused=1`) against `amd_onchip=6`",
         "(`ge_onchipPcg`, one launch of one workgroup per linear solve; and the same with `OPT_AMD_ONCHIP_REC_LDS=0`: the records always in memory), in the same process, alternating, %d solves per setting after a warm-up; LM with" % res["solves_per_setting"],
         "`q_tolerance = -1e9`. µs per PCG iteration = median solve / (steps × iterations): it carries the outer step as well. A row is **faster** only if the median under",
         "level 6 is below the minimum of the better existing loop. Raw figures: `profiles/onchip_graph.json`.", "",
         "| energy | mesh | vertices | precision | solver | steps × iterations | four launches ms (median / min) | µs / it. | two launches ms (median / min) | µs / it. | level 6 ms (median / min) | µs / it. | records | level 6, records in memory ms (median / min) | µs / it. | variant | verdict |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["workloads"]:
        c = lambda s: "%.2f / %.2f | %.2f" % (r[s]["median_ms"], r[s]["min_ms"], r[s]["us_per_pcg_iteration"])
        var = (r["on chip"]["variant"] or "").replace("ge_onchipPcg", "") or "streams (%s)" % (r["on chip"]["why_not_on_chip"] or "")
        L.append("| %s | %s | %d | %s | %s | %d × %d | %s | %s | %s | %s | %s | `%s` | %s |" % (r["energy"], r["mesh"], r["vertices"], r["precision"], r["solver"], r["steps"], r["lIterations"],
                                                                                            c("four launches"), c("two launches"), c("on chip"), r["on chip"]["records"] or "", c("on chip, records in memory"), var,
                                                                                            r["verdict"]))
    L += ["", "## The variants", "", "Registers, static LDS and scratch of every offered kernel (the build's resource remarks; dynamic LDS: 2 K scalars per vertex for p and delta,",
          "3 K where r lives there too -- cotangent and embedded in double).", "", "| `ge_onchipPcg<…>` | VGPRs | SGPRs | static LDS (bytes) | scratch |", "|---|---|---|---|---|"]
    L += ["| `%s` | %d | %d | %d | %d |" % tuple(v) for v in res["variants"]]
    L += ["", "## Not offered", "",
          "V = 2 (513 - 1024 vertices) for embedded and robust was built and measured with this tool before it was taken out (float, 5 × 125, µs per PCG iteration, level 6",
          "against the two-launch loop): embedded GN 20.7 against 14.7 at 529 vertices and 33.7 against 14.6 at 1024, LM 23.0 / 17.9 and 37.4 / 18.2; robust GN 18.8 / 15.2",
          "and 31.4 / 15.6, LM 20.8 / 18.7 and 34.6 / 19.6. It lost at both ends of its range, so these energies end at 512 vertices (in double embedded's V = 2 does not",
          "fit LDS and robust's spills under LM as well). cotangent keeps V = 2 because it is what serves head.ply, and is reported above as the loss it is: its hyperedge",
          "costs about two thousand VALU instructions, and 4086 of them on the four SIMDs of one CU take longer than the four launches they replace."]
    return "\n".join(L) + "\n"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onchip_graph.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "workloads": [], "variants": variant_table()}
    for energy, name, make, kind, steps, liters, control in workloads():
        P = make()
        row = {"energy": energy, "mesh": name, "vertices": int(P.dims[0]), "hyperedges": int(P.meta["n_edges"]), "precision": "double" if P.double else "float",
               "solver": "LM" if kind == "LMGPU" else "GN", "steps": steps, "lIterations": liters}
        row.update(measure(P, kind, steps, liters, a.solves))
        best = min(row["four launches"]["min_ms"], row["two launches"]["min_ms"])
        if control:
            row["verdict"] = "control: streams under every setting" if row["on chip"]["on_chip_status"] == 0 else "control ran on chip"
        elif row["on chip"]["on_chip_status"] == 0:
            row["verdict"] = "streams: " + (row["on chip"]["why_not_on_chip"] or "")
        else:
            row["faster"] = bool(row["on chip"]["median_ms"] < best and row["on chip"]["on_chip_status"] == 1)
            row["verdict"] = ("**faster** (%.2fx)" % (best / row["on chip"]["median_ms"])) if row["faster"] else ("LOSS (%.2fx)" % (best / row["on chip"]["median_ms"]))
        res["workloads"].append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
        f.write(markdown(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
