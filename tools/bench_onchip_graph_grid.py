#!/usr/bin/env python
"""The functor mesh energies with the whole linear solve as ONE persistent launch of several workgroups (amd_onchip = 7, amd_onchip_workgroups = G: ge_onchipPcgGrid,
opt_amd/csrc/graph_onchip_grid.h) against every existing setting: four launches per PCG iteration, two (amd_graph_fused = 1) and one workgroup (amd_onchip = 6).
The protocol is that of tools/bench_onchip_graph.py (profiles/onchip_graph.md), whose builders this tool imports: whole solves through Opt_ProblemSolve, inputs resident,
wall time between two device synchronisations, all settings alternating in one process, median and minimum of --solves (5); us per PCG iteration = median solve /
(steps x lIterations).  The three existing settings are unchanged code, so they are the parent commit's behaviour on the same device in the same minute.

Workloads, each also as a double Gauss-Newton row: cotangent GN 5 x 25 on small_armadillo (130 vertices), its subdivision (386), head.ply (689) and the raptor (2000);
embedded and robust GN and LM 5 x 125 on 130, 386, the 32 x 16 grid and the raptor.
A workgroup count counts as faster only if its median is below the MINIMUM of the best existing setting and the plan ran on chip; the automatic table
(GraphOps::ggAutoWorkgroups, graph_engine.h) may name a workload only where that holds.  Also recorded: evaluated / total hyperedges per workload and count (the
entanglement the partition costs), what amd_onchip = 7 chooses by itself (the last column) and, with --gridsync-log, the grid-wide wait in isolation: the output of
tools/microbench_gridsync.hip run once per workgroup count (`mb_gridsync 2000 G` for G = 2, 4, 8, 16, 32, appended to one file).
Writes profiles/onchip_graph_grid.json and profiles/onchip_graph_grid.md: the table, the automatic rule and whether the measurement bears it out row by row, the
entanglement bound, the ratios, the wait.

    python tools/bench_onchip_graph_grid.py [--only embedded] [--solves 5] [--gridsync-log FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_onchip_graph as base      # noqa: E402  (mesh, head, grid, plan)

COUNTS = (2, 4, 8, 16, 32)
EXISTING = {"four launches": dict(amd_graph_fused=0), "two launches": dict(amd_graph_fused=1), "one workgroup": dict(amd_onchip=6)}
SETTINGS = dict(EXISTING, **{"G=%d" % g: dict(amd_onchip=7, amd_onchip_workgroups=g) for g in COUNTS})
SETTINGS["automatic"] = dict(amd_onchip=7)      # amd_onchip_workgroups = 0: what the plan chooses by itself (GraphOps::ggAutoWorkgroups)


def workloads():
    """(energy, mesh name, problem, solver kind, steps, lIterations)"""
    w = []
    for double in (False, True):
        kinds = ("gaussNewtonGPU",) if double else ("gaussNewtonGPU", "LMGPU")
        for name, make in (("small_armadillo (130)", lambda d: base.mesh("cotangent", "armadillo", d)), ("small_armadillo subdivided (386)", lambda d: base.mesh("cotangent", "armadillo_sub", d)),
                           ("head.ply (689)", base.head), ("raptor (2000)", lambda d: base.mesh("cotangent", "raptor", d))):
            w.append(("cotangent", name, lambda make=make, double=double: make(double), "gaussNewtonGPU", 5, 25))
        for e in ("embedded", "robust"):
            for kind in kinds:
                for name, make in (("small_armadillo (130)", lambda d, e=e: base.mesh(e, "armadillo", d)), ("small_armadillo subdivided (386)", lambda d, e=e: base.mesh(e, "armadillo_sub", d)),
                                   ("grid 32x16 (512)", lambda d, e=e: base.grid(e, 32, 16, d)), ("raptor (2000)", lambda d, e=e: base.mesh(e, "raptor", d))):
                    w.append((e, name, lambda make=make, double=double: make(double), kind, 5, 125))
    return w


def measure(P, kind, steps, liters, solves):
    import torch
    from opt_amd import api
    dev = api.to_device(P)
    x0 = [dev[i].clone() for i in P.unknown_slots]
    plans = {s: base.plan(P, kind, steps, liters, p, {}) for s, p in SETTINGS.items()}
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
        solve(s)                      # warm-up (allocations, the incidence lists, the partition, first touch)
    for _ in range(solves):
        for s in SETTINGS:
            times[s].append(solve(s))
    out = {}
    for s in SETTINGS:
        t, d = times[s], plans[s].describe()
        out[s] = {"path": d.get("path"), "workgroups": d.get("workgroups"), "variant": d.get("variant"), "records": d.get("records"), "why_not_on_chip": d.get("why_not_on_chip"),
                  "evaluated_hyperedges": d.get("evaluated_hyperedges"), "held_vertices_max": d.get("held_vertices_max"), "on_chip_status": plans[s].on_chip_status(),
                  "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t), "us_per_pcg_iteration": 1e6 * statistics.median(t) / (steps * liters),
                  "final_cost": costs[s]}
        plans[s].close()
    return out


def gridsync(path):
    """{workgroups: us per round} from the output of tools/microbench_gridsync.hip (the second repetition of the flat sum)."""
    out, g = {}, None
    if path and os.path.exists(path):
        for line in open(path):
            m = re.search(r"(\d+) workgroups of", line)
            if m:
                g = int(m.group(1))
            m = re.match(r"rep 1\s+sum, flat.*?([0-9.]+) us per round", line)
            if m and g is not None:
                out[g] = float(m.group(1))
    return out


def markdown(res):
    rows = res["workloads"]
    L = ["# The functor mesh energies on several workgroups in one launch (`amd_onchip=7`)", "",
         "`tools/bench_onchip_graph_grid.py` on one MI355X (the runtime names it \"%s\"), this commit; the protocol of `profiles/onchip_graph.md`: whole solves through `Opt_ProblemSolve`, all settings" % res["device"],
         "alternating in one process, %d solves per setting after a warm-up, µs per PCG iteration = median solve / (steps × iterations); LM with `q_tolerance = -1e9`. The first three" % res["solves_per_setting"],
         "columns are unchanged code: the parent commit's behaviour on the same device in the same minute. A count is **faster** only if its median is below the *minimum* of the",
         "best existing setting. In a G column: µs per iteration (evaluated / total hyperedges), or why the plan was refused. Raw figures: `profiles/onchip_graph_grid.json`.", "",
         "| energy | mesh | precision | solver | four launches | two launches | one workgroup | " + " | ".join("G=%d" % g for g in COUNTS) + " | best count | automatic (`amd_onchip_workgroups=0`) |",
         "|---|---|---|---|---|---|---|" + "---|" * len(COUNTS) + "---|---|"]

    def cell(r, s):
        c = r[s]
        if s.startswith("G=") and c["on_chip_status"] != 1:
            return "refused: %s" % (c["why_not_on_chip"] or "")
        extra = " (%.2f)" % (int(c["evaluated_hyperedges"]) / max(1, r["hyperedges"])) if c.get("evaluated_hyperedges") else ""
        return "%.1f%s" % (c["us_per_pcg_iteration"], extra)

    for r in rows:
        a = r["automatic"]
        auto = "%s workgroup%s, %.1f: %s" % (a["workgroups"] or "-", "" if a["workgroups"] == "1" else "s", a["us_per_pcg_iteration"], r["automatic_verdict"])
        L.append("| %s | %s | %s | %s | %s | %s | %s |" % (r["energy"], r["mesh"], r["precision"], r["solver"], " | ".join(cell(r, s) for s in list(EXISTING) + ["G=%d" % g for g in COUNTS]),
                                                       r["verdict"], auto))
    wins = [r for r in rows if r.get("faster")]
    losses = [r for r in rows if not r.get("faster")]
    L += ["", "## The automatic rule", "",
          "`GraphOps::ggAutoWorkgroups` (`graph_engine.h`): with `amd_onchip_workgroups = 0` level 7 takes **32 workgroups** on a mesh of 130 to 2000 vertices -- the range",
          "measured here, in which 32 was the fastest count wherever a count won -- up to the functor's `kOnChipGridAutoMaxVertices[precision]`: 2000, and 689 for cotangent in",
          "double, which lost on the raptor. Elsewhere, and where the several-workgroup predicate refuses the plan, it does exactly what level 6 does. The last column above is",
          "that choice measured like every other setting; a row where the automatic choice took several workgroups without being faster by the rule contradicts the table:", ""]
    bad = [r for r in rows if r["automatic"]["workgroups"] not in (None, "1") and not r["automatic_faster"]]
    L += ["* %d of %d workloads have a count that is faster by the rule; %d have none (%s)." % (len(wins), len(rows), len(losses),
                                                                                              "; ".join("%s %s %s %s" % (r["energy"], r["mesh"], r["precision"], r["solver"]) for r in losses) or "none"),
          "* the automatic choice took several workgroups on %d workloads and was faster by the rule on %d of them%s." % (
              sum(1 for r in rows if r["automatic"]["workgroups"] not in (None, "1")), sum(1 for r in rows if r["automatic"]["workgroups"] not in (None, "1") and r["automatic_faster"]),
              "" if not bad else " -- NOT on: " + "; ".join("%s %s %s %s" % (r["energy"], r["mesh"], r["precision"], r["solver"]) for r in bad)),
          "* a workload that loses stays reachable through `amd_onchip_workgroups`.", "",
          "## Entanglement: evaluated / total hyperedges", "",
          "Cut hyperedges are evaluated by every workgroup that owns one of their vertices. The ratio per workload and count is the bracketed figure of the table; over all rows:", ""]
    for g in COUNTS:
        ratios = [int(r["G=%d" % g]["evaluated_hyperedges"]) / max(1, r["hyperedges"]) for r in rows if r["G=%d" % g].get("evaluated_hyperedges")]
        if ratios:
            L.append("* G = %d: %.2f to %.2f" % (g, min(ratios), max(ratios)))
    top = max(((int(r["G=%d" % g]["evaluated_hyperedges"]) / max(1, r["hyperedges"]), r, g) for r in rows for g in COUNTS if r["G=%d" % g].get("evaluated_hyperedges")), key=lambda t: t[0], default=None)
    if top:
        best = min(top[1][s]["min_ms"] for s in EXISTING)
        L += ["", "The largest ratio measured is %.2f (%s, %s, %s, G = %d), where the count is %s by the rule. The bound of the automatic choice (`kGgEntangledNum / kGgEntangledDen`," % (
                  top[0], top[1]["energy"], top[1]["mesh"], top[1]["precision"], top[2], "still faster" if top[1]["G=%d" % top[2]]["median_ms"] < best else "not faster"),
              "`graph_engine.h`, \"partition too entangled\") is 11 / 4 = 2.75: just beyond what was measured, nothing is claimed. A forced count is not held to it."]
    L += ["", "## The grid-wide wait in isolation", ""]
    if res.get("gridsync_us"):
        L += ["`tools/microbench_gridsync.hip` with a workgroup count (`mb_gridsync 2000 G`): every workgroup posts four double sums as tagged words and reads every workgroup's, 2000",
              "dependent rounds in one launch, µs per round (second repetition):", "", "| workgroups | " + " | ".join(str(g) for g in sorted(res["gridsync_us"], key=int)) + " |",
              "|---|" + "---|" * len(res["gridsync_us"]), "| µs per wait | " + " | ".join("%.2f" % res["gridsync_us"][g] for g in sorted(res["gridsync_us"], key=int)) + " |", "",
              "(256 threads per workgroup and no ring words: the kernel's own wait carries the halo's A·p as well.)"]
    else:
        L += ["not recorded in this run (`--gridsync-log`)."]
    return "\n".join(L) + "\n"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--only", default=None, help="energy name: measure its workloads only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onchip_graph_grid.json"))
    ap.add_argument("--gridsync-log", default=None, help="output of tools/microbench_gridsync.hip, one run per workgroup count")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "solves_per_setting": a.solves, "gridsync_us": {str(g): t for g, t in gridsync(a.gridsync_log).items()}, "workloads": []}
    for energy, name, make, kind, steps, liters in workloads():
        if a.only and energy != a.only:
            continue
        P = make()
        row = {"energy": energy, "mesh": name, "vertices": int(P.dims[0]), "hyperedges": int(P.meta["n_edges"]), "precision": "double" if P.double else "float",
               "solver": "LM" if kind == "LMGPU" else "GN", "steps": steps, "lIterations": liters}
        row.update(measure(P, kind, steps, liters, a.solves))
        best = min(row[s]["min_ms"] for s in EXISTING)
        ran = {s: row[s] for s in SETTINGS if s.startswith("G=") and row[s]["on_chip_status"] == 1}
        if not ran:
            row["faster"], row["verdict"] = False, "no count ran on chip"
        else:
            s = min(ran, key=lambda k: ran[k]["median_ms"])
            row["best_count"], row["faster"] = s, bool(ran[s]["median_ms"] < best)
            row["verdict"] = ("**faster** at %s (%.2fx)" if row["faster"] else "LOSS, best at %s (%.2fx)") % (s, best / ran[s]["median_ms"])
        auto = row["automatic"]
        row["automatic_faster"] = bool(auto["on_chip_status"] == 1 and auto["workgroups"] not in (None, "1") and auto["median_ms"] < best)
        row["automatic_verdict"] = "as level 6" if auto["workgroups"] in (None, "1") else ("**faster** (%.2fx)" if row["automatic_faster"] else "NOT faster (%.2fx)") % (best / auto["median_ms"])
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
