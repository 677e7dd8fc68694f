#!/usr/bin/env python
"""What a plug-in energy costs per PCG iteration, and which parameter to set: the sample plug-in (examples/plugins/spring_mesh_deformation.{t,hip}, built by
opt_amd/build.py build_plugin, loaded with OptAmd_LoadEnergyPlugin) on the reference-sized raptor mesh (2000 vertices, tests/fixtures/raptor2k_mesh.npz) in float,
Gauss-Newton 5 x 125, on three of the engine's paths: the default (four launches per PCG iteration), amd_graph_fused = 1 (two), amd_onchip = 7 with 32 workgroups
(the whole linear solve in one launch; the defaults base of OptAmdPlugin.h takes several workgroups only where the caller names a count).

The protocol of tools/bench_graph_fused.py: whole solves (Opt_ProblemSolve, inputs resident, wall time between two device synchronisations), all settings in one
process, alternating, median and minimum of --solves (5) after a warm-up; us per PCG iteration = median solve / (steps x lIterations).  No bar: the table tells a
plug-in author what to expect.  Beside it, embedded_mesh_deformation's rows for the same mesh, precision and solver from profiles/graph_fused.md and
profiles/onchip_graph_grid.md (measured when those paths were added, not re-measured here).  Writes profiles/plugin_energy.md.

    python tools/bench_plugin_energy.py [--out profiles/plugin_energy]
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

STEPS, LITERS = 5, 125
SETTINGS = [("default (four launches)", {}), ("amd_graph_fused=1 (two launches)", {"amd_graph_fused": 1}),
            ("amd_onchip=7, amd_onchip_workgroups=32 (one launch)", {"amd_onchip": 7, "amd_onchip_workgroups": 32})]


def raptor_problem():
    import numpy as np
    from opt_amd import workloads as wl
    z = np.load(os.path.join(ROOT, "tests", "fixtures", "raptor2k_mesh.npz"))
    V, F = z["vertices"].astype(np.float64), z["faces"].tolist()
    Fa = np.asarray(F)
    L = float(np.mean([np.linalg.norm(V[Fa[:, i]] - V[Fa[:, (i + 1) % 3]], axis=1).mean() for i in range(3)]))      # unit mean edge length, like the mesh tests
    order = np.argsort(V[:, 0], kind="stable"); k = max(1, len(V) // 20)
    return wl.spring_from_mesh(V / L, F, np.sort(order[:k]), np.sort(order[-k:]), double=False, seed=7, perturb=0.03)


def measure(solves):
    import torch
    from opt_amd import api, build, workloads as wl
    api.load_energy_plugin(build.plugin_path("spring_mesh_deformation"))
    P = raptor_problem()
    dev = api.to_device(P)
    x0 = dev[0].clone()
    plans = []
    for _, params in SETTINGS:
        g = api.Solver(wl.SPRING_T, "gaussNewtonGPU", P.dims, double=False)
        for k, v in dict(nIterations=STEPS, lIterations=LITERS, **params).items():
            g.set_parameter(k, v)
        plans.append(g)
    times, costs = [[] for _ in plans], [None] * len(plans)

    def solve(i):
        dev[0].copy_(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[i].solve(dev)
        torch.cuda.synchronize()
        costs[i] = plans[i].cost()
        return time.perf_counter() - t0

    for i in range(len(plans)):
        solve(i)      # warm-up: allocations, incidence lists, the partition
    for _ in range(solves):
        for i in range(len(plans)):
            times[i].append(solve(i))
    rows = []
    for i, (name, _) in enumerate(SETTINGS):
        d = plans[i].describe()
        path = d.get("path", "") + (", workgroups=" + d["workgroups"] if "workgroups" in d else "") + (", launches_per_iteration=" + d["launches_per_iteration"] if "launches_per_iteration" in d else "")
        if "why_not_on_chip" in d:
            path += ", why_not_on_chip=" + d["why_not_on_chip"]
        rows.append(dict(setting=name, path=path, status=plans[i].on_chip_status(), median_ms=1e3 * statistics.median(times[i]), min_ms=1e3 * min(times[i]),
                         us=1e6 * statistics.median(times[i]) / (STEPS * LITERS), cost=costs[i]))
        plans[i].close()
    return dict(device=torch.cuda.get_device_name(0), vertices=int(P.dims[0]), hyperedges=P.meta["n_edges"], solves=solves, rows=rows)


def embedded_rows():
    """us per PCG iteration of embedded_mesh_deformation on the raptor, float GN, as the committed tables state it: (four launches, two launches, 32 workgroups)."""
    out = {}
    try:
        for l in open(os.path.join(ROOT, "profiles", "graph_fused.md")):
            c = [x.strip() for x in l.split("|")]
            if len(c) > 9 and c[1] == "embedded, raptor (2000)" and c[3] == "float GN" and c[4] == "%d x %d" % (STEPS, LITERS):
                out["graph_fused.md"] = (c[6], c[8], None)
        for l in open(os.path.join(ROOT, "profiles", "onchip_graph_grid.md")):
            c = [x.strip() for x in l.split("|")]
            if len(c) > 13 and c[1:5] == ["embedded", "raptor (2000)", "float", "GN"]:
                out["onchip_graph_grid.md"] = (c[5], c[6], re.sub(r"\s*\(.*", "", c[12]))
    except OSError:
        pass
    return out


def markdown(res):
    L = ["# A plug-in energy on the engine's paths: what to expect, which parameter to set", "",
         f"`tools/bench_plugin_energy.py` on one MI355X (the runtime names it \"{res['device']}\"): the sample plug-in `spring_mesh_deformation` (`examples/plugins/`, loaded with",
         f"`OptAmd_LoadEnergyPlugin`) on the raptor mesh ({res['vertices']} vertices, {res['hyperedges']} half-edges), float, Gauss-Newton {STEPS} x {LITERS}.  Whole solves through `Opt_ProblemSolve`,",
         f"the settings alternating in one process, median (minimum) of {res['solves']} after a warm-up; µs per PCG iteration = median solve / ({STEPS} x {LITERS}).  No bar is attached.", "",
         "| setting | path taken | median ms (min) | µs per PCG iteration | final cost |", "|---|---|---|---|---|"]
    for r in res["rows"]:
        L.append(f"| `{r['setting']}` | {r['path']} (status {r['status']}) | {r['median_ms']:.2f} ({r['min_ms']:.2f}) | {r['us']:.1f} | {r['cost']:.6g} |")
    L += ["", "The final costs differ between the paths because this is float: 625 PCG iterations on a non-linear energy amplify the paths' different rounding (the two-launch",
          "loop forms beta by expansion, the on-chip solve sums in another order).  In double the paths agree to 1e-10 per step (`tests/test_plugin_energy_gpu.py`)."]
    emb = embedded_rows()
    if emb:
        L += ["", "For comparison, the built-in `embedded_mesh_deformation` (12 unknowns per vertex, 9 + 3 residuals) on the same mesh, float GN, µs per PCG iteration as the committed",
              "tables state it (measured when those paths were added, not re-measured here):", "", "| source | four launches | two launches | 32 workgroups |", "|---|---|---|---|"]
        for src, (a, b, c) in emb.items():
            L.append(f"| `profiles/{src}` | {a} | {b} | {c or '-'} |")
    L += ["", "A plug-in functor that derives from `GraphFunctorDefaults` reaches the one-launch solve of a mesh of more than 512 vertices only with `amd_onchip=7` AND",
          "`amd_onchip_workgroups`: the defaults name no automatic workgroup count (`kOnChipGridAutoMaxVertices = {0, 0}`).  An author who has measured a table like this one",
          "for the energy declares the constant in the functor."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plugin_energy"))
    a = ap.parse_args()
    res = measure(a.solves)
    md = markdown(res)
    with open(a.out + ".md", "w") as f:
        f.write(md)
    print(md)
    return 0


if __name__ == "__main__":
    sys.exit(main())
