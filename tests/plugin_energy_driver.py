"""Child-process body of the plug-in energy tests (test_plugin_energy_cpu.py, test_plugin_energy_gpu.py).

The kernel registry of libOpt.so is process-global and other tests enumerate it, so nothing loads a plug-in inside the pytest process: every case runs here,
    python tests/plugin_energy_driver.py <case> '<json arguments>'
and prints ONE line of JSON (floats by repr: they round-trip bit for bit).  The module is also imported by the tests for the problem builders, so that parent
and child build the same inputs; importing it loads nothing."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from opt_amd import workloads as wl      # noqa: E402

SPRING_T = wl.SPRING_T
MESHES = ("grid", "armadillo", "grid_shapes")
KINDS = {"GN": "gaussNewtonGPU", "LM": "LMGPU"}
IDX = (6, 7)      # binding slots of v0, v1; 5: the edge count; 0, 1, 2: X, UrShape, Constraints


def _set_edges(P, heads, tails):
    P.params[IDX[0]] = np.ascontiguousarray(heads, dtype=np.int32); P.params[IDX[1]] = np.ascontiguousarray(tails, dtype=np.int32)
    P.params[5] = np.array(len(heads), dtype=np.int32); P.meta["n_edges"] = int(len(heads))
    assert len(heads) == len(tails) >= 1 and 0 <= min(heads.min(), tails.min()) and max(heads.max(), tails.max()) < P.dims[0]
    return P


def problem(mesh, double):
    """The three inputs of the GPU tests.  grid: 7 x 5 vertices (35; wl.grid_mesh_edges: interior and boundary vertices in one workgroup), the left column
    pinned, the right one lifted.  armadillo: 130 vertices, unit mean edge length, the 5 % of smallest x pinned, of largest x lifted.  grid_shapes: the grid plus
    one vertex without hyperedges and one hub of degree 16 (half-edges in both directions, grouped by head), as tests/graph_cases.py builds them."""
    if mesh == "armadillo":
        z = np.load(os.path.join(ROOT, "tests", "golden", "meshes", "armadillo_mesh.npz"))
        V, F = z["vertices"].astype(np.float64), z["faces"].tolist()
        Fa = np.asarray(F)
        L = float(np.mean([np.linalg.norm(V[Fa[:, i]] - V[Fa[:, (i + 1) % 3]], axis=1).mean() for i in range(3)]))
        order = np.argsort(V[:, 0], kind="stable"); k = max(1, len(V) // 20)
        return wl.spring_from_mesh(V / L, F, np.sort(order[:k]), np.sort(order[-k:]), double=double, seed=7, perturb=0.05)
    V, F = wl.grid_surface_mesh(7, 5, seed=4)
    P = wl.spring_from_mesh(V, F, np.arange(5) * 7, np.arange(5) * 7 + 6, double=double, seed=7, perturb=0.05)
    heads, tails = wl.grid_mesh_edges(7, 5)
    _set_edges(P, heads, tails)
    if mesh == "grid":
        return P
    assert mesh == "grid_shapes", mesh
    N, hub, degree = 35, 17, 16
    have = set(int(t) for t in tails[heads == hub])
    add_h, add_t = [], []
    for v in range(N):
        if int(np.sum(heads == hub)) + len(add_h) // 2 >= degree:
            break
        if v != hub and v not in have:
            add_h += [hub, v]; add_t += [v, hub]
    heads, tails = np.concatenate([heads, np.array(add_h, np.int32)]), np.concatenate([tails, np.array(add_t, np.int32)])
    order = np.argsort(heads, kind="stable")
    rest = np.asarray(P.params[1], dtype=np.float64)
    pos = rest.mean(0) + 0.5 * rest.std(0)      # the isolated vertex: free, at rest
    for s, row in ((0, pos), (1, pos), (2, np.full(3, -np.inf))):
        P.params[s] = np.ascontiguousarray(np.concatenate([P.params[s], row[None].astype(P.params[s].dtype)]))
    P.dims = (N + 1,)
    _set_edges(P, heads[order], tails[order])
    assert int(np.sum(P.params[IDX[0]] == hub)) == degree
    return P


def probe_direction(n):
    return np.random.default_rng(11).standard_normal(n)


# ---- host-only cases -----------------------------------------------------------------------------------------------------------------------------------------
def _api():
    from opt_amd import api
    return api


def _try_load(path):
    api = _api()
    try:
        n, msg = api.load_energy_plugin(path), ""
    except RuntimeError as e:
        n, msg = -1, str(e)
    return {"n": n, "message": msg, "count": len(api.registered_energies())}


def case_before(a):
    api = _api()
    ok, msg = api.check_problem_file(SPRING_T)
    return {"ok": ok, "message": msg, "names": api.registered_energies()}


def case_load(a):
    api = _api()
    before = api.registered_energies()
    n = api.load_energy_plugin(a["plugin"])
    out = {"n": n, "before": before, "names": api.registered_energies(), "hash": "%016x" % api.problem_file_hash(SPRING_T)}
    out["own"] = api.check_problem_file(SPRING_T)
    src = open(SPRING_T).read()
    tmp = a["tmp"]

    def written(sub, name, text):
        d = os.path.join(tmp, sub); os.makedirs(d, exist_ok=True)
        p = os.path.join(d, name); open(p, "w").write(text)
        return api.check_problem_file(p)

    out["other_name"] = written("a", "my_springs.t", src)
    edited = src.replace("Energy(w_regSqrt * (length(", "Energy(2 * w_regSqrt * (length(")
    moved = src.replace('Image("UrShape", opt_float3, {N}, 1)', 'Image("UrShape", opt_float3, {N}, 4)')
    assert edited != src and moved != src
    out["edited_body"] = written("b", "spring_mesh_deformation.t", edited)
    out["moved_index"] = written("c", "spring_mesh_deformation.t", moved)
    out["builtin"] = api.check_problem_file(api.energy_file("embedded_mesh_deformation"))
    return out


def case_refusals(a):
    api = _api()
    out = {"count0": len(api.registered_energies())}
    for key in ("missing", "no_entry", "abi_skew", "duplicate_builtin", "sample", "sample_again"):
        out[key] = _try_load(a[key])
    out["names"] = api.registered_energies()
    return out


def case_env(a):
    """OPT_AMD_ENERGY_PLUGINS is set by the parent; no explicit load call.  Without a GPU Opt_NewState returns NULL (Solver raises) and has loaded the list."""
    api = _api()
    before = api.registered_energies()
    try:
        g = api.Solver(SPRING_T, "gaussNewtonGPU", (35,), double=True)
        state = True
        g.close()
    except RuntimeError:
        state = False
    return {"before": before, "state": state, "names": api.registered_energies(), "check": api.check_problem_file(SPRING_T)}


# ---- GPU cases -------------------------------------------------------------------------------------------------------------------------------------------------
def _load(a):
    if a.get("plugin"):
        _api().load_energy_plugin(a["plugin"])      # (else: OPT_AMD_ENERGY_PLUGINS, or nothing)


def _solver(P, t_file, kind, params):
    g = _api().Solver(t_file, KINDS[kind], P.dims, double=P.double)
    for k, v in params.items():
        g.set_parameter(k, v)
    return g


def case_probes(a):
    import torch
    _load(a)
    out = {}
    for mesh in MESHES:
        P = problem(mesh, a["double"])
        dev = _api().to_device(P)
        g = _solver(P, SPRING_T, "GN", {})
        v = torch.from_numpy(probe_direction(g.n).astype(np.float64 if P.double else np.float32)).cuda()
        r, diag = g.eval_jtf(dev)
        rec = {"n": g.n, "cost": g.eval_cost(dev), "r": r.cpu().numpy().astype(np.float64).tolist(), "diag": diag.cpu().numpy().astype(np.float64).tolist()}
        g.close()
        for fused in (0, 1):
            g = _solver(P, SPRING_T, "GN", {"amd_graph_fused": fused})
            o, dot = g.apply_jtj(dev, v)
            rec["out%d" % fused] = o.cpu().numpy().astype(np.float64).tolist(); rec["dot%d" % fused] = dot
            g.close()
        out[mesh] = rec
    return out


def _run(P, t_file, kind, nsteps, liters, params):
    """Init + Step by Step: return values, costs (after init and every step), the LM radius after every step, describe() before and after, the status, the unknowns."""
    api = _api()
    g = _solver(P, t_file, kind, dict(nIterations=nsteps, lIterations=liters, **params))
    dev = api.to_device(P)
    g.init(dev)
    rec = {"ret": [], "cost": [g.cost()], "radius": [], "describe_before": g.describe()}
    while True:
        more = g.step(dev)
        rec["ret"].append(int(more)); rec["cost"].append(g.cost()); rec["radius"].append(g.trust_region_radius() if kind == "LM" else 0.0)
        if not more:
            break
    rec["describe"] = g.describe(); rec["status"] = g.on_chip_status()
    rec["x"] = np.concatenate([dev[i].reshape(-1).cpu().numpy().astype(np.float64) for i in P.unknown_slots]).tolist()
    g.close()
    return rec


def case_solves(a):
    """a["runs"]: [{name, mesh, double, kind, nsteps, liters, params, energy}] run one after the other in this process."""
    _load(a)
    out = {}
    for r in a["runs"]:
        if r.get("energy", "spring") == "spring":
            P, t = problem(r["mesh"], r["double"]), SPRING_T
        else:      # a built-in energy next to the plug-in: embedded_mesh_deformation on the 7 x 5 patch
            V, F = wl.grid_surface_mesh(7, 5, seed=4)
            P = wl.embedded_from_mesh(V, F, np.arange(5) * 7, np.arange(5) * 7 + 6, double=r["double"], seed=7, perturb=0.03)
            t = _api().energy_file(P.energy)
        out[r["name"]] = _run(P, t, r["kind"], r["nsteps"], r["liters"], r.get("params", {}))
    out["names"] = _api().registered_energies()
    return out


if __name__ == "__main__":
    case, args = sys.argv[1], json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    result = globals()["case_" + case](args)
    sys.stdout.flush()
    print(json.dumps(result))
