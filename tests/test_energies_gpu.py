"""GPU parity tests (-m gpu) for every registered energy other than the headline one: each stage of the HIP
path against the CPU oracle through the C ABI, then GN and LM trajectories.  Same bar as
test_image_warping_gpu.py: 1e-5 relative in float, 1e-12 on double costs."""
import os

import numpy as np
import pytest

from opt_amd import api, workloads as wl
import parity_cases as pc
from helpers import assert_close, active_mask, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

def _raptor(double):
    """The reference's ARAP example mesh (examples/data/raptor_simplify2k.off + .mrk, frozen as tests/fixtures/raptor2k_mesh.npz):
    irregular valence 3..12, 12108 half-edges, 11 landmark constraints pulled 30 % of the way."""
    import os
    from opt_amd import io
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "raptor2k_mesh.npz"))
    return io.arap_problem_from_mesh(z["vertices"], z["faces"].tolist(), z["marker_index"], z["marker_position"], double=double, alpha=0.3)


def _poisson_real(double):
    """poisson_image_editing on the reference example's own images (examples/data/poisson0.png, poisson1.png, poisson_mask.png sampled
    every 4th pixel, tests/fixtures/poisson_real_112x80.npz), assembled like CombinedSolver.h:66-90: alpha = 255, M = 0 where the mask is 255."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "poisson_real_112x80.npz"))
    ft = np.float64 if double else np.float32
    H, W = z["mask"].shape
    alpha = np.full((H, W, 1), 255.0)
    X = np.concatenate([z["base"].astype(np.float64), alpha], -1)
    T = np.concatenate([z["inserted"].astype(np.float64), alpha], -1)
    M = np.where(z["mask"] == 255, 0.0, 255.0)
    return wl.Problem("poisson_image_editing", (W, H), [X.astype(ft), T.astype(ft), M.astype(ft)], (0,), double)


CASES = {
    "poisson": lambda double: wl.poisson_image_editing(70, 45, double=double, seed=2),
    "poisson_tiny": lambda double: wl.poisson_image_editing(5, 3, double=double, seed=4),
    "poisson_real": _poisson_real,
    "laplacian": lambda double: wl.laplacian(67, 33, seed=1),
    "curveFitting": lambda double: wl.curve_fitting(200, double=double),
    "arap": lambda double: wl.arap_mesh_deformation(23, 17, double=double, seed=3, perturb=0.01),
    "arap_rest": lambda double: wl.arap_mesh_deformation(12, 9, double=double),
    "arap_raptor": _raptor,
    "sfs": lambda double: wl.shape_from_shading(40, 32, double=double, seed=6, holes=True, noise=2e-3),
    "sfs_clean": lambda double: wl.shape_from_shading(33, 21, double=double, seed=7),
    # the functor engine (stencil_engine.h)
    "flow": lambda double: wl.optical_flow(37, 26, double=double, seed=2, init_flow=1.2),
    "flow_zero_init": lambda double: wl.optical_flow(24, 31, double=double, seed=3),          # integer sample positions: floor == ceil
    "intrinsic": lambda double: wl.intrinsic_image_decomposition(29, 23, double=double, seed=4),
    "volumetric": lambda double: wl.volumetric_mesh_deformation(9, 7, 5, double=double, seed=5, perturb=0.05),
    "volumetric_rest": lambda double: wl.volumetric_mesh_deformation(6, 6, 6, double=double),
    # the graph functor engine (graph_engine.h)
    "cotangent": lambda double: wl.cotangent_mesh_smoothing(19, 13, double=double, seed=6),
    "embedded": lambda double: wl.embedded_mesh_deformation(17, 11, double=double, seed=7, perturb=0.03),
    "embedded_rest": lambda double: wl.embedded_mesh_deformation(9, 9, double=double),
    "robust": lambda double: wl.robust_nonrigid_alignment(15, 12, double=double, seed=8, perturb=0.03),
}


def _envelopes():
    """{case_kind: (largest relative diameter of the frozen legal oracle runs' cost over the trajectory, relative spread of their final unknowns)}"""
    import json
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "float_envelopes.json")
    out = {}
    for k, e in json.load(open(p)).items():
        runs = list(e["runs"].values()); a = e["runs"]["exact-order plain"]; s = max(abs(a[0]), 1e-300)
        n = min(len(c) for c in runs)
        out[k] = (max((max(c[i] for c in runs) - min(c[i] for c in runs)) / max(abs(a[i]), 1e-7 * s) for i in range(n)), e["x_spread"])
    return out


ENVELOPES = _envelopes()


def _cases():
    out = []
    for name in sorted(CASES):
        for double in (False, True):
            if name == "laplacian" and double:
                continue   # the energy declares fixed `float` images (tests/minimal/laplacian.t)
            out.append(pytest.param(name, double, id=f"{name}-{'f64' if double else 'f32'}"))
    return out


@pytest.mark.parametrize("name,double", _cases())
def test_cost_jtf_diag_jtjp(oracle_lib, name, double):
    import torch
    P = CASES[name](double)
    tol = 1e-11 if P.double else 3e-5
    o = oracle_solver(oracle_lib, P)
    g = hip_solver(P)
    dev = api.to_device(P)
    c_ref, c_gpu = o.eval_cost(P.params), g.eval_cost(dev)
    assert abs(c_gpu - c_ref) <= (1e-12 if P.double else 1e-5) * abs(c_ref) + 1e-30
    f_ref, d_ref = o.eval_jtf(P.params)
    f_gpu, d_gpu = g.eval_jtf(dev)
    act = active_mask(P)
    assert rel_err(f_gpu.cpu().numpy()[act], f_ref[act]) < tol
    assert rel_err(d_gpu.cpu().numpy()[act], d_ref[act]) < tol
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(o.n) * act).astype(o.dtype)
    Av_ref = o.apply_jtj(P.params, v)
    Av_gpu, dot = g.apply_jtj(dev, torch.from_numpy(v).cuda())
    assert rel_err(Av_gpu.cpu().numpy(), Av_ref) < tol
    assert abs(dot - float(v.astype(np.float64) @ Av_ref.astype(np.float64))) <= 10 * tol * abs(dot) + 1e-30
    g.close(); o.close()


@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("name,double", _cases())
def test_trajectory(oracle_lib, name, double, kind):
    c = pc.energies_trajectory(name, double, kind)      # (CASES[name], 4 x 12)
    P = c.problem()
    kw = c.settings()
    o = oracle_solver(oracle_lib, P, kind, **kw)
    g = hip_solver(P, kind, **kw)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    ctol = 1e-10 if P.double else 1e-5
    xtol = 1e-9 if P.double else 2e-5
    if name == "intrinsic" and P.double:
        # weights of 500 / 1000 / 10000 on differences of ~0.02 plus the (|dr| + 1e-7)^(-0.6) re-weighting make the system ill-conditioned (unpreconditioned, 12 PCG
        # iterations, far from converged): the oracle's own legal runs (sum order, fma) end 9.4e-9 apart in the cost and 2.6e-8 in the unknowns -- no difference in pow is
        # needed to explain the library's 2.2e-9; the bar in force is twice that spread per step (tests/golden/parity_bars.json, parity_envelopes.json)
        ctol, xtol = 1e-8, 1e-7
    if not P.double:
        # Float: where legal runs of the reference's own arithmetic (reference-order sums / scatter order under several seeds, plain and fma build of the oracle; frozen
        # in tests/golden/float_envelopes.json by make_float_envelopes.py) end further apart than the contract, twice their diameter is the bar -- a measured yardstick
        # per case: 1e-5 for most, 2.6e-4 for curveFitting LM (cos / sin of ~600 rad), 2e-4 for cotangent GN (float atomics in no defined order), 3e-2 for intrinsic GN.
        env = ENVELOPES.get(f"{name}_{kind}")
        if env is not None:
            ctol, xtol = max(ctol, 2.0 * env[0]), max(xtol, 2.0 * env[1])
    scale = max(abs(o.cost()), 1e-300)
    assert_close("cost0", g.cost(), o.cost(), 1e-12 if P.double else 1e-5, floor=scale, double=P.double)
    step = 0
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        step += 1
        # costs are compared relative to the initial cost: a converged energy can be ~0 (curve fit)
        assert_close("cost", g.cost(), o.cost(), ctol, floor=1e-7 * scale, double=P.double, step=step)
        if not a:
            break
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, xtol, absolute=True, double=P.double)
    g.close(); o.close()


def test_minimal_graph_only_known_answer():
    """Reference tests/minimal_graph_only/main.cpp:43-61, 88-90: double precision, GN defaults,
    unknowns (99.7, 101.6) must reach the generator parameters (100, 102)."""
    P = wl.curve_fitting(512, double=True)
    dev = api.to_device(P)
    g = api.Solver(api.energy_file("curveFitting"), "gaussNewtonGPU", P.dims, double=True)
    g.solve(dev)
    a, b = dev[0].cpu().numpy().reshape(-1)
    assert abs(a - 100.0) < 1e-8 and abs(b - 102.0) < 1e-8
    assert g.cost() < 1e-10
    g.close()


def test_minimal_laplacian_solve():
    """Reference tests/minimal/main.cpp: 512^2 random target, GN defaults (10 x 10); the solve must smooth the
    image (cost falls monotonically) and leave it finite."""
    import torch
    P = wl.laplacian(512, 512)
    dev = api.to_device(P)
    g = api.Solver(api.energy_file("laplacian"), "gaussNewtonGPU", P.dims)
    g.init(dev); costs = [g.cost()]
    while g.step(dev):
        costs.append(g.cost())
    assert len(costs) == 11 and all(b <= a * (1 + 1e-6) for a, b in zip(costs, costs[1:])) and costs[-1] < 0.2 * costs[0]
    assert torch.isfinite(dev[0]).all()
    g.close()


def test_create_delete_cycle():
    """Reference tests/create_delete_cycle/main.cpp:22-31: repeated ProblemPlan / PlanFree must not leak or crash."""
    import torch
    api.Solver(api.energy_file("laplacian"), "gaussNewtonGPU", (512, 512)).close()      # warm-up cycle: code objects, queues and the runtime's pools exist (as in the C++ caller)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(200):
        s = api.Solver(api.energy_file("laplacian"), "gaussNewtonGPU", (512, 512))
        s.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 * 1024 * 1024


def test_plan_failures_return_null():
    with pytest.raises(RuntimeError):
        api.Solver(api.energy_file("image_warping"), "gradientDescentGPU", (8, 8))      # o.t:122
    with pytest.raises(RuntimeError):
        api.Solver("/nonexistent/image_warping.t", "gaussNewtonGPU", (8, 8))


@pytest.mark.parametrize("double", [False, True])
def test_poisson_single_kernel_iteration_matches_three_kernel_loop(double, monkeypatch):
    """march_pcgIter<PoissonMarchOp> (whole PCG iteration in one launch, A p recomputed, r rebuilt from the p ring, the p0 = r0 / 4 start-up quirk carried through
    the beta-numerator expansion) against the Step1 / Step2 / Step3 loop over 150 iterations, odd and even image sizes."""
    P = wl.poisson_image_editing(333, 257, double=double, seed=9)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("OPT_AMD_ONEKERNEL", mode)
        g = hip_solver(P, nIterations=1, lIterations=150)
        g.enable_trace()
        dev = api.to_device(P)
        g.init(dev); g.step(dev)
        res[mode] = (g.cost(), device_unknowns(P, dev), g.trace())
        g.close()
    assert abs(res["1"][0] - res["0"][0]) <= (1e-9 if double else 1e-5) * abs(res["0"][0])
    assert rel_err(res["1"][1], res["0"][1]) < (1e-9 if double else 1e-5)
    # alphaNumerator / alphaDenominator / betaNumerator of the first iterations: the quirk shows up exactly there
    np.testing.assert_allclose(res["1"][2][:5, 2:5], res["0"][2][:5, 2:5], rtol=1e-9 if double else 1e-4)


@pytest.mark.parametrize("grid", [(41, 29), (40, 30)])      # vertex counts 1189 (one vertex per thread in PCGStep3) and 1200 (a multiple of 4: whole 16-byte packs)
@pytest.mark.parametrize("kind", ["gaussNewtonGPU", "LMGPU"])
@pytest.mark.parametrize("double", [False, True])
def test_arap_symmetric_graph_path_matches_edge_list_path(double, kind, grid, monkeypatch):
    """Round 3: on a graph that carries every edge in both directions (every mesh of the reference's examples) J^T J p walks the out-lists only and reads one 64-byte record
    per neighbour (arap_applySym, PCGStep3 writing the records); OPT_AMD_ARAP_SYM=0 keeps the edge-list gather (arap_applyFused).  Same trajectory, and the timer table shows
    which kernels ran."""
    P = wl.arap_mesh_deformation(grid[0], grid[1], double=double, seed=5, perturb=0.01)
    res = {}
    if grid[0] == 40:
        monkeypatch.setenv("OPT_AMD_ARAP_VGRID", "8")      # 10 vertex groups on 8 workgroups: the XCD-aware group order with an uneven last eighth and a second trip
    for mode in ("1", "0"):
        monkeypatch.setenv("OPT_AMD_ARAP_SYM", mode)
        g = hip_solver(P, kind, timing=True, nIterations=3, lIterations=40)
        dev = api.to_device(P)
        g.init(dev); c = [g.cost()]
        while g.step(dev):
            c.append(g.cost())
        res[mode] = (c, device_unknowns(P, dev), g.kernel_timings()); g.close()
    assert "vertexRecords" in res["1"][2] and "vertexRecords" not in res["0"][2]
    assert "packDerivativeRows" in res["0"][2] and "packDerivativeRows" not in res["1"][2]
    # (float: three steps of 40 iterations take the cost from 2.2 to 3e-4 -- residuals of 1e-4 formed from coordinates of order 1 carry four digits)
    # ... and the float LM trajectory magnifies rounding differences (its double run agrees to 1e-8; each path is compared with the oracle in test_trajectory)
    np.testing.assert_allclose(res["1"][0], res["0"][0], rtol=1e-9 if double else 1e-5, atol=0 if double else 2e-7 * res["0"][0][0])      # a float cost is not resolved below ~1e-7 of the sums it started from
    assert rel_err(res["1"][1], res["0"][1]) < (1e-8 if double else (5e-3 if kind == "LMGPU" else 2e-5))


@pytest.mark.parametrize("double", [False, True])
def test_arap_asymmetric_graph_keeps_the_edge_list_path(oracle_lib, double):
    """A graph with half-edges whose reverse is missing (the API accepts any edge list) must not take the symmetric-graph shortcut: stages and trajectory against the oracle."""
    import torch
    P = wl.arap_mesh_deformation(23, 17, double=double, seed=3, perturb=0.01)
    heads, tails = P.params[7], P.params[8]
    keep = np.ones(len(heads), dtype=bool)
    keep[np.arange(5, len(heads), 7)] = False            # every seventh half-edge dropped: most of them leave their reverse behind
    P.params[7] = np.ascontiguousarray(heads[keep]); P.params[8] = np.ascontiguousarray(tails[keep])
    P.params[6] = np.array(int(keep.sum()), dtype=np.int32)
    tol = 1e-11 if double else 3e-5
    o = oracle_solver(oracle_lib, P); g = hip_solver(P, timing=True)
    dev = api.to_device(P)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(o.n).astype(o.dtype)
    Av_ref = o.apply_jtj(P.params, v)
    Av_gpu, _ = g.apply_jtj(dev, torch.from_numpy(v).cuda())
    assert rel_err(Av_gpu.cpu().numpy(), Av_ref) < tol
    assert "packVertexRecords" not in g.kernel_timings()
    g.close(); o.close()
    kw = dict(nIterations=3, lIterations=12)
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", **kw); g = hip_solver(P, "gaussNewtonGPU", **kw)
    Pref = P.clone(); dev = api.to_device(P)
    o.init(Pref.params); g.init(dev)
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        assert_close("cost", g.cost(), o.cost(), 1e-10 if double else 1e-5, double=double)
        if not a:
            break
    g.close(); o.close()


@pytest.mark.parametrize("hub,expect_planes", [(16, True), (17, False), (40, False)])
def test_arap_high_valence_vertex_and_the_ell_width(oracle_lib, hub, expect_planes):
    """Round 6: the symmetric-graph path stores the out-lists ELL-wise, one column per neighbour of the longest list (kEllMax = 16).  A mesh plus one hub vertex joined to
    `hub` others (both directions): 16 neighbours still take the plane gather (ELL width 16, most vertices use 4-6 columns of it), 17 or 40 send the graph to the edge-list
    gather.  Either way J^T J p and a 2 x 12 trajectory against the oracle."""
    import torch
    P = wl.arap_mesh_deformation(19, 13, double=True, seed=5, perturb=0.01)
    heads, tails = list(P.params[7]), list(P.params[8])
    n = 19 * 13
    h = 7 * 19 + 9                                   # an interior vertex
    have = {t for a, t in zip(heads, tails) if a == h}
    extra = [v for v in range(0, n, 3) if v != h and v not in have][:hub - len(have)]
    for v in extra:
        heads += [h, v]; tails += [v, h]
    P.params[7] = np.ascontiguousarray(np.array(heads, dtype=np.int32)); P.params[8] = np.ascontiguousarray(np.array(tails, dtype=np.int32))
    P.params[6] = np.array(len(heads), dtype=np.int32)
    assert sum(1 for a in heads if a == h) == hub
    o = oracle_solver(oracle_lib, P); g = hip_solver(P, timing=True)
    dev = api.to_device(P)
    v = np.random.default_rng(5).standard_normal(o.n).astype(o.dtype)
    Av_gpu, _ = g.apply_jtj(dev, torch.from_numpy(v).cuda())
    assert rel_err(Av_gpu.cpu().numpy(), o.apply_jtj(P.params, v)) < 1e-11
    assert ("packVertexRecords" in g.kernel_timings()) == expect_planes, g.kernel_timings().keys()
    g.close(); o.close()
    kw = dict(nIterations=2, lIterations=12)
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", **kw); g = hip_solver(P, "gaussNewtonGPU", **kw)
    Pref = P.clone(); dev = api.to_device(P)
    o.init(Pref.params); g.init(dev)
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
        if not a:
            break
    g.close(); o.close()


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("double", [False, True])
def test_volumetric_on_both_kernel_sets(oracle_lib, double, mode, monkeypatch):
    """volumetric_mesh_deformation is ARAP on the 6-neighbour lattice graph and runs on ARAP's kernel set by default (OPT_AMD_VOLUMETRIC_ARAP=1: generated half-edge list,
    record gather, two-kernel iteration); 0 keeps the stencil functor engine.  Both against the oracle's own (stencil) statement of the energy: J^T J p and a GN trajectory."""
    import torch
    monkeypatch.setenv("OPT_AMD_VOLUMETRIC_ARAP", mode)
    P = wl.volumetric_mesh_deformation(8, 6, 4, double=double, seed=5, perturb=0.05)      # 192 voxels: a multiple of 4, the two-kernel iteration's form
    tol = 1e-11 if double else 3e-5
    o = oracle_solver(oracle_lib, P); g = hip_solver(P, timing=True)
    dev = api.to_device(P)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(o.n).astype(o.dtype)
    Av_ref = o.apply_jtj(P.params, v)
    Av_gpu, _ = g.apply_jtj(dev, torch.from_numpy(v).cuda())
    assert rel_err(Av_gpu.cpu().numpy(), Av_ref) < tol
    assert ("packVertexRecords" in g.kernel_timings()) == (mode == "1")
    g.close(); o.close()
    kw = dict(nIterations=3, lIterations=12)
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", **kw); g = hip_solver(P, "gaussNewtonGPU", **kw)
    Pref = P.clone(); dev = api.to_device(P)
    o.init(Pref.params); g.init(dev)
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        assert_close("cost", g.cost(), o.cost(), 1e-10 if double else 1e-5, double=double)
        if not a:
            break
    g.close(); o.close()


def test_arap_path_is_deterministic():
    """The ARAP kernel set uses no atomics (edge pass -> records, vertex pass gathers sorted lists) for J^T F as well as J^T J p:
    two solves of the same problem give the same bits (the reference's scatter kernels do not)."""
    outs = []
    for _ in range(2):
        P = _raptor(False)
        g = hip_solver(P, "gaussNewtonGPU", nIterations=3, lIterations=30)
        dev = api.to_device(P)
        g.init(dev)
        while g.step(dev):
            pass
        outs.append((g.cost(), device_unknowns(P, dev)))
        g.close()
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", ["cotangent", "embedded", "robust"])
def test_graph_functor_engine_is_deterministic_and_scatter_mode_agrees(oracle_lib, name, monkeypatch):
    """Graph functor engine (graph_engine.h): the default gather mode (records + sorted incidence lists, no atomics) gives the same bits
    in two solves; the scatter mode (OPT_AMD_GRAPH_GATHER=0: atomics, as in the reference) agrees with it to summation-order tolerance."""
    def run():
        P = CASES[name](False)
        g = hip_solver(P, "gaussNewtonGPU", nIterations=3, lIterations=15)
        dev = api.to_device(P)
        g.init(dev)
        while g.step(dev):
            pass
        out = (g.cost(), device_unknowns(P, dev))
        g.close()
        return out
    a, b = run(), run()
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    monkeypatch.setenv("OPT_AMD_GRAPH_GATHER", "0")
    c = run()
    env = ENVELOPES[f"{name}_gaussNewtonGPU"]      # two scatter orders are two legal runs: the measured spread of such runs (tests/golden/float_envelopes.json), never below the contract
    assert abs(c[0] - a[0]) <= max(1e-5, 2.0 * env[0]) * abs(a[0])
    assert rel_err(c[1], a[1]) < max(2e-5, 2.0 * env[1])
