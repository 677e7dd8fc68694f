"""GPU parity tests (-m gpu) of the one-workgroup ARAP linear solve (opt_amd/csrc/arap_onchip.h, arap_onchipPcg<T, V, LMV>): arap_mesh_deformation and
volumetric_mesh_deformation, Gauss-Newton and Levenberg-Marquardt, solver parameter amd_onchip = 5.

By default a mesh energy runs two launches per PCG iteration (arap_flatStepPlanes + arap_applyEll).  With amd_onchip = 5 a symmetric graph whose vertices have at most 16
neighbours and fit a variant (V vertices per lane of one workgroup of up to 512 threads: V * 512 vertices) runs its whole linear solve as one launch of one workgroup.
Everything here is stepped beside the CPU oracle:
  * the opt-in gate (level 5 on chip; the default and level 4 keep the two-kernel loop);
  * every offered variant (ARAP_VARIANTS) on grid meshes whose vertex counts sit on the edges: one vertex pair, a partial wave, 64 / 65, 512 / 513 (first V = 2 size),
    1023 / 1024 / 1025 (one more than the largest variant: streams, and describe() says why);
  * the reference's own graphs: small_armadillo (130 vertices) and its sqrt(3) subdivision (386), tests/golden/meshes/armadillo_mesh.npz;
  * the LM controls (reset period, q tolerance, lIterations) of tests/test_lm_controls_gpu.py::test_arap_two_kernel_lm_iteration_controls, the early-out message, rejected steps;
  * graph shapes: a vertex with exactly 16 neighbours (on chip), 17 (streams), a missing reverse edge (streams);
  * the same iterates as the two-kernel loop (unknowns and trace rows), determinism, volumetric_mesh_deformation, Opt_ProblemSolve.
Bars (the project's for ARAP, tests/test_lm_controls_gpu.py): double 1e-10 on costs / 1e-9 on the unknowns / 1e-8 on the LM radius; float 1e-5 on costs / 1e-3 on the radius.
The kernel has no wait that could time out, so there is no time-out test.
"""
import ctypes
import os

import numpy as np
import pytest

from opt_amd import api, io, workloads as wl
from helpers import assert_close, device_unknowns, flat_unknowns, hip_solver, oracle_solver, rel_err

pytestmark = pytest.mark.gpu

# (precision, vertices per lane, Levenberg-Marquardt) of every kernel arap_onchipPcg<T, V, LMV> the library offers (tests/test_onchip_arap_resources.py checks that this
# is exactly the set instantiated).  A variant serves up to V * 512 vertices.
ARAP_VARIANTS = [("float", 1, False), ("float", 1, True), ("float", 2, False), ("float", 2, True), ("double", 1, False), ("double", 1, True), ("double", 2, False)]
LANES = 512
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "armadillo_mesh.npz")
RAPTOR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "raptor2k_mesh.npz")


def _largest(double, lm):
    return LANES * max(v for p, v, l in ARAP_VARIANTS if p == ("double" if double else "float") and l == lm)


def _variant(double, lm, n):
    return min(v for p, v, l in ARAP_VARIANTS if p == ("double" if double else "float") and l == lm and n <= v * LANES)


def _check_path(g, P, lm, expect_onchip, why=None):
    t = g.kernel_timings()
    assert ("PCGSolveOnChip" in t) == expect_onchip, t.keys()
    assert ("PCGStep1" in t) == (not expect_onchip), t.keys()
    assert g.on_chip_status() == (1 if expect_onchip else 0)
    d = g.describe()
    if expect_onchip:
        n = int(np.prod(P.dims))
        assert d["path"] == "on-chip" and d["workgroups"] == "1" and d["vertices"] == str(n), d
        assert d["variant"] == "arap_onchipPcg<%s, %d, %s>" % ("double" if P.double else "float", _variant(P.double, lm, n), "LM" if lm else "GN"), d
    else:
        assert d["path"] == "launch-per-iteration" and (why is None or why in d["why_not_on_chip"]), d


def _pair(oracle_lib, P, nsteps, liters, cost_tol, x_tol, expect_onchip=True, level=5, why=None):
    """Gauss-Newton, step by step beside the oracle."""
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", nIterations=nsteps, lIterations=liters)
    kw = {} if level is None else {"amd_onchip": level}
    g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=nsteps, lIterations=liters, **kw)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    costs = [(o.cost(), g.cost())]
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b
        costs.append((o.cost(), g.cost()))
        print("cost", len(costs) - 1, g.cost(), o.cost(), abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-12 * scale))
        assert_close("cost", g.cost(), o.cost(), cost_tol, floor=1e-12 * scale, double=P.double, step=len(costs) - 1)
        if not a:
            break
    _check_path(g, P, False, expect_onchip, why)
    if x_tol is not None:
        assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, x_tol, absolute=True, double=P.double)
    g.close(); o.close()
    return costs


def _side_by_side(oracle_lib, P, nsteps, liters, cost_tol, x_tol, radius_tol, expect_onchip=True, level=5, why=None, **controls):
    """Levenberg-Marquardt, step by step beside the oracle (tests/test_lm_controls_gpu.py::_side_by_side with the plan opted in).  Returns [(oracle, hip) cost, oracle radius]."""
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=nsteps, lIterations=liters, **controls)
    kw = dict(controls) if level is None else dict(controls, amd_onchip=level)
    g = hip_solver(P, "LMGPU", timing=True, nIterations=nsteps, lIterations=liters, **kw)
    dev = api.to_device(P)
    Pref = P.clone()
    o.init(Pref.params); g.init(dev)
    scale = max(abs(o.cost()), 1e-300)
    hist = [(o.cost(), g.cost(), o.trust_region_radius())]
    while True:
        a, b = o.step(Pref.params), g.step(dev)
        assert a == b, (a, b, hist)
        hist.append((o.cost(), g.cost(), o.trust_region_radius()))
        print("cost", len(hist) - 1, g.cost(), o.cost(), abs(g.cost() - o.cost()) / max(abs(o.cost()), 1e-12 * scale), "radius", g.trust_region_radius(), o.trust_region_radius())
        assert_close("cost" if len(hist) <= 2 else "cost_later", g.cost(), o.cost(), cost_tol, floor=1e-12 * scale, double=P.double, step=len(hist) - 1)
        assert_close("radius", g.trust_region_radius(), o.trust_region_radius(), radius_tol, double=P.double)
        if not a:
            break
    _check_path(g, P, True, expect_onchip, why)
    if x_tol is not None:
        assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, x_tol, absolute=True, double=P.double)
    g.close(); o.close()
    return hist


# ---- the opt-in gate (fails without the feature) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm", [False, True])
def test_level_5_keeps_the_linear_solve_in_one_workgroup(oracle_lib, lm):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    if lm:
        _side_by_side(oracle_lib, P, 2, 6, 1e-10, 1e-9, 1e-8)
    else:
        _pair(oracle_lib, P, 2, 6, 1e-10, 1e-9)


@pytest.mark.parametrize("level", [None, 4])
@pytest.mark.parametrize("lm", [False, True])
def test_the_default_and_level_4_keep_the_two_kernel_loop(oracle_lib, lm, level):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    g = hip_solver(P, "LMGPU" if lm else "gaussNewtonGPU", timing=True, nIterations=2, lIterations=6, **({} if level is None else {"amd_onchip": level}))
    dev = api.to_device(P)
    g.init(dev)
    while g.step(dev):
        pass
    t = g.kernel_timings()
    assert "PCGStep2+PCGStep3" in t and "PCGStep1" in t and "PCGSolveOnChip" not in t, t.keys()
    assert g.on_chip_status() == 0
    g.close()
    if lm:
        _side_by_side(oracle_lib, P, 2, 6, 1e-10, 1e-9, 1e-8, expect_onchip=False, level=level, why="amd_onchip=5 was not set")
    else:
        _pair(oracle_lib, P, 2, 6, 1e-10, 1e-9, expect_onchip=False, level=level, why="amd_onchip=5 was not set")


# ---- every offered variant, on the edges of the vertex counts ---------------------------------------------------------------------------------------------------------------
# one vertex pair; one partial wave; one full wave; one lane into the second wave; the largest V = 1 size and the first V = 2 size; around the largest V = 2 size
GRIDS = [(2, 1), (7, 9), (64, 1), (65, 1), (32, 16), (27, 19), (31, 33), (32, 32), (41, 25)]


def _mesh(nx, ny, double):
    return wl.arap_mesh_deformation(nx, ny, double=double, seed=nx * 7 + ny, perturb=0.01)


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_variants_gn(oracle_lib, nx, ny, double):
    """2 x 6 everywhere but on the two-vertex mesh in float, which runs 2 x 1.  Both of its vertices carry a handle and the first step takes the cost from 1.1e-3 to
    2.3e-7: with more than one PCG iteration per step that remainder is float noise in the REFERENCE's arithmetic already -- the CPU oracle in float against the CPU oracle
    in double after step 1 / step 2: 1 iteration 1e-8 / 2e-7, 2 iterations 1e-7 / 3e-4, 3: 4e-7 / 9e-3, 4: 3e-6 / 3e-3, 6: 4e-3 / 3e-7, 8: 2e-3 / 2e-7 -- so only the
    one-iteration solve can be held to the float bar of 1e-5.  The loop itself runs on this mesh in double (1e-15 from the oracle) and in float on every other size."""
    fits = nx * ny <= _largest(double, False)
    liters = 1 if (nx * ny == 2 and not double) else 6
    _pair(oracle_lib, _mesh(nx, ny, double), 2, liters, 1e-10 if double else 1e-5, 1e-9 if double else None, expect_onchip=fits, why="too many vertices")


@pytest.mark.parametrize("period", [10, 2])
@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_variants_lm(oracle_lib, nx, ny, double, period):
    """(float: q_tolerance = -1e9, never -- in float the zeta test can sit on a knife's edge, tests/test_onchip_general_gpu.py::test_variants_lm_float; the decisions are
    pinned in double and in test_lm_controls)"""
    fits = nx * ny <= _largest(double, True)
    kw = dict(residual_reset_period=period) if double else dict(residual_reset_period=period, q_tolerance=-1e9)
    _side_by_side(oracle_lib, _mesh(nx, ny, double), 2, 6, 1e-10 if double else 1e-5, 1e-9 if double else None, 1e-8 if double else 1e-3, expect_onchip=fits,
                  why="too many vertices", **kw)


def test_every_variant_is_reached_by_the_grids():
    reached = set()
    for nx, ny in GRIDS:
        for double in (True, False):
            for lm in (True, False):
                if nx * ny <= _largest(double, lm):
                    reached.add(("double" if double else "float", _variant(double, lm, nx * ny), lm))
    assert reached == set(ARAP_VARIANTS)
    for double in (True, False):
        for lm in (True, False):      # the largest size of every (precision, mode) and one vertex more
            sizes = {nx * ny for nx, ny in GRIDS}
            assert _largest(double, lm) in sizes and any(s == _largest(double, lm) + 1 for s in sizes)


# ---- the reference's own graphs ----------------------------------------------------------------------------------------------------------------------------------------------
def _armadillo(subdivided, double):
    m = np.load(GOLDEN)
    if subdivided:
        return io.arap_problem_from_mesh(m["vertices_sub"], m["faces_sub"].tolist(), m["marker_index"], m["marker_position"], double=double, alpha=0.1)
    return io.arap_problem_from_mesh(m["vertices"], m["faces"].tolist(), m["marker_index_coarse"], m["marker_position"], double=double, alpha=0.1)


@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("subdivided", [False, True])
def test_armadillo_gn(oracle_lib, subdivided, double):
    """small_armadillo (130 vertices) and the 386-vertex mesh the example solves on (one sqrt(3) subdivision, tests/golden/meshes/make_armadillo_mesh.py), handles at
    alpha = 0.1, 3 x 25."""
    P = _armadillo(subdivided, double)
    assert P.dims[0] == (386 if subdivided else 130)
    _pair(oracle_lib, P, 3, 25, 1e-10 if double else 1e-5, 1e-9 if double else None)


@pytest.mark.parametrize("subdivided", [False, True])
def test_armadillo_lm_double(oracle_lib, subdivided):
    _side_by_side(oracle_lib, _armadillo(subdivided, True), 3, 25, 1e-10, 1e-9, 1e-8)


def test_raptor_streams_no_variant_serves_2000_vertices(oracle_lib):
    m = np.load(RAPTOR)
    P = io.arap_problem_from_mesh(m["vertices"], m["faces"].tolist(), m["marker_index"], m["marker_position"], double=False, alpha=0.1)
    assert P.dims[0] == 2000 > _largest(False, False)
    _pair(oracle_lib, P, 1, 5, 1e-5, None, expect_onchip=False, why="too many vertices")


# ---- LM controls -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [True, False])
@pytest.mark.parametrize("period,qtol,liters", [(1, None, 6), (2, None, 10), (3, 0.5, 10), (10, None, 10), (10, 0.05, 12), (4, 0.0, 9), (7, None, 23), (5, 5.0, 10)])
def test_lm_controls(oracle_lib, period, qtol, liters, double):
    """The list of test_arap_two_kernel_lm_iteration_controls: resets inside the solve, early-outs on, next to and between resets.  No variant serves the 1044 vertices of
    36 x 29: float runs on 30 x 29 = 870 (V = 2), double -- whose LM variant ends at 512 vertices -- on 23 x 22 = 506."""
    P = wl.arap_mesh_deformation(23, 22, double=True, perturb=0.01) if double else wl.arap_mesh_deformation(30, 29, double=False, perturb=0.01)
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    if double:
        _side_by_side(oracle_lib, P, 4, liters, 1e-10, 1e-9, 1e-8, **kw)
    else:
        _side_by_side(oracle_lib, P, 3, liters, 1e-5, None, 1e-3, **kw)


def test_verbose_run_prints_the_early_out_and_keeps_the_bits(oracle_lib, capfd):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    silent = _side_by_side(oracle_lib, P, 3, 10, 1e-10, 1e-9, 1e-8, q_tolerance=0.5)
    capfd.readouterr()
    g = hip_solver(P, "LMGPU", verbosity=1, nIterations=3, lIterations=10, q_tolerance=0.5, amd_onchip=5)
    dev = api.to_device(P)
    g.init(dev)
    costs = [g.cost()]
    while g.step(dev):
        costs.append(g.cost())
    assert g.on_chip_status() == 1
    g.close()
    ctypes.CDLL(None).fflush(None)      # the library prints through C stdio
    out = capfd.readouterr().out
    assert costs == [c[1] for c in silent][:len(costs)], (costs, silent)
    assert "breaking at iteration" in out, out[-2000:]


def test_rejected_steps_shrink_the_radius_and_restore_the_unknowns(oracle_lib):
    """min_relative_decrease = 0.95 on a heavily perturbed mesh with short linear solves: the CPU oracle rejects steps 2 .. 7 (REVERT, solver.t:1148-1157; the radius falls
    from 3e4 to 1.4e-2) and accepts step 8 -- found on the oracle first; the assertion below keeps the test from passing empty."""
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.6, seed=1)
    hist = _side_by_side(oracle_lib, P, 8, 6, 1e-10, 1e-9, 1e-8, min_relative_decrease=0.95)
    rejected = [i for i in range(1, len(hist)) if hist[i][0] == hist[i - 1][0] and hist[i][2] < hist[i - 1][2]]
    assert len(rejected) >= 1, hist


# ---- graph shapes --------------------------------------------------------------------------------------------------------------------------------------------------------------
def _with_graph(P, nbrs):
    """the problem on the graph given as neighbour sets: half-edges grouped by head vertex, like createGraphFromNeighborLists"""
    heads = np.concatenate([np.full(len(s), v, dtype=np.int32) for v, s in enumerate(nbrs)])
    tails = np.concatenate([np.array(sorted(s), dtype=np.int32) for s in nbrs if s])
    P.params[6] = np.array(len(heads), dtype=np.int32); P.params[7] = heads; P.params[8] = tails
    return P


def _grid_neighbours(P):
    nb = [set() for _ in range(P.dims[0])]
    for h, t in zip(P.params[7], P.params[8]):
        nb[int(h)].add(int(t))
    return nb


def _hub(n_neighbours):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    nb = _grid_neighbours(P)
    hub = 4 * 12 + 5
    assert len(nb[hub]) == 6
    for v in range(P.dims[0]):
        if len(nb[hub]) == n_neighbours:
            break
        if v != hub and v not in nb[hub]:
            nb[hub].add(v); nb[v].add(hub)
    assert max(len(s) for s in nb) == n_neighbours
    return _with_graph(P, nb)


def test_a_vertex_with_16_neighbours_stays_on_chip(oracle_lib):
    _pair(oracle_lib, _hub(16), 2, 6, 1e-10, 1e-9)
    g = hip_solver(_hub(16), "gaussNewtonGPU", nIterations=1, lIterations=6, amd_onchip=5)
    dev = api.to_device(_hub(16))
    g.init(dev); g.step(dev)
    assert g.describe()["ell"] == "16", g.describe()
    g.close()


def test_a_vertex_with_17_neighbours_streams(oracle_lib):
    _pair(oracle_lib, _hub(17), 2, 6, 1e-10, 1e-9, expect_onchip=False, why="more than 16 neighbours")


def test_a_missing_reverse_edge_streams(oracle_lib):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    nb = _grid_neighbours(P)
    nb[40].discard(41)      # 40 -> 41 goes, 41 -> 40 stays
    _pair(oracle_lib, _with_graph(P, nb), 2, 6, 1e-10, 1e-9, expect_onchip=False, why="asymmetric graph")


# ---- the same iterates as the two-kernel loop; determinism -------------------------------------------------------------------------------------------------------------------
def test_same_iterates_as_the_two_kernel_loop():
    res = {}
    for level in (5, 1):
        P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
        g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=2, lIterations=20, amd_onchip=level)
        g.enable_trace()
        dev = api.to_device(P)
        g.solve(dev)
        assert ("PCGSolveOnChip" in g.kernel_timings()) == (level == 5)
        res[level] = (device_unknowns(P, dev), g.trace())
        g.close()
    assert rel_err(res[5][0], res[1][0]) <= 1e-9
    a, b = res[5][1], res[1][1]
    assert a.shape == b.shape == (40, 6), (a.shape, b.shape)
    assert np.array_equal(a[:, :2], b[:, :2])      # (outer step, PCG iteration)
    err = np.abs(a[:, 2:5] - b[:, 2:5]) / np.maximum(np.abs(b[:, 2:5]), 1e-300)
    print("largest relative difference of a trace entry:", err.max())
    assert err.max() <= 1e-9, (err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("kind,double", [("gaussNewtonGPU", False), ("LMGPU", True)])
def test_two_fresh_plans_give_the_same_bits(kind, double):
    res = []
    for _ in range(2):
        P = _armadillo(True, double)
        g = hip_solver(P, kind, nIterations=3, lIterations=25, amd_onchip=5)
        dev = api.to_device(P)
        g.init(dev)
        costs = [g.cost()]
        while g.step(dev):
            costs.append(g.cost())
        assert g.on_chip_status() == 1
        res.append((costs + [g.cost()], device_unknowns(P, dev)))
        g.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1])


# ---- volumetric_mesh_deformation on ARAP's kernels; Opt_ProblemSolve ----------------------------------------------------------------------------------------------------------
def test_volumetric_mesh_deformation(oracle_lib):
    P = wl.volumetric_mesh_deformation(6, 5, 4, double=True, perturb=0.01)
    _pair(oracle_lib, P, 2, 8, 1e-10, 1e-9)


def test_problem_solve_gives_the_costs_of_init_and_step(oracle_lib):
    P = wl.arap_mesh_deformation(12, 9, double=True, perturb=0.01)
    g = hip_solver(P, "gaussNewtonGPU", nIterations=4, lIterations=10, amd_onchip=5)
    dev = api.to_device(P)
    g.init(dev)
    while g.step(dev):
        pass
    stepped = (g.cost(), device_unknowns(P, dev))
    g.close()
    g = hip_solver(P, "gaussNewtonGPU", timing=True, nIterations=4, lIterations=10, amd_onchip=5)
    dev = api.to_device(P)
    g.solve(dev)
    assert g.kernel_timings()["PCGSolveOnChip"][0] == 4 and g.on_chip_status() == 1
    assert g.cost() == stepped[0] and np.array_equal(device_unknowns(P, dev), stepped[1])
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", nIterations=4, lIterations=10)
    Pref = P.clone()
    o.solve(Pref.params)
    assert_close("cost", g.cost(), o.cost(), 1e-10, double=True)
    assert_close("x", rel_err(device_unknowns(P, dev), flat_unknowns(Pref)), 0.0, 1e-9, absolute=True, double=True)
    g.close(); o.close()
