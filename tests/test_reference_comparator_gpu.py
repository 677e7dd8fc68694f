"""The HIP probes and the first PCG steps of a real solve against the reference's comparator maths (-m gpu).

Same fixtures, relations and compared sets as tests/test_reference_comparator_cpu.py.  Double plans are held to 1e-11 max|ref| per element against
the widened recording, float plans to 2e-5.  The GN steps (one iteration, lIterations = 1, 2, 3, double) run on the default path and with
OPT_AMD_ONCHIP=0, so the marching / on-chip kernels a real solve uses are checked, not only the streaming probes."""
import os

import numpy as np
import pytest

import reference_cases as rc
from opt_amd import api, workloads as wl
from helpers import device_unknowns, flat_unknowns, hip_solver
from test_reference_comparator_cpu import GOLDEN, REL, assert_elementwise, compared_rows, load_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_hip_operators_agree_with_the_comparator(name, double):
    import torch
    P, G = load_case(name)
    s = REL[P.energy]
    if double:
        P = rc.as_double(P)
    tol = 1e-11 if double else 2e-5
    rows = compared_rows(P)
    g = hip_solver(P)
    dev = api.to_device(P)
    cost = g.eval_cost(dev)
    jtf, _ = g.eval_jtf(dev)
    Av, _ = g.apply_jtj(dev, torch.from_numpy(G["v"].astype(np.float64 if double else np.float32)).cuda())
    g.close()
    assert abs(s["F"] * cost - float(G["F"])) <= tol * abs(float(G["F"]))
    assert_elementwise(s["b"] * jtf.cpu().numpy(), G["b"], rows, tol, "J^T F")
    assert_elementwise(s["A"] * Av.cpu().numpy(), G["jtj_v"], rows, tol, "J^T J v")


@pytest.mark.parametrize("path", ["default", "onchip_off"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_hip_first_pcg_steps_agree_with_the_comparator(monkeypatch, name, path):
    if path == "onchip_off":
        monkeypatch.setenv("OPT_AMD_ONCHIP", "0")
    P0, G = load_case(name)
    for k in (1, 2, 3):
        P = rc.as_double(P0)
        x0 = flat_unknowns(P)
        g = hip_solver(P, timing=True, nIterations=1, lIterations=k)
        dev = api.to_device(P)
        g.solve(dev)
        ran = g.kernel_timings()
        g.close()
        if P.energy == "arap_mesh_deformation":                 # graph energies: the streaming PCGStep1 family on either path
            assert "PCGStep1" in ran and "PCGSolveOnChip" not in ran, sorted(ran)
            assert ("packVertexRecords" in ran) == (name == "arap_raptor2k"), sorted(ran)      # ELL planes vs the edge-list gather of the hub
        elif path == "default":
            assert "PCGSolveOnChip" in ran, sorted(ran)
        else:
            assert "PCGIteration" in ran and "PCGSolveOnChip" not in ran, sorted(ran)
        rows = compared_rows(P)
        assert_elementwise(device_unknowns(P, dev) - x0, G[f"x{k}"], rows, 1e-11, f"x_{k}")


@pytest.mark.parametrize("double", [True, False], ids=["double", "float"])
def test_hip_image_warping_operators_agree_with_the_comparator(double):
    """comparator_iw_23x17.npz (Mask == 0): F = 2 cost, comparator -J^T F = -2 jtf, applyJTJ = 2 J^T J v, per element."""
    import torch
    G = np.load(GOLDEN)
    W, H = int(G["W"]), int(G["H"])
    P = wl.image_warping(W, H, random_state=19, mask_fraction=0.0, perturb=0.4)
    v = np.random.default_rng(4).standard_normal(3 * W * H).astype(np.float32)
    np.testing.assert_array_equal(v, G["v"])
    if double:
        P = rc.as_double(P)
    tol = 2e-5                            # the recording is the float build of the header
    to_flat = lambda a: np.concatenate([a[:, :2].reshape(-1), a[:, 2]])
    g = hip_solver(P)
    dev = api.to_device(P)
    cost = g.eval_cost(dev)
    jtf, _ = g.eval_jtf(dev)
    Av, _ = g.apply_jtj(dev, torch.from_numpy(v.astype(np.float64 if double else np.float32)).cuda())
    g.close()
    rows = slice(None)
    assert abs(2.0 * cost - float(G["F"])) <= tol * abs(float(G["F"]))
    assert_elementwise(-2.0 * jtf.cpu().numpy(), to_flat(G["minus_jtf"]), rows, tol, "J^T F")
    assert_elementwise(2.0 * Av.cpu().numpy(), to_flat(G["jtj_v"]), rows, tol, "J^T J v")
