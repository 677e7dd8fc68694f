"""CORROBORATION ONLY -- NOT A PIN.

The reference ships a hand-written CUDA comparator for image_warping whose per-variable maths is plain C++ in a header
(examples/image_warping/src/WarpingSolverEquations.h:9-349: evalFDevice, evalMinusJTFDevice, applyJTJDevice).  What that maths computes on the input
below was recorded once (tests/golden/make_reference_fixtures.py compiles the header where it lies with g++, against a throw-away stand-in for
<cuda_runtime.h>; nothing of it is copied into the repo) and is stored as data in tests/golden/reference_data/comparator_iw_23x17.npz.  This test checks the
relations SURVEY.md section 7 step 1 predicts at Mask == 0:
    comparator F          == 2 * Opt cost            (the comparator sums w r^2, Opt 1/2 sum r^2 with sqrt weights)
    comparator -J^T F     == 2 * oracle r0 = -2 J^T F
    comparator J^T J p    == 2 * oracle J^T J p
It corroborates that the oracle's residuals, Jacobian blocks and sign conventions are the ones the reference authors wrote by hand.
"""
import os

import numpy as np

from opt_amd import workloads as wl
from helpers import oracle_solver, rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data", "comparator_iw_23x17.npz")


def test_oracle_agrees_with_the_hand_written_comparator_maths(oracle_lib):
    G = np.load(GOLDEN)
    W, H = int(G["W"]), int(G["H"])
    assert (W, H) == (23, 17)
    P = wl.image_warping(W, H, random_state=19, mask_fraction=0.0, perturb=0.4)          # Mask == 0: the exact 2x relations hold
    v = np.random.default_rng(4).standard_normal(3 * W * H).astype(np.float32)
    np.testing.assert_array_equal(v, G["v"])                                              # the input the comparator was run on
    F = float(G["F"])
    rest = [G["minus_jtf"], G["jtj_v"]]
    to_flat = lambda a: np.concatenate([a[:, :2].reshape(-1), a[:, 2]])                   # comparator per-variable (x, y, angle) -> Opt's [O x N | a x N]
    o = oracle_solver(oracle_lib, P)
    cost = o.eval_cost(P.params)
    jtf, _ = o.eval_jtf(P.params)
    Av = o.apply_jtj(P.params, v)
    assert abs(F - 2.0 * cost) <= 2e-5 * abs(F)
    assert rel_err(to_flat(rest[0]), -2.0 * jtf) < 2e-5
    assert rel_err(to_flat(rest[1]), 2.0 * Av) < 2e-5
    o.close()


# ---- poisson, ARAP and SFS against the reference's comparator maths ------------------------------------------------------------------------------
# tests/golden/make_reference_fixtures.py compiles each comparator header twice (as written in float, and widened to double), runs it on the
# problems of tests/reference_cases.py and stores F, b = evalMinusJTFDevice, applyJTJDevice(v), the comparator's preconditioner (poisson, ARAP) or
# the diagonal of its applyJTJ read off 25 period-5 probes (SFS, after checking that its stencil reaches 2 pixels), and x_1..x_3 of a PCG run
# on its operator.  The widened recording is kept because it matches the float one to float rounding on every case; it is the reference here.
#
# Relations, with Opt's cost = 1/2 sum r^2, jtf = J^T F, A = J^T J (derived from the headers and confirmed on every case):
#   poisson  F = 2 cost, b = -1/2 jtf, applyJTJ = 1/2 A.  Opt's gather has no exclude test, so J^T F at an unknown holds both directed residuals
#            of each edge, also towards a masked neighbour; the comparator counts the pixel's own four.  The comparator's preconditioner is 1.
#   ARAP     F = 2 cost, b = -2 jtf, applyJTJ = 2 A, preconditioner = 1 / (2 diag A).  The comparator differentiates F = sum w e^2 itself.
#   SFS      F = 2 cost, b = -jtf, applyJTJ = A, probed diagonal = diag A: the comparator's b is -1/2 dF/dx (not -dF/dx as for ARAP).
# The SFS comparator defines residuals only at x in [2, W-6], y in [2, H-6]; the fixtures clear the depth outside that window, so both sides hold
# the same residual set.  The compared set below is every unknown row of Opt whose stencil support lies inside both definitions.
# The CG iterates are scale-free: the recorder preconditions like Opt (none for poisson and SFS, 1/(1+sqrt(diag))^2 for ARAP), so x_k equals
# the step of one Gauss-Newton iteration with lIterations = k.
import pytest

import reference_cases as rc
from helpers import flat_unknowns

REL = {"poisson_image_editing": dict(F=2.0, b=-0.5, A=0.5), "arap_mesh_deformation": dict(F=2.0, b=-2.0, A=2.0), "shape_from_shading": dict(F=2.0, b=-1.0, A=1.0)}
MIN_COVER = {"poisson_rand_241x9": 0.45, "poisson_tiny_5x3": 0.13, "poisson_real_112x80": 0.15, "arap_raptor2k": 1.0, "arap_hub17_19x13": 1.0,
             "sfs_40x32": 0.6, "sfs_130x37": 0.7, "sfs_real_48x40": 0.65}


def compared_rows(P):
    """Rows of Opt's flat unknown vector where the comparator and Opt define the same operator."""
    if P.energy == "poisson_image_editing":                      # the unknowns: M == 0
        return np.repeat(np.asarray(P.params[2]).reshape(-1) == 0, 4)
    if P.energy == "shape_from_shading":                         # valid depth inside the comparator's residual window
        W, H = P.dims
        y, x = np.mgrid[0:H, 0:W]
        inside = (x >= 2) & (x <= W - 6) & (y >= 2) & (y <= H - 6)
        return (inside & (np.asarray(P.params[17]) > 0)).reshape(-1)
    return np.ones(flat_unknowns(P).size, dtype=bool)            # ARAP: every vertex (symmetric graph)


def load_case(name):
    """(problem, fixture) with the inputs checked against the recorded checksums."""
    P = rc.problem(name)
    G = np.load(rc.fixture_path(name))
    v = rc.probe_vector(P, name)
    np.testing.assert_array_equal(v, G["v"])
    assert list(rc.checksums(P, v)) == list(G["checksums"]), f"{name}: the inputs differ from the ones the comparator was recorded on"
    return P, G


def assert_elementwise(got, ref, rows, tol, what):
    """max_i |got_i - ref_i| <= tol max|ref| on the compared rows, and the norm-wise relative error below tol."""
    got, ref = np.asarray(got, dtype=np.float64)[rows], np.asarray(ref, dtype=np.float64)[rows]
    scale = np.max(np.abs(ref))
    assert scale > 0, what
    err = np.max(np.abs(got - ref)) / scale
    assert err <= tol, f"{what}: max elementwise error {err:.3e} > {tol:.1e} (at row {int(np.argmax(np.abs(got - ref)))})"
    assert rel_err(got, ref) <= tol, what


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_operators_agree_with_the_comparator(oracle_lib, name):
    P, G = load_case(name)
    s = REL[P.energy]
    Pd = rc.as_double(P)
    rows = compared_rows(Pd)
    assert rows.mean() >= MIN_COVER[name], f"compared set shrank to {rows.mean():.3f} of the unknowns"
    o = oracle_solver(oracle_lib, Pd)
    cost = o.eval_cost(Pd.params)
    jtf, diag = o.eval_jtf(Pd.params)
    Av = o.apply_jtj(Pd.params, G["v"].astype(np.float64))
    o.close()
    assert abs(s["F"] * cost - float(G["F"])) <= 1e-12 * abs(float(G["F"]))
    assert abs(s["F"] * cost - float(G["F_float"])) <= 1e-5 * abs(float(G["F_float"]))
    assert_elementwise(s["b"] * jtf, G["b"], rows, 1e-12, "J^T F")
    assert_elementwise(s["A"] * Av, G["jtj_v"], rows, 1e-12, "J^T J v")
    if P.energy == "arap_mesh_deformation":
        assert_elementwise(1.0 / (s["A"] * diag[rows]), G["pre"][rows], slice(None), 1e-12, "preconditioner")
    elif P.energy == "shape_from_shading":
        assert float(G["radius"]) == 2.0                          # what makes the period-5 probes exact
        assert_elementwise(s["A"] * diag, G["diag"], rows, 1e-12, "diag J^T J")
    else:
        assert np.all(G["pre"][rows] == 1.0)                      # poisson.t: UsePreconditioner(false)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_first_pcg_steps_agree_with_the_comparator(oracle_lib, name):
    P, G = load_case(name)
    for k in (1, 2, 3):
        Pd = rc.as_double(P)
        x0 = flat_unknowns(Pd)
        o = oracle_solver(oracle_lib, Pd, nIterations=1, lIterations=k)
        o.solve(Pd.params)
        o.close()
        rows = compared_rows(Pd)
        assert_elementwise(flat_unknowns(Pd) - x0, G[f"x{k}"], rows, 1e-12, f"x_{k}")
        assert np.all(flat_unknowns(Pd)[~rows] == x0[~rows])
