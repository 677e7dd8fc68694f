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
