"""CPU test (no GPU): why tests/test_onchip_graph_grid_gpu.py::test_trajectory_on_the_armadillo holds float cotangent Gauss-Newton to 1 x 12 where every other case runs
3 x 12.  On that input the CPU oracle's own legal summation orders (set_reduction(1, seed), seeds 1-3, against its exact-order run) agree to 1e-7 after the first step and
are as far apart as the float bar of 1e-5 itself after the second (the cost rises in that step), so no implementation can be held to the bar there; under
Levenberg-Marquardt they stay below 1e-6 over all three steps, and that case keeps 3 x 12."""
import numpy as np
import pytest

import graph_cases as gc
from helpers import oracle_solver

BAR = 1e-5      # the project's float bar on costs


def _costs(oracle_lib, P, kind, seed):
    Q = P.clone()
    o = oracle_solver(oracle_lib, Q, kind, nIterations=3, lIterations=12)
    if seed:
        o.set_reduction(1, seed)
    o.init(Q.params)
    c = [o.cost()]
    while True:
        more = o.step(Q.params)
        c.append(o.cost())
        if not more:
            break
    o.close()
    return np.array(c[:4])


@pytest.fixture(scope="module")
def spread(oracle_lib):
    P = gc.base_problem("cotangent", "armadillo", False)
    out = {}
    for kind in ("gaussNewtonGPU", "LMGPU"):
        ref = _costs(oracle_lib, P, kind, 0)
        out[kind] = np.max([np.abs(_costs(oracle_lib, P, kind, s) - ref) / np.abs(ref) for s in (1, 2, 3)], axis=0)
        print(kind, out[kind])
    return out


def test_the_first_gauss_newton_step_is_far_below_the_bar(spread):
    assert spread["gaussNewtonGPU"][1] <= 0.1 * BAR, spread


def test_the_second_gauss_newton_step_spreads_as_far_as_the_bar(spread):
    assert spread["gaussNewtonGPU"][2] >= BAR, spread


def test_levenberg_marquardt_stays_far_below_the_bar(spread):
    assert spread["LMGPU"].max() <= 0.1 * BAR, spread
