"""GPU parity tests (-m gpu) of the per-vertex edge lists (opt_amd/csrc/graph_lists.h VertexLists) at their smallest sizes: an empty list between two non-empty ones
and a graph of one hyperedge, for ArapOps (two one-slot lists) and for one functor energy (GraphOps, one combined list).  The larger shapes -- hubs, a vertex without
hyperedges at the end, a tail-only vertex, repeated hyperedges (equal keys, distinct ids in the insertion sort), re-bound graphs -- are tests/test_graph_shapes_gpu.py,
whose helpers and float bars these tests share."""
import numpy as np
import pytest

import graph_cases as gc
from helpers import flat_unknowns, hip_solver, oracle_solver, rel_err
from test_graph_shapes_gpu import _as_double, _base, _solve

pytestmark = pytest.mark.gpu


def _oracle_run(oracle_lib, P, **kw):
    o = oracle_solver(oracle_lib, P, "gaussNewtonGPU", **kw)
    R = P.clone()
    o.init(R.params)
    costs = [o.cost()]
    while True:
        more = o.step(R.params)
        costs.append(o.cost())
        if not more:
            break
    o.close()
    return costs, flat_unknowns(R)


@pytest.mark.parametrize("energy", ["arap", "embedded"])
@pytest.mark.parametrize("case", ["unused_vertex", "one_edge"])
def test_edge_lists_at_their_smallest(oracle_lib, case, energy):
    """unused_vertex: 5 vertices of which vertex 2 is in no hyperedge (an empty list between two non-empty ones); one_edge: the armadillo with its index arrays cut to
    nE = 1 (every list but two empty; ARAP: asymmetric, the edge-list gather).  Float, Gauss-Newton, 2 steps x 4 PCG iterations beside the float oracle.  (A hyperedge
    listed twice -- equal keys, distinct ids in the insertion sort -- is test_graph_shapes[duplicates-cotangent-gather].)
    Bars: the float bars of test_graph_shapes_gpu.py -- costs 1e-5 (relative to the initial cost where the energy has converged, as _check_trajectory), unknowns 3e-5 norm-wise -- or, where
    the float oracle's own run ends further than half of that from the double oracle on the same float inputs, twice that distance (the yardstick of
    test_energies_gpu.py::test_trajectory's envelopes: one_edge converges to a cost that is rounding noise of the unknowns)."""
    P = gc.tetrahedron_with_unused_vertex(energy, False) if case == "unused_vertex" else gc.truncated(_base(energy, "armadillo", False), 1)
    kw = dict(nIterations=2, lIterations=4)
    c_ref, x_ref = _oracle_run(oracle_lib, P, **kw)
    c_dbl, x_dbl = _oracle_run(oracle_lib, _as_double(P), **kw)
    assert len(c_ref) == len(c_dbl) and np.all(np.isfinite(c_ref)) and np.all(np.isfinite(x_ref))
    g = hip_solver(P, "gaussNewtonGPU", **kw)
    c, x, _ = _solve(g, P)
    g.close()
    assert len(c) == len(c_ref)
    scale = abs(c_ref[0])
    for i, (a, b, d) in enumerate(zip(c, c_ref, c_dbl)):
        bar = max(1e-5 * max(abs(b), 1e-7 * scale), 2 * abs(b - d))
        print(f"cost {i}: gpu {a:.9g} oracle {b:.9g} double oracle {d:.9g} |gpu - oracle| {abs(a - b):.3g} bar {bar:.3g}")
        assert abs(a - b) <= bar, (i, a, b, d, bar)
    xbar = max(3e-5, 2 * rel_err(x_ref, x_dbl))
    print(f"unknowns: |gpu - oracle| / |oracle| {rel_err(x, x_ref):.3g}, float oracle against double oracle {rel_err(x_ref, x_dbl):.3g}, bar {xbar:.3g}")
    assert rel_err(x, x_ref) <= xbar
