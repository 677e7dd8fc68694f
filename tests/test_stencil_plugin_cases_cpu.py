"""CPU test (no GPU): the cases of the image-domain plug-in tests (tests/stencil_plugin_cases.py) are fit for the bars the GPU tests hold them to.

For every case used with a float bar, the numpy restatement of the energy is run in float32 arithmetic and must stay within a TENTH of that bar of its float64 run --
the probes (cost, J^T F, diag J^T J, J^T J v) and the Gauss-Newton trajectory over the steps the GPU test takes.  A case that cannot hold this would be replaced, not
its bar widened.  The structured Jacobian of the restatement is checked against its dense expansion on the small shapes, and by finite differences."""
import numpy as np
import pytest

import stencil_plugin_cases as sc
from helpers import rel_err

NAMES = [c["name"] for c in sc.CASES]


def test_the_case_list_is_the_issue_s():
    assert [(c["W"], c["H"]) for c in sc.CASES[::3]] == [(13, 9), (70, 5), (1, 7), (7, 1), (130, 37)]
    assert len(sc.CASES) == 15 and len(set(NAMES)) == 15
    for c in sc.CASES:
        P = sc.problem(c, True)
        ex = np.asarray(P.params[2]) > 0
        assert P.dims == (c["W"], c["H"]) and P.params[0].shape == (c["H"], c["W"], 2) and P.unknown_slots == (0,)
        if c["mask"] is None:
            assert not ex.any()
        else:
            assert ex.any() and not ex.all(), c      # something is excluded, something is left
        if c["mask"] == "border" and min(c["W"], c["H"]) >= 3:
            assert ex[0].all() and ex[-1].all() and ex[:, 0].all() and ex[:, -1].all() and not ex[1:-1, 1:-1].any()
        if c["mask"] == "block":
            ys, xs = np.nonzero(ex)
            assert ex[ys.min():ys.max() + 1, xs.min():xs.max() + 1].all()      # one full block
        # eps at the scale of the neighbour differences: the square root is neither linear (|d| >> eps) nor singular (|d| << eps)
        m = sc.Model(P)
        d = np.concatenate([np.linalg.norm(m.dx, axis=-1).reshape(-1), np.linalg.norm(m.dy, axis=-1).reshape(-1)])
        eps = float(P.params[5])
        assert 0.3 * eps < np.median(d) < 3.0 * eps, (c["name"], np.median(d), eps)
    # 130 x 37: several workgroups of 256 pixels with a ragged last one; 70 x 5: a row longer than a wave
    assert 130 * 37 > 4 * 256 and (130 * 37) % 256 != 0 and 70 > 64


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("130x37")])
def test_structured_products_match_the_dense_jacobian(name):
    P = sc.problem(sc.case(name), True)
    m = sc.Model(P)
    F, J = m.jacobian_dense()
    keep = np.repeat(~m.ex.reshape(-1), 2).astype(np.float64)
    v = sc.probe_direction(J.shape[1])
    assert rel_err(m.jtf(), keep * (J.T @ F)) < 1e-13
    assert rel_err(m.diag(), keep * (J * J).sum(0)) < 1e-13
    assert rel_err(m.jtj(v), keep * (J.T @ (J @ v))) < 1e-13
    rows = np.repeat(~m.ex.reshape(-1), 4)
    assert abs(m.cost() - 0.5 * float(F[rows] @ F[rows])) <= 1e-13 * m.cost()
    # the Jacobian itself, by central differences on the residual vector
    X = np.asarray(P.params[0], np.float64)
    h = 1e-6
    for j in np.random.default_rng(1).choice(J.shape[1], size=min(8, J.shape[1]), replace=False):
        e = np.zeros(J.shape[1]); e[j] = h
        Fp, _ = sc.Model(P, X + e.reshape(X.shape)).jacobian_dense()
        Fm, _ = sc.Model(P, X - e.reshape(X.shape)).jacobian_dense()
        assert np.max(np.abs((Fp - Fm) / (2 * h) - J[:, j])) < 1e-7


@pytest.mark.parametrize("name", NAMES)
def test_float32_arithmetic_stays_within_a_tenth_of_the_float_bars(name):
    P = sc.problem(sc.case(name), False)
    m64, m32 = sc.Model(P), sc.Model(P, dt=np.float32)
    v = sc.probe_direction(m64.X.size).astype(np.float32)
    bar = 0.1 * sc.BARS["probe"][False]
    errs = {"cost": abs(m32.cost() - m64.cost()) / m64.cost(), "r": rel_err(m32.jtf(), m64.jtf()), "diag": rel_err(m32.diag(), m64.diag()), "out": rel_err(m32.jtj(v), m64.jtj(v))}
    print(name, errs)
    assert max(errs.values()) <= bar, (errs, bar)
    c64, x64 = sc.gauss_newton(P, dt=np.float64)
    c32, x32 = sc.gauss_newton(P, dt=np.float32)
    bar = 0.1 * sc.BARS["trajectory"][False]
    drift = [abs(a - b) / abs(b) for a, b in zip(c32, c64)]
    print(name, "cost drift", drift, "x", rel_err(x32, x64))
    assert len(c64) == sc.GN_STEPS + 1 and max(drift) <= bar and rel_err(x32, x64) <= bar, (drift, bar)
    assert c64[1] < c64[0] and np.isfinite(x64).all()
