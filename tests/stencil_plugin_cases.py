"""The cases of the image-domain plug-in tests (examples/plugins/vector_tv_denoising.{t,hip}) and the energy restated in numpy.

The CPU oracle knows the built-in energies only, so -- as tests/test_plugin_energy_gpu.py does for the spring energy -- the sample is restated here: the residuals,
the analytic Jacobian (d sqrt(|d|^2 + eps^2) / dX = +-d / sqrt(.)) and the reference's Gauss-Newton / Jacobi-PCG loop (PCGInit1 (+ _Finish), PCGStep1-3 and
PCGLinearUpdate of solverGPUGaussNewton.t:361-560 with the CERES guarded inverse 1 / (1 + sqrt(d))^2, :323-332).  The Jacobian is held as its non-zero entries (per
residual row the partials w.r.t. the centre pixel and w.r.t. the forward neighbour), because the largest case has 9620 unknowns and 19240 rows; jacobian_dense()
expands it for the small cases, where tests/test_stencil_plugin_cases_cpu.py checks the structured products against it.

The engine's semantics of Exclude (stencil_engine.h, energy.h): an excluded pixel is not an unknown -- its rows of J^T F, diag(J^T J) and J^T J p are 0 -- the residuals
centred on it do not count in the cost, but they do count in J^T F / J^T J of their non-excluded neighbours.

`dt` is the arithmetic of the vectors: float64 for the reference, float32 to measure what single precision costs (the sums are accumulated in double and rounded to
dt, as every kernel of the library does).  Importing this module loads nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from opt_amd import workloads as wl      # noqa: E402

# the smallest shapes at which the kernels can go wrong: a few rows in one workgroup; a row longer than a wave; no neighbour in one direction (both ways); several
# workgroups with a ragged last one (4810 pixels = 18 workgroups of 256 + 202)
SHAPES = [(13, 9), (70, 5), (1, 7), (7, 1), (130, 37)]
MASKS = ["block", "border", None]
CASES = [dict(name="%dx%d-%s" % (W, H, m or "nomask"), W=W, H=H, mask=m, seed=3 + i) for i, (W, H) in enumerate(SHAPES) for m in MASKS]
GN_STEPS, GN_LITERS = 3, 10          # the trajectory the GPU tests take
BARS = {"probe": {True: 1e-12, False: 1e-5}, "trajectory": {True: 1e-10, False: 1e-5}}      # [double]: the README's parity contracts


def case(name):
    return next(c for c in CASES if c["name"] == name)


def problem(c, double):
    return wl.vector_tv_denoising(c["W"], c["H"], double=double, seed=c["seed"], mask=c["mask"])


class Model:
    """The energy at X (H, W, 2) on the problem's own (possibly float32-rounded) inputs, in arithmetic dt."""

    def __init__(self, P, X=None, dt=np.float64):
        self.dt = dt
        self.X = np.asarray(P.params[0] if X is None else X, dt).reshape(P.params[0].shape)
        self.A, self.M = np.asarray(P.params[1], dt), np.asarray(P.params[2], dt)
        self.wf, self.wr, self.eps = dt(P.params[3]), dt(P.params[4]), dt(P.params[5])
        self.H, self.W = self.M.shape
        self.ex = self.M > 0
        X = self.X
        self.F0 = self.wf * (X - self.A)                                   # fit rows (H, W, 2)
        self.dx = X[:, :-1] - X[:, 1:]                                     # centre (x, y), neighbour (x + 1, y): centres x < W - 1
        self.dy = X[:-1, :] - X[1:, :]
        self.lx = np.sqrt(self.dx[..., 0] * self.dx[..., 0] + self.dx[..., 1] * self.dx[..., 1] + self.eps * self.eps)
        self.ly = np.sqrt(self.dy[..., 0] * self.dy[..., 0] + self.dy[..., 1] * self.dy[..., 1] + self.eps * self.eps)
        self.Fx, self.Fy = self.wr * (self.lx - self.eps), self.wr * (self.ly - self.eps)
        self.gx = self.wr * (self.dx / self.lx[..., None])                # d Fx / d X(centre); d Fx / d X(neighbour) = -gx
        self.gy = self.wr * (self.dy / self.ly[..., None])

    def _sum(self, a):
        return self.dt(np.sum(np.asarray(a, np.float64)))

    def cost(self):
        inc = ~self.ex
        s = (self.F0 * self.F0).sum(-1).astype(np.float64) * inc
        s[:, :-1] += (self.Fx * self.Fx).astype(np.float64) * inc[:, :-1]
        s[:-1, :] += (self.Fy * self.Fy).astype(np.float64) * inc[:-1, :]
        return 0.5 * float(s.sum())

    def _rows(self, a):      # rows of excluded unknowns are 0
        a = a.copy(); a[self.ex] = 0
        return a.reshape(-1)

    def jtf(self):
        G = self.wf * self.F0
        G[:, :-1] += self.gx * self.Fx[..., None]; G[:, 1:] -= self.gx * self.Fx[..., None]
        G[:-1, :] += self.gy * self.Fy[..., None]; G[1:, :] -= self.gy * self.Fy[..., None]
        return self._rows(G)

    def diag(self):
        D = np.full(self.X.shape, self.wf * self.wf, self.dt)
        D[:, :-1] += self.gx * self.gx; D[:, 1:] += self.gx * self.gx
        D[:-1, :] += self.gy * self.gy; D[1:, :] += self.gy * self.gy
        return self._rows(D)

    def jtj(self, v):
        v = np.asarray(v, self.dt).reshape(self.X.shape)
        jx = (self.gx * (v[:, :-1] - v[:, 1:])).sum(-1)                   # (J v) of the rows Fx
        jy = (self.gy * (v[:-1, :] - v[1:, :])).sum(-1)
        O = self.wf * (self.wf * v)
        O[:, :-1] += self.gx * jx[..., None]; O[:, 1:] -= self.gx * jx[..., None]
        O[:-1, :] += self.gy * jy[..., None]; O[1:, :] -= self.gy * jy[..., None]
        return self._rows(O)

    def jacobian_dense(self):
        """(F, J): all 4 W H residual rows (pixel-major: fit 0, fit 1, x difference, y difference; 0 where the stencil leaves the image), columns 2 (y W + x) + c."""
        H, W = self.H, self.W
        F = np.zeros(4 * H * W); J = np.zeros((4 * H * W, 2 * H * W))
        for y in range(H):
            for x in range(W):
                i = y * W + x
                for c in range(2):
                    F[4 * i + c] = self.F0[y, x, c]; J[4 * i + c, 2 * i + c] = self.wf
                if x + 1 < W:
                    F[4 * i + 2] = self.Fx[y, x]
                    J[4 * i + 2, 2 * i:2 * i + 2] = self.gx[y, x]; J[4 * i + 2, 2 * (i + 1):2 * (i + 1) + 2] = -self.gx[y, x]
                if y + 1 < H:
                    F[4 * i + 3] = self.Fy[y, x]
                    J[4 * i + 3, 2 * i:2 * i + 2] = self.gy[y, x]; J[4 * i + 3, 2 * (i + W):2 * (i + W) + 2] = -self.gy[y, x]
        return F, J


def gauss_newton(P, nsteps=GN_STEPS, liters=GN_LITERS, dt=np.float64):
    """(costs after init and every step, final X flattened): the reference's loop in arithmetic dt."""
    X = np.asarray(P.params[0], dt).copy()
    m = Model(P, X, dt)
    costs = [m.cost()]
    one = dt(1)
    for _ in range(nsteps):
        r = -m.jtf()                                               # PCGInit1
        s = one + np.sqrt(m.diag())
        M = one / (s * s)                                          # guardedInvert (CERES), PCGInit1_Finish
        p = M * r
        delta = np.zeros_like(r)
        a_num = m._sum(r * p)
        for _ in range(liters):
            Ap = m.jtj(p); a_den = m._sum(p * Ap)                  # PCGStep1
            alpha = a_num / a_den if a_den > 0 else dt(0)          # PCGStep2
            delta = delta + alpha * p; r = r - alpha * Ap
            z = M * r; b_num = m._sum(z * r)
            beta = b_num / a_num if a_num > 0 else dt(0)           # PCGStep3
            p = z + beta * p
            a_num = b_num
        X = X + delta.reshape(X.shape)                             # PCGLinearUpdate
        m = Model(P, X, dt)
        costs.append(m.cost())
    return costs, np.asarray(X, np.float64).reshape(-1)


def probe_direction(n):
    return np.random.default_rng(11).standard_normal(n)


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))
