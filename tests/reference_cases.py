"""Inputs of the reference-comparator fixtures (tests/golden/reference_data/comparator_*.npz).

tests/golden/make_reference_fixtures.py runs the reference's hand-written comparator maths on these problems and records what it computes;
tests/test_reference_comparator_cpu.py and tests/test_reference_comparator_gpu.py rebuild the same problems and compare.  Every array is
float32-representable, so the float recording, the widened (double) recording, float plans and double plans all read the same numbers.
Each fixture stores a checksum of every input array and of the probe vector v: a change to a workload generator fails loudly.
"""
import hashlib
import os

import numpy as np

from opt_amd import workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "reference_data")


def _f32(P):
    """The problem with every floating-point array rounded to float32 (scalars and index arrays unchanged)."""
    P = P.clone()
    P.params = [np.ascontiguousarray(a, dtype=np.float32) if isinstance(a, np.ndarray) and a.dtype.kind == "f" and a.ndim > 0 else a for a in P.params]
    P.double = False
    return P


def as_double(P):
    """The same problem for a double plan: unknowns and arrays widened, host scalars (declared `float` in the .t) kept."""
    P = P.clone()
    P.params = [a.astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim > 0 else a for a in P.params]
    P.double = True
    return P


def _poisson_real():
    z = np.load(os.path.join(HERE, "fixtures", "poisson_real_112x80.npz"))
    H, W = z["mask"].shape
    alpha = np.full((H, W, 1), 255.0)
    X = np.concatenate([z["base"].astype(np.float64), alpha], -1)
    T = np.concatenate([z["inserted"].astype(np.float64), alpha], -1)
    M = np.where(z["mask"] == 255, 0.0, 255.0)
    return wl.Problem("poisson_image_editing", (W, H), [X, T, M], (0,), False)


def _poisson_random_mask(W, H, seed):
    P = wl.poisson_image_editing(W, H, seed=seed)
    P.params[2] = np.where(np.random.default_rng(seed + 100).random((H, W)) < 0.5, 0.0, 255.0)
    return P


def _arap_perturbed(P, seed):
    """Offsets and angles moved off the rest pose (rotations away from I, non-zero regulariser residuals)."""
    rng = np.random.default_rng(seed)
    N = P.params[2].shape[0]
    P.params[2] = P.params[2] + 0.002 * rng.standard_normal((N, 3))
    P.params[3] = P.params[3] + 0.05 * rng.standard_normal((N, 3))
    return P


def _arap_raptor():
    from opt_amd import io
    z = np.load(os.path.join(HERE, "fixtures", "raptor2k_mesh.npz"))
    return _arap_perturbed(io.arap_problem_from_mesh(z["vertices"], z["faces"].tolist(), z["marker_index"], z["marker_position"], alpha=0.3), 11)


def _arap_hub(hub=17):
    """The 19x13 grid of test_arap_high_valence_vertex_and_the_ell_width with one interior vertex joined to `hub` others (both directions):
    more than 16 neighbours sends the graph to the edge-list gather instead of the ELL planes.  Edges stay grouped by head vertex."""
    P = wl.arap_mesh_deformation(19, 13, seed=5, perturb=0.01)
    heads, tails = list(P.params[7]), list(P.params[8])
    n, h = 19 * 13, 7 * 19 + 9
    have = {t for a, t in zip(heads, tails) if a == h}
    extra = [v for v in range(0, n, 3) if v != h and v not in have][:hub - len(have)]
    nb = [[] for _ in range(n)]
    for a, t in zip(heads, tails):
        nb[a].append(t)
    for v in extra:
        nb[h].append(v); nb[v].append(h)
    P.params[7] = np.array([a for a in range(n) for _ in nb[a]], dtype=np.int32)
    P.params[8] = np.array([t for a in range(n) for t in nb[a]], dtype=np.int32)
    P.params[6] = np.array(len(P.params[7]), dtype=np.int32)
    return P


def sfs_comparator_window(P):
    """The comparator defines SFS residuals only at x in [2, W-6], y in [2, H-6] (SFSSolverEquations.h:89); Opt everywhere inside a 1-pixel
    border.  Clearing the depth (and the unknown) outside that window leaves both definitions with the same residual set."""
    P = P.clone()
    W, H = P.dims
    y, x = np.mgrid[0:H, 0:W]
    out = (x < 2) | (x > W - 6) | (y < 2) | (y > H - 6)
    for k in (16, 17):
        P.params[k] = np.where(out, -10000.0, P.params[k])
    return P


def _sfs_real_crop(x0=20, y0=16, w=48, h=40):
    z = np.load(os.path.join(HERE, "golden", "sfs_real_crop_96x80.npz"))
    params = [np.array(z[f"param_{k}"]) for k in range(21)]
    params[5] = np.array(params[5] - x0, dtype=np.float32)          # principal point in the crop's pixel frame
    params[6] = np.array(params[6] - y0, dtype=np.float32)
    for k in range(16, 21):
        params[k] = np.ascontiguousarray(params[k][y0:y0 + h, x0:x0 + w])
    return wl.Problem("shape_from_shading", (w, h), params, (16,), False)


CASES = {
    "poisson_rand_241x9": lambda: _poisson_random_mask(241, 9, 3),          # wider than one double strip of the marching kernels
    "poisson_tiny_5x3": lambda: wl.poisson_image_editing(5, 3, seed=4),
    "poisson_real_112x80": _poisson_real,
    "arap_raptor2k": _arap_raptor,
    "arap_hub17_19x13": _arap_hub,
    "sfs_40x32": lambda: sfs_comparator_window(wl.shape_from_shading(40, 32, double=False, seed=6, holes=True, noise=2e-3)),
    "sfs_130x37": lambda: sfs_comparator_window(wl.shape_from_shading(130, 37, double=False, seed=8, holes=True, noise=2e-3)),
    "sfs_real_48x40": lambda: sfs_comparator_window(_sfs_real_crop()),
}


def problem(name):
    """The float32 problem of fixture `name` (use as_double() for a double plan)."""
    return _f32(CASES[name]())


def probe_vector(P, name):
    """The seeded vector the comparator's applyJTJ was recorded on (Opt's flat unknown layout)."""
    n = sum(np.asarray(P.params[i]).size for i in P.unknown_slots)
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def checksums(P, v):
    """sha256 of every array parameter (and of v), in binding order."""
    out = [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in P.params if isinstance(a, np.ndarray) and a.ndim > 0]
    return np.array(out + [hashlib.sha256(v.tobytes()).hexdigest()])


def fixture_path(name):
    return os.path.join(DATA, f"comparator_{name}.npz")
