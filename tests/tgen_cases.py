"""What the tests of generated energies share (test_tgen_cpu.py, test_tgen_gpu.py, tgen_driver.py): the six energies that are generated and run on the GPU, their
.t files, their libraries and their inputs.  Importing this module loads nothing.

The six: the two samples under examples/plugins/ (a hand-written plug-in source exists for each: the comparator) and gen_ copies of four built-in energies (the
project's own .t bodies copied to gen_<energy>.t, so that the stem differs from the built-in name: the registry resolves a .t by its stem first, and the generated
plug-in and the built-in kernel set coexist in one process).  The libraries of the two samples are built beside, not onto, the hand-written plug-ins' libraries
(opt_amd/lib/plugins/gen/): other tests load those by their default path."""
import os
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from opt_amd import workloads as wl      # noqa: E402

SAMPLES = {"vector_tv_denoising": wl.VECTOR_TV_T, "spring_mesh_deformation": wl.SPRING_T}
COPIES = ("image_warping", "arap_mesh_deformation", "embedded_mesh_deformation", "cotangent_mesh_smoothing")
SIX = list(SAMPLES) + ["gen_" + e for e in COPIES]
IMAGE_ENERGIES = ("vector_tv_denoising", "gen_image_warping")
KEY = {"gen_arap_mesh_deformation": "arap", "gen_embedded_mesh_deformation": "embedded", "gen_cotangent_mesh_smoothing": "cotangent"}
# images: a few rows in one workgroup; the smallest with an interior; wider than a wave, thin, with a ragged last block (335 pixels = 256 + 79)
IMAGE_SHAPES = [(5, 3), (13, 9), (67, 5)]
MASKS = [None, "block", "border"]
MESHES = ("grid", "grid_shapes", "armadillo")
BARS = {"probe": {True: 1e-12, False: 1e-5}, "trajectory": {True: 1e-10, False: 1e-5}}      # [double]: the README's parity contracts


def builtin_of(name):
    return name[4:] if name.startswith("gen_") else None


def t_file(name, tmp):
    """The .t of one of the six: the sample's own file, or the built-in energy's body copied to <tmp>/gen_<energy>.t."""
    from opt_amd import api
    if name in SAMPLES:
        return SAMPLES[name]
    dst = os.path.join(str(tmp), name + ".t")
    if not os.path.exists(dst):
        os.makedirs(str(tmp), exist_ok=True)
        shutil.copy(api.energy_file(builtin_of(name)), dst)
    return dst


def library_path(name):
    from opt_amd import build
    return os.path.join(build.PLUGIN_LIBDIR, "gen", "lib%s.so" % name) if name in SAMPLES else build.plugin_path(name)


def remarks_stem(name):
    """What build.plugin_kernel_resources takes for the library of library_path(name)."""
    return "lib" + name if name in SAMPLES else name


def library(name, tmp, force=False):
    from opt_amd import tgen
    return tgen.compile_energy(t_file(name, tmp), force=force, out=library_path(name) if name in SAMPLES else None)


def build_all(tmp, names=SIX, jobs=4, force=False):
    """{name: library path}, at most `jobs` compilers at once."""
    with ThreadPoolExecutor(jobs) as ex:
        return dict(zip(names, ex.map(lambda n: library(n, tmp, force), names)))


def image_name(W, H, mask):
    return "%dx%d-%s" % (W, H, mask or "nomask")


IMAGE_INPUTS = [image_name(W, H, m) for W, H in IMAGE_SHAPES for m in MASKS]


def _mask(W, H, mask, value):
    M = np.zeros((H, W))
    if mask == "block":
        x0, y0 = W // 3, H // 3
        M[y0:y0 + max(1, H // 4), x0:x0 + max(1, W // 4)] = value
    elif mask == "border":
        M[0, :] = value; M[-1, :] = value; M[:, 0] = value; M[:, -1] = value
    else:
        assert mask is None, mask
    return M


def image_problem(name, inp, double):
    """vector_tv_denoising / image_warping on the input `WxH-mask`.  image_warping: perturbed offsets and angles, rest positions off the lattice (the general
    UrShape), a tenth of the pixels constrained; masked pixels carry 255 like the example's."""
    shape, mask = inp.split("-")
    W, H = (int(v) for v in shape.split("x"))
    mask = None if mask == "nomask" else mask
    if name == "vector_tv_denoising":
        return wl.vector_tv_denoising(W, H, double=double, seed=3 + W, mask=mask)
    assert name in ("gen_image_warping", "image_warping"), name
    P = wl.image_warping(W, H, double=double, random_state=5 + W, perturb=0.3, jitter_urshape=0.2, fit_fraction=0.1)
    P.params[4] = _mask(W, H, mask, 255.0).astype(P.params[4].dtype)
    return P


def mesh_problem(name, mesh, double):
    """spring: the inputs of tests/plugin_energy_driver.py.  The gen_ energies: the built-in energy's problem on the 7 x 5 open patch (grid), on that patch with a
    degree-16 hub and one isolated vertex (grid_shapes) and on the armadillo (130 vertices), as tests/graph_cases.py builds them."""
    if name == "spring_mesh_deformation":
        import plugin_energy_driver as drv
        return drv.problem(mesh, double)
    import graph_cases as gc
    key = KEY[name] if name in KEY else name
    if mesh == "armadillo":
        return gc.base_problem(key, "armadillo", double)
    P = gc.base_problem(key, "open_patch", double)
    if mesh == "grid_shapes":
        P = gc.with_hub(P, 16)
        R = gc._rest_positions(P)
        P = gc._append_vertex(P, R.mean(0) + 0.5 * R.std(0))      # (with_isolated_vertex without its odd-count assertion: the vertex count becomes 36)
    else:
        assert mesh == "grid", mesh
    return P


def inputs_of(name):
    return IMAGE_INPUTS if name in IMAGE_ENERGIES else list(MESHES)


def problem(name, inp, double):
    return image_problem(name, inp, double) if name in IMAGE_ENERGIES else mesh_problem(name, inp, double)


def probe_direction(n):
    return np.random.default_rng(11).standard_normal(n)


# ---- the round trip: an energy nobody wrote a functor for ------------------------------------------------------------------------------------------------------
ROUND_TRIP_STEM = "smooth_spring_deformation"
ROUND_TRIP_T = """-- spring_mesh_deformation plus a smoothness term: neighbouring vertices should be displaced alike.  Written for tests/test_tgen_gpu.py.
local N = Dim("N", 0)
local X = Unknown("X", opt_float3, {N}, 0)
local UrShape = Image("UrShape", opt_float3, {N}, 1)
local Constraints = Image("Constraints", opt_float3, {N}, 2)
local w_fitSqrt = Param("w_fitSqrt", float, 3)
local w_regSqrt = Param("w_regSqrt", float, 4)
local G = Graph("G", 5, "v0", {N}, 6, "v1", {N}, 7)
local w_smoothSqrt = Param("w_smoothSqrt", float, 8)

UsePreconditioner(true)

local pinned = greatereq(Constraints(0)(0), -999999.9)
Energy(Select(pinned, w_fitSqrt * (X(0) - Constraints(0)), 0))

local function length(d) return Sqrt(Dot3(d, d)) end
Energy(w_regSqrt * (length(X(G.v1) - X(G.v0)) - length(UrShape(G.v1) - UrShape(G.v0))))

-- the displacement field X - UrShape is smooth along every half-edge (a vector term: one residual per channel)
local function displacement(v) return X(v) - UrShape(v) end
Energy(w_smoothSqrt * (displacement(G.v1) - displacement(G.v0)))
"""
ROUND_TRIP_W_SMOOTH = 0.7


def round_trip_problem(double):
    import plugin_energy_driver as drv
    P = drv.problem("grid", double)
    P.params.append(np.array(ROUND_TRIP_W_SMOOTH, dtype=np.float32))
    P.energy = ROUND_TRIP_STEM
    return P


def round_trip_residuals_and_jacobian(P, X):
    """F (3 N vertex residuals, then per half-edge the spring residual and the three smoothness residuals) and the dense J at X [N, 3], in float64."""
    f = np.float64
    U, C, wf, wr, v0, v1, ws = np.asarray(P.params[1], f), np.asarray(P.params[2], f), float(P.params[3]), float(P.params[4]), np.asarray(P.params[6]), np.asarray(P.params[7]), float(P.params[8])
    N, E = len(X), len(v0)
    valid = C[:, 0] >= -999999.9
    F = np.zeros(3 * N + 4 * E); J = np.zeros((3 * N + 4 * E, 3 * N))
    F[:3 * N] = np.where(valid[:, None], wf * (X - np.where(valid[:, None], C, 0.0)), 0.0).reshape(-1)
    for v in np.flatnonzero(valid):
        for c in range(3):
            J[3 * v + c, 3 * v + c] = wf
    d = X[v1] - X[v0]
    ln = np.linalg.norm(d, axis=1)
    u = U[v1] - U[v0]
    for e in range(E):
        row = 3 * N + 4 * e
        F[row] = wr * (ln[e] - np.linalg.norm(u[e]))
        g = wr * d[e] / ln[e]
        J[row, 3 * v1[e]:3 * v1[e] + 3] += g
        J[row, 3 * v0[e]:3 * v0[e] + 3] -= g
        for c in range(3):
            F[row + 1 + c] = ws * ((X[v1[e], c] - U[v1[e], c]) - (X[v0[e], c] - U[v0[e], c]))
            J[row + 1 + c, 3 * v1[e] + c] += ws
            J[row + 1 + c, 3 * v0[e] + c] -= ws
    return F, J
