"""The problems and solver settings behind every parity bar above the contract (tests/golden/parity_bars.json), in one importable place.

A parity test steps a problem side by side through the CPU oracle and the HIP library.  Where the bar of such a test sits above the contract (1e-12 double, 1e-5 float)
it comes from the frozen ensemble of legal oracle runs of the SAME case (tests/golden/parity_envelopes.json, written by tests/golden/make_parity_envelopes.py), so the
test and the generator must build the same thing: both call the functions below.  A Case is what the oracle sees -- the problem, the solver kind, the iteration counts,
the controls and the oracle's thread count -- and its `key` names the envelope; kernel variants the oracle never sees (OPT_AMD_ONCHIP_ROWS / WAVES) share one envelope.

ENTRY_CASES maps the pytest node ids whose bars sit above the contract to their Case (tests/test_parity_envelopes_cpu.py checks the table against it).
"""
import hashlib
import os

import numpy as np

from opt_amd import workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))


class Case:
    def __init__(self, tag, make, kind, nsteps, liters, controls=None, threads=1):
        self.make, self.kind, self.nsteps, self.liters, self.threads = make, kind, int(nsteps), int(liters), int(threads)
        self.controls = dict(controls or {})
        ctl = ",".join(f"{k}={self.controls[k]:g}" for k in sorted(self.controls))
        self.key = f"{tag}|{kind}|n{self.nsteps}|l{self.liters}|{ctl}|t{self.threads}"

    def problem(self):
        return self.make()

    def settings(self):
        """keyword arguments of helpers.oracle_solver / helpers.hip_solver"""
        return dict(nIterations=self.nsteps, lIterations=self.liters, **self.controls)

    def checksum(self, P=None):
        """sha256 over everything the oracle is given: settings and every bound array (dtype, shape, values).  Floating-point arrays are hashed on a grid of 2^-20 of their
        largest magnitude: another seed, size, mask or constant changes the sum, a last-bit difference between two hosts' sin / exp in the workload generators does not."""
        P = P if P is not None else self.problem()
        h = hashlib.sha256()
        h.update(repr((P.energy, tuple(int(d) for d in P.dims), bool(P.double), tuple(P.unknown_slots), self.kind, self.nsteps, self.liters,
                       sorted((k, float(v)) for k, v in self.controls.items()), self.threads)).encode())
        for p in P.params:
            a = np.ascontiguousarray(p)
            h.update(repr((a.dtype.str, a.shape)).encode())
            if a.dtype.kind == "f" and a.size:
                top = float(np.max(np.abs(a)))
                a = np.round(a.astype(np.float64) * (2.0 ** 20 / top)).astype(np.int64) if top > 0 and np.isfinite(top) else a
            h.update(a.tobytes())
        return h.hexdigest()[:16]


def _prec(double):
    return "f64" if double else "f32"


def masked_poisson(W, H, double, seed, mask):
    """poisson_image_editing with a random mask that reaches the border ("random"), none ("none") or the workload's own box"""
    P = wl.poisson_image_editing(W, H, double=double, seed=seed)
    rng = np.random.default_rng(seed + 100)
    M = P.params[2]
    if mask == "random":
        M[...] = np.where(rng.random(M.shape) < 0.3, 255.0, 0.0)
    elif mask == "none":
        M[...] = 0.0
    return P


# ---- tests/test_energies_gpu.py ------------------------------------------------------------------------------------------------------------------------------------
def _energy_case(name, double):
    import test_energies_gpu      # (its CASES table, as tests/golden/make_float_envelopes.py takes it)
    return test_energies_gpu.CASES[name](double)


def energies_trajectory(name, double, kind):
    return Case(f"energies.{name}({_prec(double)})", lambda: _energy_case(name, double), kind, 4, 12)


# ---- tests/test_onchip_sfs_gpu.py ----------------------------------------------------------------------------------------------------------------------------------
def sfs_variants_double(W, H, rows, kind):
    seed = W + 3 * H + rows
    return Case(f"sfs({W}x{H},f64,seed={seed},holes,noise=2e-3)", lambda: wl.shape_from_shading(W, H, double=True, seed=seed, holes=True, noise=2e-3), kind, 3, 10, threads=4)


def sfs_variants_float(W, H, rows, kind):
    seed = W + H + rows
    return Case(f"sfs({W}x{H},f32,seed={seed},holes,noise=2e-3)", lambda: wl.shape_from_shading(W, H, double=False, seed=seed, holes=True, noise=2e-3), kind, 2, 10,
                {"q_tolerance": -1e9} if kind == "LMGPU" else {}, threads=4)


def sfs_lm_rejected_steps():
    return Case("sfs(96x64,f64,seed=5,noise=5e-3)", lambda: wl.shape_from_shading(96, 64, double=True, seed=5, noise=5e-3), "LMGPU", 6, 10, {"trust_region_radius": 1e12}, threads=4)


# ---- tests/test_onchip_lm_gpu.py / tests/test_onchip_gpu.py --------------------------------------------------------------------------------------------------------
def onchip_lm_double(W, H, liters, period):
    rs = W * 13 + H + liters + period
    return Case(f"image_warping({W}x{H},f64,rs={rs},mask=0.1,perturb=0.4)", lambda: wl.image_warping(W, H, double=True, random_state=rs, mask_fraction=0.1, perturb=0.4),
                "LMGPU", 3, liters, {"residual_reset_period": period})


def onchip_lm_variants_float(W, H, rows, liters, period):
    rs = W * 7 + H + rows + liters
    return Case(f"image_warping({W}x{H},f32,rs={rs},mask=0.1,perturb=0.4)", lambda: wl.image_warping(W, H, random_state=rs, mask_fraction=0.1, perturb=0.4),
                "LMGPU", 3, liters, {"residual_reset_period": period, "q_tolerance": -1e9})


def onchip_many_steps():
    return Case("image_warping(260x131,f64,rs=21,mask=0.05,perturb=0.3)", lambda: wl.image_warping(260, 131, double=True, random_state=21, mask_fraction=0.05, perturb=0.3),
                "gaussNewtonGPU", 9, 5)


def onchip_deferred_time_out(nsteps):
    return Case("image_warping(300x120,f64,rs=4,mask=0.05,perturb=0.3)", lambda: wl.image_warping(300, 120, double=True, random_state=4, mask_fraction=0.05, perturb=0.3),
                "gaussNewtonGPU", nsteps, 8)


# ---- tests/test_onchip_stencil_gpu.py / tests/test_stencil_march_gpu.py --------------------------------------------------------------------------------------------
def stencil_intrinsic_double(W, H, liters):
    seed = W + H + liters
    return Case(f"intrinsic({W}x{H},f64,seed={seed})", lambda: wl.intrinsic_image_decomposition(W, H, double=True, seed=seed), "gaussNewtonGPU", 2, liters)


def stencil_lm_poisson_double(W, H, mask):
    seed = W * 3 + H
    return Case(f"poisson({W}x{H},f64,seed={seed},mask={mask})", lambda: masked_poisson(W, H, True, seed, mask), "LMGPU", 3, 10, threads=4)


# ---- tests/test_image_warping_gpu.py -------------------------------------------------------------------------------------------------------------------------------
def _cat_mask(double):
    from opt_amd import io
    m = np.load(os.path.join(HERE, "fixtures", "cat_mask_128.npz"))["mask_red"]
    P = io.image_warping_problem_from_mask(m, downsample=1, double=double)
    for sx, sy, tx, ty in wl.CAT512_MARKERS:
        P.params[3][sy // 4, sx // 4] = (tx / 4.0, ty / 4.0)
    return P


def real_cat_mask(double):
    return Case(f"image_warping(cat_mask_128,{_prec(double)})", lambda: _cat_mask(double), "gaussNewtonGPU", 1, 5)


# ---- tests/test_lm_controls_gpu.py ---------------------------------------------------------------------------------------------------------------------------------
def _lm_controls(period, qtol):
    kw = dict(residual_reset_period=period)
    if qtol is not None:
        kw["q_tolerance"] = qtol
    return kw


def lm_controls_image_warping_float(period, qtol):
    return Case("image_warping(64x48,f32,rs=9,mask=0.05,perturb=0.4)", lambda: wl.image_warping(64, 48, double=False, random_state=9, mask_fraction=0.05, perturb=0.4),
                "LMGPU", 3, 10, _lm_controls(period, qtol))


def lm_controls_image_warping_launch_loop(period, qtol, liters, double):
    return Case(f"image_warping(61x47,{_prec(double)},rs=5,mask=0.05,perturb=0.4)", lambda: wl.image_warping(61, 47, double=double, random_state=5, mask_fraction=0.05, perturb=0.4),
                "LMGPU", 4 if double else 3, liters, _lm_controls(period, qtol))


LAUNCH_LOOP_CONTROLS = [(1, None, 6), (2, None, 10), (3, None, 12), (3, 0.5, 10), (10, None, 25), (10, 0.05, 12), (4, 0.0, 9), (7, None, 23), (5, 5.0, 10),
                        (10, 0.01, 40), (6, 0.002, 60), (10, None, 1), (10, None, 2), (10, None, 3), (2, None, 3), (1, None, 1), (1, None, 2), (3, 5.0, 4)]


def lm_controls_arap(period, qtol, liters, double):
    return Case(f"arap(36x29,{_prec(double)},perturb=0.01)", lambda: wl.arap_mesh_deformation(36, 29, double=double, perturb=0.01), "LMGPU", 4 if double else 3, liters,
                _lm_controls(period, qtol))


# ---- tests/test_reference_order_mode_gpu.py ------------------------------------------------------------------------------------------------------------------------
def reference_order(name):
    import test_reference_order_mode_gpu      # (its CASES table)
    _, make, kind, nsteps, liters = next(c for c in test_reference_order_mode_gpu.CASES if c[0] == name)
    return Case(f"reference_order.{name.replace(' ', '_')}", make, kind, nsteps, liters)


# ---- pytest node id -> Case, for every check whose bar sits above the contract ---------------------------------------------------------------------------------------
def _entry_cases():
    out = {}
    f = "tests/test_energies_gpu.py::test_trajectory"
    for kind in ("gaussNewtonGPU", "LMGPU"):
        out[f"{f}[intrinsic-f64-{kind}]"] = energies_trajectory("intrinsic", True, kind)
    out["tests/test_image_warping_gpu.py::test_real_cat_mask[True]"] = real_cat_mask(True)
    f = "tests/test_lm_controls_gpu.py::test_arap_two_kernel_lm_iteration_controls"
    out[f"{f}[7-None-23-True]"] = lm_controls_arap(7, None, 23, True)
    for period, qtol, liters in [(1, None, 6), (2, None, 10), (3, 0.5, 10), (10, None, 10), (10, 0.05, 12), (4, 0.0, 9), (7, None, 23), (5, 5.0, 10)]:
        out[f"{f}[{period}-{qtol}-{liters}-False]"] = lm_controls_arap(period, qtol, liters, False)
    for period, qtol in [(2, None), (3, 0.5), (10, 0.05), (5, 0.0)]:
        out[f"tests/test_lm_controls_gpu.py::test_image_warping_float_controls[{period}-{qtol}]"] = lm_controls_image_warping_float(period, qtol)
    for period, qtol, liters in LAUNCH_LOOP_CONTROLS:
        out[f"tests/test_lm_controls_gpu.py::test_image_warping_launch_per_iteration_loop_controls[{period}-{qtol}-{liters}-False]"] = lm_controls_image_warping_launch_loop(period, qtol, liters, False)
    out["tests/test_onchip_gpu.py::test_many_steps_tag_counter_runs_on"] = onchip_many_steps()
    for fail_launch in (3, 7, 9):      # (the launch that times out is the library's business: one envelope)
        out[f"tests/test_onchip_gpu.py::test_a_time_out_among_deferred_steps_sends_the_solve_back_to_that_step[{fail_launch}-12]"] = onchip_deferred_time_out(12)
    out["tests/test_onchip_lm_gpu.py::test_double[700-3-12-5]"] = onchip_lm_double(700, 3, 12, 5)
    for W, H in [(96, 64), (300, 40), (517, 33), (64, 300), (260, 131), (1, 70), (257, 9)]:
        for rows in (2, 4, 8):
            for liters, period in [(10, 10), (12, 5), (25, 10), (9, 2)]:
                out[f"tests/test_onchip_lm_gpu.py::test_variants_float[{W}-{H}-{rows}-{liters}-{period}]"] = onchip_lm_variants_float(W, H, rows, liters, period)
    out["tests/test_onchip_sfs_gpu.py::test_lm_rejected_steps"] = sfs_lm_rejected_steps()
    for W, H, rows_list in [(123, 4, (4, 8, 10)), (5, 70, (4, 6, 10))]:
        for rows in rows_list:
            for waves in (4, 8):
                out[f"tests/test_onchip_sfs_gpu.py::test_variants_double[{W}-{H}-{rows}-{waves}-gaussNewtonGPU]"] = sfs_variants_double(W, H, rows, "gaussNewtonGPU")
    for W, H in [(40, 32), (130, 37), (200, 150)]:
        for rows in (4, 6, 8, 10):
            for waves in (4, 8):
                for kind in ("gaussNewtonGPU", "LMGPU"):
                    out[f"tests/test_onchip_sfs_gpu.py::test_variants_float[{W}-{H}-{rows}-{waves}-{kind}]"] = sfs_variants_float(W, H, rows, kind)
    for W, H in [(61, 5), (62, 3), (63, 9), (300, 40)]:
        for rows, waves in [(2, 4), (4, 4), (2, 8)]:
            out[f"tests/test_onchip_stencil_gpu.py::test_intrinsic_double[{W}-{H}-{rows}-{waves}-12]"] = stencil_intrinsic_double(W, H, 12)
    out["tests/test_onchip_stencil_gpu.py::test_lm_poisson_double[7-9-none-4-4]"] = stencil_lm_poisson_double(7, 9, "none")
    out["tests/test_reference_order_mode_gpu.py::test_reference_order_against_the_oracle[image_warping_LM_float]"] = reference_order("image_warping LM float")
    for W, H in [(240, 3), (241, 9), (300, 40), (517, 33)]:
        out[f"tests/test_stencil_march_gpu.py::test_intrinsic_double[{W}-{H}-12]"] = stencil_intrinsic_double(W, H, 12)
    return out


ENTRY_CASES = _entry_cases()


def envelope_cases():
    """{envelope key: Case}: the distinct cases behind ENTRY_CASES"""
    out = {}
    for c in ENTRY_CASES.values():
        out.setdefault(c.key, c)
    return out
