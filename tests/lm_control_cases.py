"""Cases of the Levenberg-Marquardt outer-loop control tests (CPU-only to import): every LM path of the library x every scenario that drives the
accept / reject / exit logic of solverGPUGaussNewton.t:1119-1157 and the diagonal clamp of PCGFinalizeDiagonal (:631-664) off its defaults.

tests/test_lm_control_cases_cpu.py runs the oracle alone on every case and proves what the GPU tests depend on (which branch is reached at which step, the
share of clamped unknowns, that no decision is a close call); tests/test_lm_outer_controls_gpu.py steps the same cases side by side with the library.

A PATH names one way the library runs an LM step: the problem, the controls that select the path (both sides), the library-only switches, and what
kernel_timings() / on_chip_status() / describe() must say afterwards.  A SCENARIO is a set of controls, a number of outer steps, and parameter changes
applied between steps on both sides.
"""
from dataclasses import dataclass, field

import numpy as np

from opt_amd import workloads as wl
from helpers import active_mask, flat_unknowns, oracle_solver
import reference_cases as rc

NSTEPS, LITERS = 12, 10


# ---- paths ------------------------------------------------------------------------------------------------------------------------------------------------------
def _iw(W, H, jitter=0.0):
    return lambda double: wl.image_warping(W, H, double=double, random_state=5, mask_fraction=0.05, perturb=0.4, jitter_urshape=jitter)


def _poisson(W, H):
    def make(double):      # a random mask: unknowns with 0 .. 4 unknown neighbours, so the diagonal takes every value it can
        P = wl.poisson_image_editing(W, H, double=double, seed=4)
        P.params[2][...] = np.where(np.random.default_rng(104).random(P.params[2].shape) < 0.3, 255.0, 0.0)
        return P
    return make


def _hub(double):
    P = rc._arap_hub(17)
    return rc.as_double(P) if double else rc._f32(P)


@dataclass
class Path:
    family: str                  # kernel-set family: one float run per family
    make: object                 # double -> Problem
    liters: int = LITERS
    controls: dict = field(default_factory=dict)      # both sides
    hip: dict = field(default_factory=dict)           # library only
    onchip: bool = False
    kernels: tuple = ()          # names kernel_timings() must list
    absent: tuple = ()           # ... and must not
    describe: tuple = ()         # (key, substring) pairs of describe()
    float_too: bool = False


_RESET = dict(residual_reset_period=5)
PATHS = {
    # image_warping on the unit lattice
    "iw_onchip": Path("image_warping", _iw(61, 47), onchip=True, absent=("PCGIteration",), float_too=True),
    "iw_iter": Path("image_warping", _iw(130, 37), hip=dict(amd_onchip=0), kernels=("PCGIteration",)),
    # (the reference-order loop -- PCGStep1 / PCGStep2 / PCGStep3 per iteration -- behind the LMINIT march, which does PCGInit1 and PCGFinalizeDiagonal in one pass)
    "iw_reforder": Path("image_warping", _iw(61, 47), hip=dict(amd_reference_order=1), kernels=("PCGInit1", "PCGStep2", "PCGStep3+PCGStep1"),
                        absent=("PCGIteration", "PCGFinalizeDiagonal"), describe=(("path", "reference-order"),)),
    # ... and off it
    "iw_general_onchip": Path("image_warping", _iw(61, 47, 0.2), hip=dict(amd_onchip=4), onchip=True, absent=("PCGIteration",)),
    "iw_general_iter": Path("image_warping", _iw(61, 47, 0.2), hip=dict(amd_onchip=0), kernels=("PCGIteration",)),
    # the 5-point-stencil energies
    "poisson_onchip": Path("stencil", _poisson(40, 36), onchip=True, float_too=True),
    "poisson_reset": Path("stencil", _poisson(40, 36), liters=12, controls=_RESET, hip=dict(amd_onchip=2), onchip=True),
    "poisson_stream": Path("stencil", _poisson(130, 17), hip=dict(amd_onchip=0)),
    "flow_onchip": Path("stencil", lambda d: wl.optical_flow(37, 26, double=d, seed=2, init_flow=1.2), onchip=True),
    "flow_reset": Path("stencil", lambda d: wl.optical_flow(37, 26, double=d, seed=2, init_flow=1.2), liters=12, controls=_RESET, hip=dict(amd_onchip=2), onchip=True),
    "flow_stream": Path("stencil", lambda d: wl.optical_flow(37, 26, double=d, seed=2, init_flow=1.2), hip=dict(amd_onchip=0)),
    # shape_from_shading
    "sfs_onchip": Path("sfs", lambda d: wl.shape_from_shading(72, 56, double=d, seed=2), onchip=True, float_too=True),
    "sfs_reset": Path("sfs", lambda d: wl.shape_from_shading(72, 56, double=d, seed=2), liters=12, controls=_RESET, hip=dict(amd_onchip=3), onchip=True,
                      describe=(("path", "residual resets inside the solve"),)),
    "sfs_march": Path("sfs", lambda d: wl.shape_from_shading(130, 37, double=d, seed=2), hip=dict(amd_onchip=0)),
    # the mesh kernel set
    "arap_two_kernel": Path("arap", lambda d: wl.arap_mesh_deformation(36, 29, double=d, perturb=0.01), kernels=("PCGStep2+PCGStep3", "PCGStep1"), absent=("PCGStep3",),
                            float_too=True),
    "arap_onchip": Path("arap", lambda d: wl.arap_mesh_deformation(20, 20, double=d, perturb=0.01), hip=dict(amd_onchip=5), onchip=True, absent=("PCGStep1",)),
    "arap_hub": Path("arap", _hub, kernels=("PCGStep1",), absent=("packVertexRecords",)),
    "volumetric": Path("arap", lambda d: wl.volumetric_mesh_deformation(9, 7, 5, double=d, seed=5, perturb=0.05), kernels=("PCGStep1",)),
    # the graph functor engine: k_finalizeDiagonal in graph mode
    "cotangent": Path("graph", lambda d: wl.cotangent_mesh_smoothing(19, 13, double=d, seed=6), kernels=("PCGFinalizeDiagonal",), float_too=True),
    "embedded": Path("graph", lambda d: wl.embedded_mesh_deformation(17, 11, double=d, seed=7, perturb=0.03), kernels=("PCGFinalizeDiagonal",)),
}
# Paths on which the SSq saved at the first step differs from guardedInvert of a later step's diagonal: the preconditioned energies whose diag(J^T J) depends on the
# unknowns.  (image_warping's does not; poisson, optical_flow and shape_from_shading do not precondition: their SSq is the constant guardedInvert(1) = 1 / 4.)
SSQ_MOVES = ["arap_two_kernel", "arap_onchip", "arap_hub", "volumetric", "cotangent", "embedded"]
FLOAT_PATHS = [n for n, p in PATHS.items() if p.float_too]

_PROBLEMS = {}


def problem(path, double=True):
    """A fresh copy of the path's problem (built once per session)."""
    k = (path, double)
    if k not in _PROBLEMS:
        _PROBLEMS[k] = PATHS[path].make(double)
    return _PROBLEMS[k].clone()


def set_flat(P, x):
    """Write the flat unknown vector x back into P's unknown arrays."""
    o = 0
    for s in P.unknown_slots:
        a = np.asarray(P.params[s])
        P.params[s] = np.ascontiguousarray(x[o:o + a.size].reshape(a.shape).astype(a.dtype))
        o += a.size
    return P


def perturbed(P, seed=1):
    """P with its active unknowns moved by 1e-3 of their rms: the input of the second Opt_ProblemInit on a used plan."""
    P = P.clone()
    x = flat_unknowns(P).astype(np.float64)
    m = active_mask(P)
    x[m] += 1e-3 * np.sqrt(np.mean(x[m] ** 2)) * np.random.default_rng(seed).standard_normal(int(m.sum()))
    return set_flat(P, x)


# ---- scenarios --------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Scenario:
    controls: dict
    nsteps: int = NSTEPS
    changes: dict = field(default_factory=dict)      # {k: {parameter: value}}: set on both sides after step k has returned
    ends: str = ""               # what the CPU file proves of the oracle's run: "ftol" / "minradius" (the exit taken), "cap", ""


FTOL = Scenario(dict(function_tolerance=0.3), ends="ftol")
MINRADIUS = Scenario(dict(min_relative_decrease=0.95, min_trust_region_radius=1e3))
# every step rejected: 1e4 -> 5000 -> 1250 -> 156.25 <= 1e3 (a relative decrease of 2 would mean the cost fell twice as far as the model promised)
MINRADIUS_FORCED = Scenario(dict(min_relative_decrease=2.0, min_trust_region_radius=1e3), ends="minradius")
# radius_decrease_factor starts at 8: two rejections (/ 8, / 16), an accepted step (the factor back to 2), two rejections (/ 2, / 4)
FACTOR8 = Scenario(dict(radius_decrease_factor=8.0, min_relative_decrease=2.0), nsteps=5, changes={2: dict(min_relative_decrease=1e-3), 3: dict(min_relative_decrease=2.0)})
CAP = Scenario(dict(max_trust_region_radius=2e4), nsteps=6, ends="cap")
# captured at Opt_ProblemInit (solver.t:996-1001): changing them after step 2 changes nothing
CAPTURED = dict(trust_region_radius=77.0, radius_decrease_factor=8.0, min_lm_diagonal=0.3, max_lm_diagonal=0.4)
# (step 2 and step 3 are rejected whatever they do -- min_relative_decrease = 2 -- so the decrease factor in force shows: 2 then 4, not the 8 set in between)
_LATE = {1: dict(min_relative_decrease=2.0), 3: dict(min_relative_decrease=1e-3)}
LATE_CAPTURED = Scenario({}, nsteps=5, changes={**_LATE, 2: CAPTURED})
LATE_NOTHING = Scenario({}, nsteps=5, changes=_LATE)
# read at every step (solver.t:1020-1023): changing them after step 2 acts on step 3
LATE_FTOL = Scenario({}, nsteps=5, changes={2: dict(function_tolerance=0.999)})
LATE_REJECT_EXIT = Scenario({}, nsteps=5, changes={2: dict(min_relative_decrease=2.0, min_trust_region_radius=1e30)})
LATE_CAP = Scenario({}, nsteps=5, changes={2: dict(max_trust_region_radius=123.0)})

FIXED = {"ftol": FTOL, "minradius": MINRADIUS, "minradius_forced": MINRADIUS_FORCED, "factor8": FACTOR8, "cap": CAP, "late_captured": LATE_CAPTURED,
         "late_nothing": LATE_NOTHING, "late_ftol": LATE_FTOL, "late_reject_exit": LATE_REJECT_EXIT, "late_cap": LATE_CAP}
CLAMP = ["clamp", "clamp_reject", "clamp_095", "clamp_upper", "clamp_lower"]
SCENARIOS = list(FIXED) + CLAMP
# min_relative_decrease = 0.95 as the issue of these tests sets it, on the energies it quotes (image_warping, ARAP, optical_flow, cotangent).  The other inputs decide
# some step within 1 % of 0.95 (shape_from_shading's ninth: 0.9502): they take the min-radius exit in "minradius_forced" only.
MINRADIUS_PATHS = ["iw_onchip", "iw_iter", "iw_reforder", "iw_general_onchip", "iw_general_iter", "flow_onchip", "flow_reset", "flow_stream", "arap_two_kernel",
                   "arap_onchip", "cotangent"]
# (for the same reason "clamp_095" leaves out arap_hub: its second and third steps decide at 0.960)


def cases(paths=None):
    """(path, scenario name) of every case"""
    return [(p, s) for p in (paths or PATHS) for s in SCENARIOS if (s != "minradius" or p in MINRADIUS_PATHS) and (s != "clamp_095" or p != "arap_hub")]


# float runs the GPU file leaves out, with the reason
FLOAT_EXCLUDED = {}


def float_cases():
    return [(p, s) for p, s in cases(FLOAT_PATHS) if s not in FLOAT_EXCLUDED.get(p, {})]


_RUNS = {}


def oracle_run(oracle_lib, path, name, double=True):
    """run_oracle on the path's own problem, once per session"""
    k = (path, name, double)
    if k not in _RUNS:
        _RUNS[k] = run_oracle(oracle_lib, path, scenario(oracle_lib, path, name), double)
    return _RUNS[k]


def margin_bar(sc_controls):
    """How far (relative) every accept / reject / exit decision of the oracle must lie from its threshold: 10 %.  Under min_relative_decrease = 0.95 an accepted step
    cannot do that -- a relative decrease of 1, the model being exact, lies 1 / 0.95 - 1 = 5.3 % above it, and the runs the controls were chosen for (image_warping, ARAP:
    accepted at 0.997-1.000, rejected at 0.90-0.91) decide at 4-5 %: two thirds of the attainable, 3.5 %, is asked there, 1e7 x the double cost bar."""
    return 0.035 if abs(sc_controls.get("min_relative_decrease", 0) - 0.95) < 1e-6 else 0.1


def margins(run):
    """per step: the relative distance of relative_decrease from min_relative_decrease, and -- accepted steps -- of cost_change from prevCost * function_tolerance"""
    out = []
    for d in run.decisions:
        m = abs(d["relative_decrease"] / d["mrd"] - 1.0)
        if d["accepted"]:
            m = min(m, abs(d["cost_change"] / (d["prev"] * d["ftol"]) - 1.0))
        out.append(m)
    return out
REINIT_AFTER = ["ftol", "minradius_forced", "clamp"]      # a second Opt_ProblemInit on the used plan must re-seed radius, decrease factor and SSq
SOLVE = ["ftol", "minradius_forced"]
SOLVE_PATHS = ["iw_onchip", "poisson_onchip", "sfs_onchip", "arap_two_kernel", "cotangent"]


def guarded_invert(d):
    s = 1.0 + np.sqrt(d)
    return 1.0 / (s * s)


def first_step_rho(oracle_lib, path):
    """rho = d * SSq over the active unknowns at the first step (double): d the raw diag(J^T J), SSq what PCGSaveSSq keeps.  PCGFinalizeDiagonal clamps
    CtC = d / radius between min_lm_diagonal / (SSq radius) and max_lm_diagonal / (SSq radius): from below iff rho < min_lm_diagonal, from above iff rho > max_lm_diagonal."""
    P = problem(path)
    o = oracle_solver(oracle_lib, P, "LMGPU", nIterations=1, lIterations=1)
    _, d = o.eval_jtf(P.params)
    o.init(P.params); o.step(P.params)
    ssq = o.vector("SSq")
    o.close()
    return (d * ssq)[active_mask(problem(path))]


def _candidates(rho, clearance):
    """Bounds a float32 parameter can take between neighbouring distinct values of rho, at least `clearance` (relative) away from every rho."""
    u = np.unique(rho)
    mids = np.float32(0.5 * (u[:-1] + u[1:])).astype(np.float64)
    ok = (mids - u[:-1] >= 1.001 * clearance * mids) & (u[1:] - mids >= 1.001 * clearance * mids)
    return mids[ok]


# rho of poisson_image_editing takes three values -- 1 at the four image corners (0.2 % of the unknowns), 1.5 on the image border, 2 inside: no three classes of
# 10 % exist, so lo = hi between border and interior: two classes, every unknown clamped to one value.
TWO_CLASSES = {"poisson_onchip", "poisson_reset", "poisson_stream"}
# rho of these inputs is continuous with thousands of distinct values a few 1e-5 (relative) apart where most of them lie: no bound inside the middle 80 % keeps
# 1e-3 from its neighbours.  Their bounds keep 1e-5 instead -- still 1e6 x the 1e-11 to which the library's diagonal is held to the oracle's in double
# (tests/test_energies_gpu.py) -- and they are not run in float.
CLEARANCE = {"flow_onchip": 1e-5, "flow_reset": 1e-5, "flow_stream": 1e-5, "iw_general_onchip": 1e-5, "iw_general_iter": 1e-5}
_BOUNDS = {}


def clamp_bounds(oracle_lib, path):
    """(min_lm_diagonal, max_lm_diagonal) for the path, derived from rho: among the candidate pairs lo < hi the one whose smallest class (low-clamped, free,
    high-clamped) is largest -- bounds near the terciles of rho, a little outside the 30th / 70th percentiles."""
    if path not in _BOUNDS:
        rho = first_step_rho(oracle_lib, path)
        c = _candidates(rho, CLEARANCE.get(path, 1e-3))
        assert len(c) >= 1, (path, np.unique(rho)[:20])
        below = np.array([(rho < m).mean() for m in c])
        if path in TWO_CLASSES:
            i = int(np.argmax(np.minimum(below, 1 - below)))
            _BOUNDS[path] = (float(c[i]), float(c[i]))
        else:
            best, pair = -1.0, None
            for i in range(len(c) - 1):
                worst = np.minimum(np.minimum(below[i], below[i + 1:] - below[i]), 1 - below[i + 1:])
                if worst.max() > best:
                    best, pair = float(worst.max()), (i, i + 1 + int(np.argmax(worst)))
            _BOUNDS[path] = (float(c[pair[0]]), float(c[pair[1]]))
    return _BOUNDS[path]


def class_shares(rho, lo, hi):
    """shares of the low-clamped, free and high-clamped unknowns"""
    return float((rho < lo).mean()), float(((rho >= lo) & (rho <= hi)).mean()), float((rho > hi).mean())


def scenario(oracle_lib, path, name):
    if name in FIXED:
        return FIXED[name]
    lo, hi = clamp_bounds(oracle_lib, path)
    if name == "clamp":
        return Scenario(dict(min_lm_diagonal=lo, max_lm_diagonal=hi), nsteps=5)
    if name == "clamp_reject":      # a rejected step between accepted ones: SSq and the bounds stay, the radius (and with it every clamped value) moves
        return Scenario(dict(min_lm_diagonal=lo, max_lm_diagonal=hi), nsteps=7, changes={1: dict(min_relative_decrease=2.0), 2: dict(min_relative_decrease=1e-3)})
    if name == "clamp_095":
        return Scenario(dict(min_lm_diagonal=lo, max_lm_diagonal=hi, min_relative_decrease=0.95), nsteps=3)
    if name == "clamp_upper":
        return Scenario(dict(max_lm_diagonal=hi), nsteps=5)
    if name == "clamp_lower":
        return Scenario(dict(min_lm_diagonal=lo), nsteps=5)
    raise KeyError(name)


def all_controls(path, sc):
    p = PATHS[path]
    return dict(nIterations=sc.nsteps, lIterations=p.liters, **p.controls, **sc.controls)


# ---- the oracle alone -------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Run:
    ret: list
    cost: list                   # cost() before the first step and after every step
    radius: list                 # after every step
    x: np.ndarray                # final unknowns
    decisions: list = None       # per step: dict(prev, new, model_change, cost_change, relative_decrease, mrd, ftol, factor, accepted)


def run_oracle(oracle_lib, path, sc, double=True, P=None):
    """The scenario on the oracle.  decisions: per step, what the accept / reject / exit tests compared (OracleSolver.last_decision)."""
    P = problem(path, double) if P is None else P.clone()
    o = oracle_solver(oracle_lib, P, "LMGPU", **all_controls(path, sc))
    live = {"min_relative_decrease": 1e-3, "function_tolerance": 1e-6}
    live.update({k: v for k, v in sc.controls.items() if k in live})
    o.init(P.params)
    run = Run([], [o.cost()], [], None, [])
    for k in range(1, sc.nsteps + 2):
        a = o.step(P.params)
        run.ret.append(a); run.cost.append(o.cost()); run.radius.append(o.trust_region_radius())
        if k <= sc.nsteps:
            prev, new, model_change, factor = o.last_decision()
            cc = prev - new
            mrd, ftol = float(np.float32(live["min_relative_decrease"])), float(np.float32(live["function_tolerance"]))
            run.decisions.append(dict(prev=prev, new=new, model_change=model_change, cost_change=cc, relative_decrease=cc / model_change, mrd=mrd, ftol=ftol, factor=factor,
                                      accepted=bool(cc >= 0 and cc / model_change > mrd)))
        if not a:
            break
        for name, v in sc.changes.get(k, {}).items():
            o.set(name, v)
            if name in live:
                live[name] = v
    run.x = flat_unknowns(P).copy()
    o.close()
    return run
