"""Cases of tests/test_sfs_march_gpu.py: shape_from_shading's row-marching kernels (sfs_pcgMarch, sfs_costMarch in opt_amd/csrc/energy_sfs.hip) at many rows per workgroup.

SfsOps::marchGrid sizes the grid to the co-resident workgroup count (several hundred), so a small image gives every workgroup ONE row: the two-trip unrolled loop,
the by-name rotation of three row registers, the halo rows that read delta / CtC / b from row 0 and the eight XCD ranges with idle workgroups at their ends are then
only ever run in their degenerate form.  OPT_AMD_SFS_MARCH_GRID (a switch of the product build, read when the plan is made) replaces the co-resident count; the table
below picks (image, forced grid) pairs that put each regime of the march on a small image.  march_grid() restates marchGrid with the constants read from the sources,
so that a retune of SFS_MARCH_WAVES or kMaxPartials makes the table's claims fail (tests/test_sfs_march_cases_cpu.py) instead of silently testing something else.
"""
import os
import re
from collections import namedtuple

from opt_amd import workloads as wl

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opt_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern):
    m = re.findall(pattern, text, flags=re.M)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def constants():
    """The constants marchGrid and tileGrid are written in, from the sources themselves."""
    sfs, common = _read("energy_sfs.hip"), _read("common.h")
    assert re.search(r"kSfsMarchBlock = SFS_MARCH_WAVES \* kWave, kSfsSpan = kWave - 4;", sfs)          # columns a wave owns: its 64 lanes less a two-pixel ring on either side
    assert re.search(r"constexpr int kSfsTW = SFS_TW, kSfsTH = SFS_TH;", sfs)
    return {"waves": _int(sfs, r"^#define SFS_MARCH_WAVES (\d+)\b"), "wave": _int(common, r"^constexpr int kWave = (\d+);"),
            "max_partials": _int(common, r"^constexpr int kMaxPartials = (\d+);"), "tile_w": _int(sfs, r"^#define SFS_TW (\d+)\b"), "tile_h": _int(sfs, r"^#define SFS_TH (\d+)\b")}


Grid = namedtuple("Grid", "mgx mgy rows per launched last idle")


def march_grid(W, H, g, k=None):
    """SfsOps::marchGrid with `target` = g: column strips, row groups, rows per group, row groups per XCD range, workgroups launched; and from them the rows of the last
    group and the idle workgroup slots per column strip."""
    k = k or constants()
    div_up = lambda a, b: -(-a // b)
    mgx = div_up(W, k["waves"] * (k["wave"] - 4))
    mgy = max(1, min(H, g // mgx, (k["max_partials"] // 2 - 8 * mgx) // mgx))
    rows = div_up(H, mgy)
    mgy = div_up(H, rows)
    per = div_up(mgy, 8)
    return Grid(mgx, mgy, rows, per, 8 * per * mgx, H - (mgy - 1) * rows, 8 * per - mgy)


# (W, H, forced grid) -> what the table claims: rows per group, rows of the last group, row groups, idle slots per strip, groups per XCD range, column strips
Case = namedtuple("Case", "W H g rows last groups idle per strips gn lm what")
_C = lambda W, H, g, rows, last, groups, idle, per, strips, what, gn=True, lm=True: Case(W, H, g, rows, last, groups, idle, per, strips, gn, lm, what)
TABLE = [
    _C(61, 301, 1, 301, 301, 1, 7, 1, 1, "one workgroup marches everything, odd count"),
    _C(61, 301, 3, 101, 99, 3, 5, 1, 1, "odd rows, ragged last group"),
    _C(61, 301, 24, 13, 2, 24, 0, 3, 1, "two-row last group, several groups per XCD"),
    _C(123, 70, 2, 35, 35, 2, 6, 1, 1, "even split"),
    _C(123, 70, 24, 3, 1, 24, 0, 3, 1, "one-row last group"),
    _C(241, 103, 8, 26, 25, 4, 4, 1, 2, "second strip one column wide"),
    _C(241, 103, 40, 6, 1, 18, 6, 3, 2, "strips x groups x idle tail"),
    _C(481, 57, 12, 15, 12, 4, 4, 1, 3, "third strip one column wide"),
    _C(64, 99, 12, 9, 9, 11, 5, 2, 1, "idle tail with more than one group per XCD"),
    _C(7, 400, 12, 34, 26, 12, 4, 2, 1, "narrower than one wave's span, long march"),
    _C(5, 70, 3, 24, 22, 3, 5, 1, 1, "narrower than the ring", lm=False),                   # LM stalls after its first step on this image: Gauss-Newton only
    _C(130, 37, 8, 5, 2, 8, 0, 1, 1, "the on-chip tests' shape"),
    # the band is shorter than the halo; 300 x 2 reaches cost 0 after one step: probes only
    _C(300, 2, 1, 2, 2, 1, 7, 1, 2, "two rows in one group", gn=False, lm=False),
    _C(40, 1, 1, 1, 1, 1, 7, 1, 1, "a single row", gn=False, lm=False),
]
TRAJECTORY = [c for c in TABLE if c.gn or c.lm]
FLOAT_ROWS = [(61, 301, 3), (241, 103, 40), (123, 70, 24), (64, 99, 12)]
THREE_KERNEL_SHAPES = [(123, 70), (241, 103)]
TILE_LOOP_SHAPE = (1050, 500)              # 33 x 63 tiles of 32 x 8: more than the tiled kernels' grid may ever have (kMaxPartials / 2), ragged in both directions

GN_LITERS = [1, 2, 3, 9, 10]               # the first launch; the one that takes r.r from the private partials; odd and even launch counts
# name -> (steps, lIterations, controls) of the Levenberg-Marquardt runs
LM_RUNS = {
    "reset5": (3, 12, {"residual_reset_period": 5}),      # restart launches, sfs_applyTiled<T, true> as computeAdelta
    "default": (3, 12, {}),
    "rejected": (3, 12, {"trust_region_radius": 1e12}),   # the first steps are rejected: PCGInit1 with saveSSq = 0, the model-cost march
    "early_out": (3, 12, {"q_tolerance": 0.5}),
}


def case_id(c):
    return f"{c.W}x{c.H}-g{c.g}"


def case(W, H, g):
    return next(c for c in TABLE if (c.W, c.H, c.g) == (W, H, g))


def shapes(cases):
    """The distinct images of a list of cases, in table order: each is also run once on the natural grid."""
    out = []
    for c in cases:
        if (c.W, c.H) not in out:
            out.append((c.W, c.H))
    return out


def problem(W, H, double=True):
    return wl.shape_from_shading(W, H, double=double, seed=W + 3 * H, holes=True, noise=2e-3)


OracleRun = namedtuple("OracleRun", "cost0 ret cost radius x")
_RUNS = {}


def oracle_run(oracle_lib, W, H, double, kind, nsteps, liters, **controls):
    """The oracle's trajectory on a case's image: initial cost, then return value, cost and trust-region radius of every step, and the final unknowns.  The forced grids
    of one image and its natural-grid twin are all compared with the same run: computed once, never changed."""
    key = (W, H, double, kind, nsteps, liters, tuple(sorted(controls.items())))
    if key not in _RUNS:
        from helpers import flat_unknowns, oracle_solver
        P = problem(W, H, double)
        o = oracle_solver(oracle_lib, P, kind, nIterations=nsteps, lIterations=liters, **controls)
        o.init(P.params)
        run = OracleRun(o.cost(), [], [], [], None)
        while True:
            run.ret.append(o.step(P.params)); run.cost.append(o.cost()); run.radius.append(o.trust_region_radius())
            if not run.ret[-1]:
                break
        x = flat_unknowns(P)
        x.setflags(write=False)
        _RUNS[key] = run._replace(x=x)
        o.close()
    return _RUNS[key]
