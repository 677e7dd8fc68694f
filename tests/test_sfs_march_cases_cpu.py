"""CPU tests of tests/sfs_march_cases.py: what tests/test_sfs_march_gpu.py depends on, proved without a GPU.

  * march_grid() restates SfsOps::marchGrid with SFS_MARCH_WAVES and kMaxPartials read from the sources; every row of the case table is in the regime it claims (rows per
    workgroup, rows of the last group, row groups, idle workgroup slots per column strip, row groups per XCD range, column strips), and the table as a whole holds every
    regime the GPU file is for;
  * the tile-loop image has more tiles than the tiled kernels' grid can have;
  * the oracle alone on every trajectory case: a positive initial cost, at least 90 % of the unknowns active, a first step that lowers the cost; the early-out run does end
    its linear solves early, and the one rejected step the cases contain is where the GPU file's docstring says it is.
"""
import numpy as np
import pytest

import sfs_march_cases as sc
from helpers import active_mask


def test_constants_are_read_from_the_sources():
    k = sc.constants()
    assert k == {"waves": 4, "wave": 64, "max_partials": 4096, "tile_w": 32, "tile_h": 8}, k      # the values the table was computed with


@pytest.mark.parametrize("c", sc.TABLE, ids=sc.case_id)
def test_case_is_in_its_regime(c):
    g = sc.march_grid(c.W, c.H, c.g)
    assert (g.rows, g.last, g.mgy, g.idle, g.per, g.mgx) == (c.rows, c.last, c.groups, c.idle, c.per, c.strips), g
    assert g.launched == 8 * c.per * c.strips and g.launched <= sc.constants()["max_partials"] // 2
    assert (c.groups - 1) * c.rows + c.last == c.H and 1 <= c.last <= c.rows


def test_the_table_holds_every_regime():
    t = sc.TRAJECTORY
    assert any(c.groups == 1 and c.rows == c.H for c in t)                                  # one workgroup marches the whole image
    assert {c.last for c in t if c.groups > 1 and c.last < c.rows} >= {1, 2}                # a last group of one row and of two
    assert {c.rows % 2 for c in t} == {0, 1} and {c.last % 2 for c in t} == {0, 1}          # trip counts that are and are not a multiple of the unroll
    assert any(c.per > 1 and c.idle > 0 for c in t) and any(c.per > 1 and c.idle == 0 for c in t) and any(c.per == 1 and c.idle > 0 for c in t)
    assert any(c.strips > 1 and c.groups > 1 and c.idle > 0 and c.per > 1 for c in t)       # strips x groups x idle tail
    span = sc.constants()["waves"] * (sc.constants()["wave"] - 4)
    assert any(c.W % span == 1 and c.strips == 2 for c in t) and any(c.W % span == 1 and c.strips == 3 for c in t)      # a last strip one column wide
    assert any(c.W < sc.constants()["wave"] - 4 for c in t) and any(c.W <= 5 for c in t)
    assert all(c.rows > 1 for c in t)                                                       # no trajectory case is the one-row regime the rest of the suite runs
    assert all(sc.case(*r) in t for r in sc.FLOAT_ROWS) and all(s in sc.shapes(t) for s in sc.THREE_KERNEL_SHAPES)
    assert [(c.W, c.H) for c in sc.TABLE if not (c.gn or c.lm)] == [(300, 2), (40, 1)] and [(c.W, c.H) for c in t if not c.lm] == [(5, 70)]


def test_tile_loop_image_has_more_tiles_than_the_grid_may_have():
    k = sc.constants()
    W, H = sc.TILE_LOOP_SHAPE
    tx, ty = -(-W // k["tile_w"]), -(-H // k["tile_h"])
    assert (tx, ty) == (33, 63) and tx * ty > k["max_partials"] // 2                        # tileGrid's cap whatever the occupancy query returns
    assert W % k["tile_w"] and H % k["tile_h"]                                              # ragged in both directions


def _runs(c):
    out = [("gaussNewtonGPU", 2, 9, {})] if c.gn else []
    if c.lm:
        out += [("LMGPU", n, l, kw) for n, l, kw in sc.LM_RUNS.values()]
    return out


@pytest.mark.parametrize("W,H", sc.shapes(sc.TRAJECTORY))
def test_oracle_alone_on_the_trajectory_images(oracle_lib, W, H):
    c = next(c for c in sc.TRAJECTORY if (c.W, c.H) == (W, H))
    P = sc.problem(W, H)
    assert active_mask(P).mean() >= 0.9
    for kind, nsteps, liters, kw in _runs(c):
        r = sc.oracle_run(oracle_lib, W, H, True, kind, nsteps, liters, **kw)
        print(W, H, kind, kw, r.cost0, r.cost, r.ret, r.radius)
        assert r.cost0 > 0 and r.ret == [1] * nsteps + [0]
        assert r.cost[0] < r.cost0                                                          # the first step is accepted and lowers the cost
        assert np.all(np.isfinite(r.x)) and not r.x.flags.writeable


@pytest.mark.parametrize("W,H", [s for s in sc.shapes(sc.TRAJECTORY) if s != (5, 70)])
def test_lm_runs_reach_their_branches(oracle_lib, W, H):
    run = lambda name: sc.oracle_run(oracle_lib, W, H, True, "LMGPU", *sc.LM_RUNS[name][:2], **sc.LM_RUNS[name][2])
    plain, early, wide = run("default"), run("early_out"), run("rejected")
    # q_tolerance = 0.5 ends the first linear solve after a few of its 12 iterations: a visibly different step (481 x 57: a better one)
    assert abs(early.cost[0] / plain.cost[0] - 1) > 0.01
    # A radius of 1e12 leaves CtC at its lower clamp: an (almost) undamped step.  On these images the oracle ACCEPTS it -- the radius grows from 1e12 -- so this run
    # checks the clamp and the float radius parameter, not a rejection ...
    assert wide.radius[0] > 1e12 and abs(wide.cost[0] / plain.cost[0] - 1) > 1e-6
    # ... and the rejected step of the table (unknowns restored, radius halved, PCGInit1 again with the saved SSq, the model-cost march in front of it) is the third
    # step of 7 x 400, in every LM run
    for r in (plain, run("reset5"), wide, early):
        rejected = [i for i in range(1, 3) if r.cost[i] == r.cost[i - 1]]
        assert rejected == ([2] if (W, H) == (7, 400) and r is not early else []), (rejected, r.cost)
        for i in rejected:
            assert r.radius[i] == 0.5 * r.radius[i - 1]
