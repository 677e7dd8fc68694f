"""CPU tests of tests/lm_control_cases.py: the oracle alone on every case of the Levenberg-Marquardt outer-loop control tests.

tests/test_lm_outer_controls_gpu.py compares the library with the oracle on these cases; what it depends on is proved here, without a GPU:
  * the runs the cases were chosen for: which step takes the function-tolerance exit, the radii of the min-radius exits, the capped radii;
  * every scenario reaches its branch on every path (an exit really is that exit, the cap really binds, a late parameter acts on step 3 or never);
  * the diagonal clamp's bounds split the active unknowns into classes of at least 10 %, the oracle's own CtC confirms the classes, the clamped run differs from the
    default one, and from the second step on the saved SSq is not the current diagonal's;
  * no accept / reject / exit decision is a close call (lm_control_cases.margin_bar), so that a difference of 1e-10 -- or of 1e-3 in float -- cannot flip one;
  * the float oracle decides like the double one wherever the GPU file runs float.
"""
import numpy as np
import pytest

import lm_control_cases as lc
from helpers import active_mask, oracle_solver

QUOTED_FTOL_EXIT = {"cotangent": 1, "iw_onchip": 2, "sfs_onchip": 3, "embedded": 4, "arap_two_kernel": 5}      # function_tolerance = 0.3: the step that returns 0


def test_every_family_has_a_float_path_and_every_scenario_a_case():
    assert {lc.PATHS[p].family for p in lc.FLOAT_PATHS} == {p.family for p in lc.PATHS.values()}
    assert {s for _, s in lc.cases()} == set(lc.SCENARIOS)
    assert set(lc.SOLVE_PATHS) <= set(lc.PATHS) and set(lc.REINIT_AFTER + lc.SOLVE) <= set(lc.SCENARIOS)


@pytest.mark.parametrize("path,step", sorted(QUOTED_FTOL_EXIT.items()))
def test_function_tolerance_exit_steps(oracle_lib, path, step):
    r = lc.oracle_run(oracle_lib, path, "ftol")
    assert r.ret == [1] * (step - 1) + [0], r.ret
    d = r.decisions[-1]
    assert d["accepted"] and d["cost_change"] <= d["prev"] * d["ftol"]
    assert r.cost[-1] == d["prev"] and r.cost[-1] == r.cost[-2]            # cost() keeps the previous cost (solver.t:1129-1132) ...
    P = lc.set_flat(lc.problem(path), r.x)                                 # ... while the unknowns are the updated ones
    o = oracle_solver(oracle_lib, P)
    assert o.eval_cost(P.params) == pytest.approx(d["new"], rel=1e-12) and d["new"] < d["prev"]
    o.close()
    if path == "cotangent":
        assert r.cost[0] == pytest.approx(125.4, rel=1e-3) and d["new"] == pytest.approx(106.6, rel=1e-3)


@pytest.mark.parametrize("path", ["iw_onchip", "arap_two_kernel", "flow_onchip"])
def test_min_radius_exit_after_an_accepted_step(oracle_lib, path):
    r = lc.oracle_run(oracle_lib, path, "minradius")
    assert r.ret == [1, 1, 1, 0] and r.radius == pytest.approx([3e4, 1.5e4, 3750.0, 468.75], rel=1e-12)
    assert [d["accepted"] for d in r.decisions] == [True, False, False, False]
    first = lc.run_oracle(oracle_lib, path, lc.Scenario(lc.MINRADIUS.controls, nsteps=1))
    assert np.array_equal(r.x, first.x)                                    # reverted at the exit: the unknowns of the one accepted step


def test_min_radius_exit_cotangent(oracle_lib):
    r = lc.oracle_run(oracle_lib, "cotangent", "minradius")
    assert r.ret == [1, 1, 0] and r.radius == pytest.approx([5000.0, 1250.0, 156.25], rel=1e-12)
    assert np.array_equal(r.x, lc.flat_unknowns(lc.problem("cotangent")))


def test_radius_cap_quoted(oracle_lib):
    assert lc.oracle_run(oracle_lib, "sfs_onchip", "cap").radius[:6] == [2e4] * 6
    r = lc.oracle_run(oracle_lib, "iw_onchip", "cap").radius
    assert r[0] == 2e4 and r[1] == pytest.approx(2e4, rel=1e-3) and r[2] < 0.7 * r[1]


@pytest.mark.parametrize("path,name", lc.cases())
def test_scenario_reaches_its_branch_and_decides_with_margin(oracle_lib, path, name):
    sc = lc.scenario(oracle_lib, path, name)
    r = lc.oracle_run(oracle_lib, path, name)
    m = lc.margins(r)
    print(path, name, "ret", r.ret, "radius", r.radius, "margins", m)
    assert min(m) >= lc.margin_bar(sc.controls), (m, r.decisions)
    last = r.decisions[-1]
    if name == "ftol":
        assert r.ret[-1] == 0 and len(r.ret) <= sc.nsteps and last["accepted"] and last["cost_change"] <= last["prev"] * last["ftol"]
    if name in ("minradius", "minradius_forced"):
        assert r.ret[-1] == 0 and len(r.ret) <= sc.nsteps and not last["accepted"] and r.radius[-1] <= 1e3
        assert all(x > 1e3 for x in r.radius[:-1])
    if name == "minradius_forced":
        assert r.ret == [1, 1, 0] and r.radius == [5000.0, 1250.0, 156.25]
    if name == "factor8":
        assert [d["accepted"] for d in r.decisions] == [False, False, True, False, False] and [d["factor"] for d in r.decisions] == [16.0, 32.0, 2.0, 4.0, 8.0]
        assert r.radius[:2] == [1250.0, 78.125] and r.radius[3] == r.radius[2] / 2 and r.radius[4] == r.radius[2] / 8
    if name == "cap":
        if path == "cotangent":      # its first step earns no growth (relative decrease 0.5) and the radius only falls from there: "late_cap" is where its cap binds
            assert max(r.radius) < 2e4 and lc.oracle_run(oracle_lib, path, "late_cap").radius[2] == 123.0
        else:                        # the first accepted step's x 3 (a relative decrease above 0.79) is capped
            assert r.radius[0] == 2e4 and r.decisions[0]["accepted"] and r.decisions[0]["relative_decrease"] > 0.79
    if name == "late_ftol":
        assert r.ret[:2] == [1, 1]
        if r.decisions[2]["accepted"]:                                     # (optical_flow and poisson with resets reject their third step: nothing to exit from)
            assert r.ret == [1, 1, 0]                                      # acts on step 3
    if name == "late_reject_exit":
        assert r.ret == [1, 1, 0] and not r.decisions[2]["accepted"]
    if name == "late_cap":
        if r.decisions[2]["accepted"]:                                     # (the cap is applied where a step is accepted, solver.t:1139)
            assert r.radius[2] == 123.0
        assert r.radius[1] > 123.0 and all(r.radius[i] <= 123.0 for i in range(2, len(r.decisions)) if r.decisions[i]["accepted"] and r.ret[i])
    if name == "late_captured":
        plain = lc.oracle_run(oracle_lib, path, "late_nothing")
        assert (r.ret, r.cost, r.radius) == (plain.ret, plain.cost, plain.radius) and np.array_equal(r.x, plain.x)
        assert [d["accepted"] for d in r.decisions[1:3]] == [False, False] and [d["factor"] for d in r.decisions[1:3]] == [4.0, 8.0]
    if name in ("clamp_reject",):
        acc = [d["accepted"] for d in r.decisions]      # a rejected step between two accepted ones (optical_flow rejects on its own until the radius has come down to 29)
        assert acc[:2] == [True, False] and True in acc[2:], acc
    if name in lc.CLAMP and name != "clamp_095":
        assert r.ret[:5] == [1] * 5                                        # at least five outer steps
        plain = lc.run_oracle(oracle_lib, path, lc.Scenario({k: v for k, v in sc.controls.items() if "lm_diagonal" not in k}, sc.nsteps, sc.changes))
        moved = max(abs(a - b) / abs(b) for a, b in zip(r.cost[1:], plain.cost[1:]))
        print("   the clamp moves the costs by", moved)
        assert moved > 1e-7                                                # 1000 x the double cost bar: a kernel that ignores the bounds fails it


@pytest.mark.parametrize("path", list(lc.PATHS))
def test_clamp_classes(oracle_lib, path):
    rho = lc.first_step_rho(oracle_lib, path)
    lo, hi = lc.clamp_bounds(oracle_lib, path)
    assert lo == float(np.float32(lo)) and hi == float(np.float32(hi))
    assert np.min(np.abs(rho / lo - 1)) >= lc.CLEARANCE.get(path, 1e-3) and np.min(np.abs(rho / hi - 1)) >= lc.CLEARANCE.get(path, 1e-3)
    low, free, high = lc.class_shares(rho, lo, hi)
    print(path, "bounds", lo, hi, "shares", low, free, high, "distinct", len(np.unique(rho)))
    if path in lc.TWO_CLASSES:
        assert lo == hi and low >= 0.1 and high >= 0.1 and len(np.unique(rho)) == 3 and (rho == rho.min()).mean() < 0.01
    else:
        assert lo < hi and min(low, free, high) >= 0.1
    # the oracle's own first step: which unknowns PCGFinalizeDiagonal moved
    P = lc.problem(path)
    sc = lc.scenario(oracle_lib, path, "clamp")
    o = oracle_solver(oracle_lib, P, "LMGPU", **lc.all_controls(path, sc))
    _, d = o.eval_jtf(P.params)
    o.init(P.params)
    radius = 1e4
    o.step(P.params)
    m = active_mask(lc.problem(path))
    ctc, unclamped = o.vector("CtC")[m], (d / radius)[m]
    assert ((ctc > unclamped * (1 + 1e-9)).mean(), (ctc < unclamped * (1 - 1e-9)).mean()) == pytest.approx((low, high), abs=1e-12)
    o.close()


@pytest.mark.parametrize("path", lc.SSQ_MOVES)
def test_saved_ssq_is_not_the_current_diagonal_from_step_2_on(oracle_lib, path):
    """A kernel that clamped against guardedInvert of the CURRENT diagonal instead of the SSq saved at the first step would write other bounds, min_lm_diagonal /
    (SSq radius): at the second step's unknowns the two differ by more than 1e-6 -- 1e4 x the double cost bar -- on at least 10 % of the active unknowns, clamped ones."""
    P = lc.problem(path)
    sc = lc.scenario(oracle_lib, path, "clamp")
    lo, hi = lc.clamp_bounds(oracle_lib, path)
    o = oracle_solver(oracle_lib, P, "LMGPU", **lc.all_controls(path, sc))
    o.init(P.params)
    assert o.step(P.params) == 1
    ssq = o.vector("SSq")
    _, d = o.eval_jtf(P.params)
    o.close()
    m = active_mask(lc.problem(path))
    rho = (d * ssq)[m]
    off = np.abs(lc.guarded_invert(d[m]) / ssq[m] - 1.0)
    share = float((((rho < lo) | (rho > hi)) & (off > 1e-6)).mean())
    print(path, "clamped unknowns whose bound would move by more than 1e-6:", share, "median move", float(np.median(off)))
    assert share >= 0.1


@pytest.mark.parametrize("path,name", lc.float_cases())
def test_float_oracle_decides_like_the_double_one(oracle_lib, path, name):
    sc = lc.scenario(oracle_lib, path, name)
    f, d = lc.oracle_run(oracle_lib, path, name, double=False), lc.oracle_run(oracle_lib, path, name)
    assert f.ret == d.ret and [x["accepted"] for x in f.decisions] == [x["accepted"] for x in d.decisions]
    assert f.radius == pytest.approx(d.radius, rel=1e-2)
    assert min(lc.margins(f)) >= 0.5 * lc.margin_bar(sc.controls), lc.margins(f)
