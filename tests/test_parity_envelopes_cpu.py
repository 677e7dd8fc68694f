"""CPU tests of the yardstick behind every parity bar above the contract (tests/golden/parity_bars.json, tests/golden/parity_envelopes.json).

A bar above 1e-12 (double) / 1e-5 (float) is twice the diameter of a frozen ensemble of legal oracle runs of the same case (tests/helpers.py::assert_close,
tests/golden/make_parity_envelopes.py), never a multiple of what the library itself produced.  Nothing here needs a GPU:
  * every entry above the contract names an envelope that exists, and it is the envelope of the case the test builds (tests/parity_cases.py::ENTRY_CASES);
  * the inputs the envelope was computed from are the inputs the test builds today (checksum over settings and every bound array);
  * no bar exceeds the value it had as 10 x the library's own error, the table's bar is what the rule gives, and the bar in force at any step is never above the table's;
  * the ensemble is the fixed 34 runs for every case: {plain, fma} x {exact order, seeds 1 .. 16};
  * leave-one-out: every legal run lies within the bar the other 33 would set (max(contract, 2 x their diameter)) at every step -- else the ensemble is too small a yardstick;
  * the smallest case, run again on the oracle, reproduces its frozen exact-order costs.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import helpers
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
BARS = json.load(open(os.path.join(HERE, "golden", "parity_bars.json")))
FILE = json.load(open(os.path.join(HERE, "golden", "parity_envelopes.json")))
ENVS = FILE["cases"]
RUNS = np.load(os.path.join(HERE, "golden", FILE["meta"]["runs"]))      # every run behind the summaries: deviations from run 0
CONTRACT = helpers.CONTRACT
LABELS = [("exact-order " if s == 0 else f"reference-order seed {s} ") + v for v in ("plain", "fma") for s in range(17)]


def _tool():
    spec = importlib.util.spec_from_file_location("make_parity_bars", os.path.join(os.path.dirname(HERE), "tools", "make_parity_bars.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _split(key):
    tp, prec, kind = key.split("|")
    test, _, par = tp.partition("[")
    return test, ("[" + par) if par else "", prec, kind


def _above():
    return {k: e for k, e in BARS.items() if _split(k)[2] in CONTRACT and e["bar"] > CONTRACT[_split(k)[2]]}


def _named(key, e):
    """{parametrisation: envelope key} an entry names (a function-level entry names ENTRY_CASES: one envelope per parametrisation of its test)"""
    test, par, _, _ = _split(key)
    if "envelope" in e:
        return {par: e["envelope"]}
    if "envelopes" in e:
        assert e["envelopes"] == "ENTRY_CASES", key
        named = {k[len(test):]: helpers.envelope_name(e, test, k[len(test):]) for k in pc.ENTRY_CASES if k.startswith(test + "[")}
        return {p: n for p, n in named.items() if _split(key)[3] != "radius" or pc.ENTRY_CASES[test + p].kind == "LMGPU"}      # (a Gauss-Newton case has no radius)
    return {}


def _runs(env, q):
    """values[run][step] of 'costs' / 'radius'"""
    return np.asarray(env[q], dtype=np.float64)[None, :] + RUNS[f"{q}_{env['row']}"].astype(np.float64)


def test_every_bar_above_the_contract_names_the_envelope_of_its_case():
    above = _above()
    assert above, "the table has entries above the contract; an empty selection means this test looks at nothing"
    for key, e in above.items():
        test, _, _, _ = _split(key)
        named = _named(key, e)
        assert named, ("above the contract without an envelope", key)
        for par, name in named.items():
            assert name in ENVS, (key, par, name)
            assert (test + par) in pc.ENTRY_CASES and pc.ENTRY_CASES[test + par].key == name, (key, par, name)


def test_every_entry_that_names_an_envelope_names_one_that_exists():
    n = 0
    for key, e in BARS.items():
        for par, name in _named(key, e).items():
            assert name in ENVS, (key, par, name)
            n += 1
    assert n >= 65


def test_envelope_inputs_are_the_inputs_the_tests_build_today():
    cases = pc.envelope_cases()
    assert set(cases) == set(ENVS)
    for key, case in cases.items():
        P = case.problem()
        assert case.checksum(P) == ENVS[key]["checksum"], key
        assert bool(P.double) == ENVS[key]["double"] and case.kind == ENVS[key]["kind"], key


def test_no_bar_rose_and_the_table_follows_the_rule():
    tool = _tool()
    assert len(tool.OPEN) <= 3
    assert sorted(k for k, e in BARS.items() if "open" in e) == sorted(tool.OPEN)
    for key, e in BARS.items():
        test, par, prec, kind = _split(key)
        if "was_10x_measured" in e:
            assert e["bar"] <= e["was_10x_measured"], key
        if not _named(key, e):
            assert prec not in CONTRACT or e["bar"] <= CONTRACT[prec], key
            continue
        if key in tool.OPEN:
            continue
        assert e["bar"] <= max(CONTRACT[prec], helpers.ENVELOPE_FACTOR * e["legal_diameter"]) * (1 + 1e-12), key
        for p, name in _named(key, e).items():      # the bar in force: never above the table's, never below the contract, at any step
            env = ENVS[name]
            steps = [None] if kind == "x" else range(1, len(env["costs"]))
            for s in steps:
                b = helpers.bar_in_force(e, test, p, prec, kind, s, 0.0)
                assert CONTRACT[prec] <= b <= e["bar"], (key, p, s, b)


def test_the_rule_in_force_on_a_case_with_a_step_far_inside_the_table_bar():
    """shape_from_shading 123 x 4, rows 4: the legal runs spread 4.9e-9 after the first step and 3.7e-11 after the third -- the third step is held to 7.4e-11, not to 5e-9"""
    key = "tests/test_onchip_sfs_gpu.py::test_variants_double[123-4-4-4-gaussNewtonGPU]|double|cost_later"
    e = BARS[key]
    env = ENVS[e["envelope"]]
    d2, d3 = helpers.envelope_diameter(env, "cost_later", 2), helpers.envelope_diameter(env, "cost_later", 3)
    assert d3 < 0.1 * d2
    assert helpers.bar_in_force(e, key.split("[")[0], "[123-4-4-4-gaussNewtonGPU]", "double", "cost_later", 3) == pytest.approx(2 * d3, rel=1e-12)
    assert helpers.bar_in_force(e, key.split("[")[0], "[123-4-4-4-gaussNewtonGPU]", "double", "cost_later", 2) == pytest.approx(min(e["bar"], 2 * d2), rel=1e-12)
    assert e["bar"] * 4 <= e["was_10x_measured"]      # (the thin-image bars are at least 4 x tighter than 10 x measured)
    with pytest.raises(ValueError):
        helpers.bar_in_force(e, key.split("[")[0], "[123-4-4-4-gaussNewtonGPU]", "double", "cost_later", None)


def test_the_ensemble_is_the_fixed_34_runs_for_every_case():
    """... and the summaries the bars are computed from are the spreads of those runs"""
    assert FILE["meta"]["ensemble"] == LABELS and len(LABELS) == 34
    assert FILE["meta"]["host_seconds"] > 0
    assert sorted(e["row"] for e in ENVS.values()) == list(range(len(ENVS)))
    for key, env in ENVS.items():
        n = len(env["costs"])
        xd = RUNS[f"x_dist_{env['row']}"]
        assert n >= 2 and xd.shape == (34,) and xd[0] == 0.0 and env["x_diameter"] >= xd.max() * (1 - 1e-3), key
        assert ("radius" in env) == (env["kind"] == "LMGPU"), key
        for q in ("costs", "radius") if "radius" in env else ("costs",):
            v = _runs(env, q)
            assert v.shape == (34, n) and not RUNS[f"{q}_{env['row']}"][0].any(), (key, q)
            assert np.allclose(v.max(0) - v.min(0), env[q + "_spread"], rtol=1e-3, atol=0), (key, q)


def _leave_one_out(env):
    """[(quantity, step, run, distance outside the others' range, bar the others set)] for the runs that fall outside"""
    c = CONTRACT["double" if env["double"] else "float"]
    bad = []
    for q in ("costs", "radius") if "radius" in env else ("costs",):
        allv = _runs(env, q)
        for s in range(allv.shape[1]):
            vals = [float(v) for v in allv[:, s]]
            den = max(abs(vals[0]), 1e-300)
            for i, v in enumerate(vals):
                rest = vals[:i] + vals[i + 1:]
                lo, hi = min(rest), max(rest)
                out = max(lo - v, v - hi, 0.0) / den
                bar = max(c, helpers.ENVELOPE_FACTOR * (hi - lo) / den)
                if out > bar:
                    bad.append((q, s, LABELS[i], out, bar))
    xd = [float(v) for v in RUNS[f"x_dist_{env['row']}"]]
    for i in range(1, len(xd)):
        rest = max(xd[1:i] + xd[i + 1:])
        if xd[i] > max(c, helpers.ENVELOPE_FACTOR * rest):
            bad.append(("x", None, LABELS[i], xd[i], max(c, helpers.ENVELOPE_FACTOR * rest)))
    return bad


def test_leave_one_out_every_legal_run_lies_within_the_bar_of_the_other_33():
    bad = {key: b for key, env in ENVS.items() for b in [_leave_one_out(env)] if b}
    assert not bad, bad


def test_the_smallest_case_reproduces_its_frozen_exact_order_costs(oracle_lib):
    """(the smallest double case)"""
    key, case = min(((k, c) for k, c in pc.envelope_cases().items() if ENVS[k]["double"]), key=lambda kc: sum(p.size for p in kc[1].problem().params))
    env = ENVS[key]
    P = case.problem()
    o = helpers.oracle_solver(oracle_lib, P, case.kind, **case.settings())
    o.set_threads(case.threads)
    o.init(P.params)
    costs, radii = [o.cost()], [o.trust_region_radius()]
    while True:
        more = o.step(P.params)
        costs.append(o.cost()); radii.append(o.trust_region_radius())
        if not more:
            break
    o.close()
    assert len(costs) == len(env["costs"])
    for got, want in zip(costs, env["costs"]):
        assert abs(got - want) <= 1e-14 * abs(want), (key, costs, env["costs"])
    for got, want in zip(radii, env.get("radius", [])):
        assert abs(got - want) <= 1e-14 * abs(want), (key, radii, env["radius"])
