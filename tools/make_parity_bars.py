#!/usr/bin/env python
"""tests/golden/parity_bars.json from a logged GPU run of the parity tests ("assert 1e-12 where the measured error allows ... per case, with the
reason -- not a blanket 1e-10 / 1e-8").

    OPT_PARITY_LOG=$PWD/parity_log.jsonl python -m pytest tests -m gpu        (on the GPU box; tests/helpers.py assert_close appends one line per check)
    python tools/make_parity_bars.py [--files tests/test_a.py,...] parity_log.jsonl [more logs ...]         (no log: re-derives the table in place from the envelopes)

--files keeps only the checks of the named test files.  The table in the tree was made that way from the nine files whose entries sat above the contract (NINE below): a log
of the whole suite stops this tool today, on parametrisations of test files that were added after the table was last built and still run at their call sites' defaults
(test_lm_outer_controls_gpu.py, test_graph_fused_gpu.py, test_graph_shapes_gpu.py, ...) -- they need cases in tests/parity_cases.py and envelopes first.

Rule, per test FUNCTION, precision and quantity (cost0 = before any step, cost = after the first outer step or every step, cost_later = later outer steps, radius, x):
  double   bar = 1e-12 (the contract) for every parametrisation whose measured error is <= 1e-13; a parametrisation above that gets its OWN entry;
  float    costs keep the contract 1e-5 (or the measured envelope of legal oracle runs, tests/golden/float_envelopes.json) that the call site passes; only the quantities
           whose call-site default is looser than the contract (later outer steps, the LM radius: 1e-3) get an entry.
An entry above the contract is never derived from the error the library itself produced.  It names the frozen ensemble of legal oracle runs of the same case
(tests/golden/parity_envelopes.json, tests/golden/make_parity_envelopes.py; the case is tests/parity_cases.py::ENTRY_CASES') and its bar is
      max(contract, 2 x the largest diameter of the legal runs over the steps the check covers)
-- tests/helpers.py::assert_close applies the same rule step by step, so the bar in force is never above this one.  A parametrisation above the contract whose case is not in
ENTRY_CASES stops this tool: add the case, regenerate the envelopes, run again.  Regenerating never raises a bar: every entry is clamped to min(previous, new); the value an
entry had when it was 10 x the library's own error stays in `was_10x_measured`.  Entries in OPEN keep their previous bar: the library's error sits outside the legal spread
there and the cause is not found yet (profiles/parity_evidence.md has the trace comparison); tests/test_parity_envelopes_cpu.py holds the list to at most three.
"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "parity_bars.json")
CONTRACT = {"double": 1e-12, "float": 1e-5}
NINE = ["tests/test_onchip_stencil_gpu.py", "tests/test_onchip_sfs_gpu.py", "tests/test_stencil_march_gpu.py", "tests/test_energies_gpu.py", "tests/test_image_warping_gpu.py",
        "tests/test_lm_controls_gpu.py", "tests/test_onchip_gpu.py", "tests/test_onchip_lm_gpu.py", "tests/test_reference_order_mode_gpu.py"]
OPEN = []      # keys of parity_bars.json that keep the bar they had: at most three
WHY = {      # what the frozen legal runs show about a parametrisation above the contract (per test function; '*' = any)
    "test_intrinsic_double": "intrinsic_image_decomposition, ill-conditioned and unpreconditioned: sum order and fma alone spread the legal runs this far (no pow difference needed)",
    "test_trajectory": "4 x 12 PCG iterations amplify last-bit differences of the sums; intrinsic: sum order and fma alone spread the legal runs this far",
    "test_variants_double": "thin images under an undamped Gauss-Newton step: the oracle's own legal roundings diverge this far; the damped LM step holds 1e-12",
    "test_many_steps_tag_counter_runs_on": "9 outer steps: rounding differences of the sums compound from step to step, among the oracle's legal runs as well",
    "*": "PCG iterations amplify last-bit differences of the sums; the oracle's legal runs spread this far",
}


def steps_by_convention(kind, nrec, splits_later):
    """the steps a check covers when no log says so: costs[0] is the cost before any step; tests that split 'cost' / 'cost_later' check 'cost' after the first step only"""
    if kind == "x":
        return [None]
    if kind == "cost_later":
        return list(range(2, nrec))
    if kind == "cost" and splits_later:
        return [1]
    return list(range(1, nrec))


def main():
    import helpers
    import parity_cases as pc
    envs = helpers.envelopes()
    prev = json.load(open(OUT)) if os.path.exists(OUT) else {}
    rows = []
    args = sys.argv[1:]
    files = None
    if "--files" in args:      # --files tests/test_a.py,tests/test_b.py: only the checks of these test files
        i = args.index("--files")
        files = set(args[i + 1].split(",")); del args[i:i + 2]
    for p in args:
        rows += [r for r in (json.loads(l) for l in open(p)) if files is None or r["test"].split("::")[0] in files]
    per = collections.defaultdict(lambda: collections.defaultdict(float))      # (test, prec, kind) -> params -> max err
    checks = collections.defaultdict(set)                                      # (test, params, prec, kind) -> {(step, floor)}
    dflt = {}
    for r in rows:
        k = (r["test"], r["prec"], r["kind"])
        per[k][r["params"]] = max(per[k][r["params"]], r["err"])
        dflt[k] = max(dflt.get(k, 0.0), r["default"] or 0.0)      # (None: a call site that relies on its entry)
        checks[(r["test"], r["params"], r["prec"], r["kind"])].add((r.get("step"), r.get("floor", 0.0)))
    later = {k.split("|")[0].split("[")[0] + "|" + k.split("|")[1] for k in list(prev) if k.endswith("|cost_later")} | {f"{t}|{p}" for (t, p, kd) in per if kd == "cost_later"}
    missing = []

    def diameter(test, par, prec, kind):
        """(envelope key, largest diameter over the steps the check covers) or None if the case is not registered"""
        case = pc.ENTRY_CASES.get(test + par)
        if case is None or case.key not in envs:
            missing.append(test + par)
            return None
        env = envs[case.key]
        logged = checks.get((test, par, prec, kind))
        if logged and (kind == "x" or all(s is not None for s, _ in logged)):
            cover = sorted(logged, key=str)
        elif logged:      # (a log from before the call site passed its step: every step, over the floor it logged)
            cover = [(s, max(f for _, f in logged)) for s in steps_by_convention(kind, len(env["costs"]), False)]
        else:
            floor = 0.0      # (no log: the denominator without the call site's floor -- never smaller than with it)
            cover = [(s, floor) for s in steps_by_convention(kind, len(env["costs"]), f"{test}|{prec}" in later)]
        return case.key, max(helpers.envelope_diameter(env, kind, s, f) for s, f in cover)

    def envelope_entry(key, test, pars, prec, kind, base, single):
        """an entry above the contract: bar = max(contract, 2 x diameter) over its parametrisations, clamped to what it was"""
        c = CONTRACT[prec]
        got = {par: diameter(test, par, prec, kind) for par in pars}
        if any(v is None for v in got.values()):
            return None
        dmax = max(v[1] for v in got.values())
        old = prev.get(key, {})
        was = old.get("was_10x_measured", None if ("envelope" in old or "envelopes" in old) else old.get("bar"))      # (None: an entry that never was 10 x measured)
        e = dict(base)
        e["bar"] = max(c, helpers.ENVELOPE_FACTOR * dmax)
        if was is not None:
            e["bar"] = min(e["bar"], old["bar"]); e["was_10x_measured"] = was
        elif "was" in base:
            e["bar"] = min(e["bar"], base["was"], old.get("bar", base["was"]))      # a new entry: never above the default its call site passes
        e["legal_diameter"] = dmax
        if single:
            e["envelope"] = got[pars[0]][0]
        else:
            e["envelopes"] = "ENTRY_CASES"      # (one envelope per case: tests/parity_cases.py::ENTRY_CASES names it for each parametrisation)
        fn = test.split("::")[-1]
        e["why"] = (WHY.get(fn, WHY["*"]) if prec == "double" else "float later steps / LM radius: max(contract, 2 x the spread of the legal oracle runs of each case)")
        return e

    bars = {}
    for (test, prec, kind), byp in sorted(per.items()):
        if prec not in CONTRACT:
            continue
        c = CONTRACT[prec]
        if prec == "float":
            if dflt[(test, prec, kind)] <= 1e-5 or kind in ("cost0", "cost") or (kind == "x"):
                continue      # the call site's bar already is the contract (or a measured envelope)
            key = f"{test}|{prec}|{kind}"
            m = max(byp.values())
            base = {"measured_max": m, "cases": len(byp), "was": dflt[(test, prec, kind)]}
            if m <= 0.1 * c and not all((test + p) in pc.ENTRY_CASES for p in byp):      # (a function whose cases all have envelopes keeps that yardstick, however small its error is today)
                bars[key] = dict(base, bar=c, why="float: later outer steps / the LM radius meet the 1e-5 contract with a factor 10 to spare")
            else:
                e = envelope_entry(key, test, sorted(byp), prec, kind, base, False)
                if e:
                    bars[key] = e
            continue
        ok = {p: e for p, e in byp.items() if e <= 0.1 * c}
        out = {p: e for p, e in byp.items() if e > 0.1 * c}
        if ok or not out:
            bars[f"{test}|{prec}|{kind}"] = {"bar": c, "measured_max": max(ok.values()) if ok else 0.0, "cases": len(ok), "was": dflt[(test, prec, kind)], "why": "meets the 1e-12 contract with a factor 10 to spare"}
        for p, err in sorted(out.items()):
            key = f"{test}{p}|{prec}|{kind}"
            base = {"measured": err, "was": dflt[(test, prec, kind)]}
            if (test + p) not in pc.ENTRY_CASES and err <= c:
                bars[key] = dict(base, bar=c, why="meets the 1e-12 contract (measured within a factor 10 of it)")
                continue
            e = envelope_entry(key, test, [p], prec, kind, base, True)
            if e:
                bars[key] = e
    # entries the logs did not touch are carried over; one above the contract that names no envelope yet is re-derived from its envelope
    for key, old in sorted(prev.items()):
        if key in bars:
            bars[key]["bar"] = min(bars[key]["bar"], old["bar"])      # regenerating never raises a bar
            if "envelope" not in bars[key] and "envelopes" not in bars[key] and bars[key]["bar"] == old["bar"]:
                bars[key] = old      # (an entry at the contract that stays there: keep the run it was frozen from)
            continue
        tp, prec, kind = key.split("|")
        if prec not in CONTRACT or old["bar"] <= CONTRACT[prec] or "envelope" in old or "envelopes" in old:
            bars[key] = old
            continue
        test, _, par = tp.partition("[")
        par = ("[" + par) if par else ""
        pars = [par] if par or (test in pc.ENTRY_CASES) else sorted(k[len(test):] for k in pc.ENTRY_CASES if k.startswith(test + "["))
        e = envelope_entry(key, test, pars, prec, kind, {k: v for k, v in old.items() if k not in ("bar", "why")}, bool(par) or test in pc.ENTRY_CASES)
        if e:
            bars[key] = e
    for key in OPEN:
        old = prev[key]
        bars[key] = dict(old, bar=old.get("was_10x_measured", old["bar"]), open="the library's error is outside the legal spread; cause not found (profiles/parity_evidence.md)")
    if missing:
        sys.exit("above the contract without a frozen envelope (add the case to tests/parity_cases.py::ENTRY_CASES, run tests/golden/make_parity_envelopes.py):\n  " + "\n  ".join(sorted(set(missing))))
    json.dump(bars, open(OUT, "w"), indent=0, sort_keys=True)
    n12 = sum(1 for k, v in bars.items() if "|double|" in k and v["bar"] <= 1e-12)
    above = {k: v for k, v in bars.items() if v["bar"] > CONTRACT.get(k.split("|")[1], 1.0)}
    print(f"{len(bars)} entries; double entries at the 1e-12 contract: {n12}; above the contract (all with an envelope): {len(above)}; open: {len(OPEN)}")
    for k, v in sorted(above.items(), key=lambda kv: -kv[1]["bar"]):
        print(f"   {v['bar']:.1e}  (was {v.get('was_10x_measured', v['bar']):.0e})  {k}")


if __name__ == "__main__":
    main()
