#!/usr/bin/env python3
"""Cost of the coverage pass (CheckerBuilder.coverage).

    python scripts/coverage_rate.py                       (2pc N=9, paxos C=3)
    python scripts/coverage_rate.py --inclock 11          (increment_lock N=11 as well)
    python scripts/coverage_rate.py --out profiles/coverage_pass.txt

Per check: one warm-up run each way, then `repeats` runs without the option and `repeats` with it,
alternating run by run so that drift hits both alike. Prints, min-max: the search's own time without
the option and with it (stats()["level_loop_sec"]: the pass is not part of it), the pass' pass_ms, and
the ratio of each run's pass_ms to that same run's level_loop. One JSON line per check. The checks run
as bench.py runs them (FAST order, the capacity hint of the known state count)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402


def inclock_states(t):
    return 1 + 4 * sum(math.factorial(t) // math.factorial(t - k) for k in range(1, t + 1))


# (name, model, unique states: the capacity hint; bench.py's figures)
CHECKS = [
    ("2pc N=9", lambda: sr.TwoPhaseSys(9), 6 ** 9 + 4 ** 9 + 2 ** 9),
    ("paxos C=3", lambda: sr.Paxos(3), 1_194_428),
]
INCLOCK = {n: inclock_states(n) for n in (9, 10, 11)}


def run(model, on, hint):
    b = model.checker().coverage(on).order("fast")
    if hint:
        b = b.capacity_hint(hint)
    c = b.spawn_bfs().join()
    st = c.stats()
    out = {"unique": c.unique_state_count(), "loop_ms": st["level_loop_sec"] * 1e3, "total_ms": st["total_sec"] * 1e3}
    if on:
        cov = c.coverage()
        assert cov["states"] == out["unique"]
        out["pass_ms"] = cov["pass_ms"]
        out["taken"] = sum(k["taken"] for k in cov["classes"])
    return out


def span(xs, fmt="{:.3f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inclock", type=int, default=0, choices=[0] + sorted(INCLOCK), help="also increment_lock of this many threads")
    ap.add_argument("--only", default="", help="run only the checks whose name contains this")
    ap.add_argument("--aa", action="store_true", help="both arms run with the option off: what alternation alone does "
                                                      "to the second arm's level_loop")
    ap.add_argument("--out", default="", help="append the lines to this file too")
    a = ap.parse_args()
    checks = list(CHECKS)
    if a.inclock:
        n = a.inclock
        checks.append((f"increment_lock N={n}", lambda: sr.IncrementLock(n), INCLOCK[n]))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name, make, hint in checks:
        if a.only and a.only not in name:
            continue
        model = make()
        for on in (False, not a.aa):
            run(model, on, hint)
        off, on = [], []
        for _ in range(a.repeats):
            off.append(run(model, False, hint))
            on.append(run(model, not a.aa, hint))
        if a.aa:
            emit(f"{name}: both arms with the option off, {a.repeats} runs each, alternating, min-max")
            emit(f"  first arm:  level_loop {span([x['loop_ms'] for x in off])} ms")
            emit(f"  second arm: level_loop {span([x['loop_ms'] for x in on])} ms")
            continue
        if on[0]["unique"] != hint:
            hint_note = f" (hint {hint})"
        else:
            hint_note = ""
        ratio = [x["pass_ms"] / x["loop_ms"] for x in on]
        emit(f"{name}: unique {on[0]['unique']}{hint_note}, successors {on[0]['taken']}, {a.repeats} runs each way, min-max")
        emit(f"  search, option off: level_loop {span([x['loop_ms'] for x in off])} ms")
        emit(f"  search, option on:  level_loop {span([x['loop_ms'] for x in on])} ms")
        emit(f"  pass: pass_ms {span([x['pass_ms'] for x in on])}; pass_ms over the same run's level_loop {span(ratio, '{:.2f}')}; "
             f"states/s {span([x['unique'] / (x['pass_ms'] * 1e-3) for x in on], '{:.3e}')}")
        emit(json.dumps({"check": name, "unique": on[0]["unique"], "repeats": a.repeats, "digest": N.build_digest(),
                         "off_loop_ms": [x["loop_ms"] for x in off], "on_loop_ms": [x["loop_ms"] for x in on],
                         "pass_ms": [x["pass_ms"] for x in on], "ratio": ratio}))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
