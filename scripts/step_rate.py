#!/usr/bin/env python3
"""Cost of the step pass beside the coverage pass on the same checks.

    python scripts/step_rate.py
    python scripts/step_rate.py --repeats 5 --out profiles/step_pass.txt

Per check: one warm-up run, then `repeats` runs with the coverage pass on, so that both passes follow the same
search. Prints, min-max: the search's own time (stats()["level_loop_sec"]: neither pass is part of it), the
coverage pass' pass_ms, the step pass' scan_ms (the counting launch and its read-back, shared by the model's
step properties) and min_ms (per property with a violation: the tie-break launches, the tree path and the
acceptance on the host), the step pass' total (scan_ms + every property's min_ms), and both passes over the same
run's level_loop. One JSON line per check. The checks run in FAST order with the capacity hint of the known
state count."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import StepGraph  # noqa: E402

GRAPH = (24, 2, 1, 1000, 0, 1)  # about 13.4 M of the 2^24 nodes are reachable

# (name, model, unique states: the capacity hint, 0: read off the warm-up run)
CHECKS = [
    ("2pc-step N=9", lambda: sr.TwoPhaseStepSys(9), 6 ** 9 + 4 ** 9 + 2 ** 9),
    ("step graph 24 bits, 1 word", lambda: StepGraph(*GRAPH), 0),
    ("step graph 24 bits, 4 words", lambda: StepGraph(*GRAPH, words=4), 0),
    # the control: with f_mod = 0 the first hook returns before its 64-bit modulo (the graph is the same)
    ("step graph 24 bits, 1 word, f_mod 0", lambda: StepGraph(*GRAPH[:3], 0, *GRAPH[4:]), 0),
]


def run(model, hint):
    b = model.checker().coverage().order("fast")
    if hint:
        b = b.capacity_hint(hint)
    c = b.spawn_bfs().join()
    st = c.stats()
    cov = c.coverage()
    steps = {name: c.step(name) for name, exp in c.properties() if exp == sr.Expectation.AlwaysStep}
    first = next(iter(steps.values()))
    assert first["edges"] == sum(k["taken"] for k in cov["classes"])
    return {"unique": c.unique_state_count(), "loop_ms": st["level_loop_sec"] * 1e3, "cover_ms": cov["pass_ms"],
            "edges": first["edges"], "scan_ms": first["scan_ms"], "min_ms": {n: s["min_ms"] for n, s in steps.items()},
            "violations": {n: s["violations"] for n, s in steps.items()},
            "step_index": {n: s["step_index"] for n, s in steps.items()}}


def span(xs, fmt="{:.3f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="run only the checks whose name contains this")
    ap.add_argument("--out", default="", help="append the lines to this file too")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name, make, hint in CHECKS:
        if a.only and a.only not in name:
            continue
        model = make()
        hint = hint or run(model, 0)["unique"]
        run(model, hint)
        runs = [run(model, hint) for _ in range(a.repeats)]
        total = [r["scan_ms"] + sum(r["min_ms"].values()) for r in runs]
        emit(f"{name}: unique {runs[0]['unique']}, edges {runs[0]['edges']}, {a.repeats} runs, min-max")
        emit(f"  search: level_loop {span([r['loop_ms'] for r in runs])} ms")
        emit(f"  coverage pass: pass_ms {span([r['cover_ms'] for r in runs])}; over the same run's level_loop "
             f"{span([r['cover_ms'] / r['loop_ms'] for r in runs], '{:.2f}')}")
        emit(f"  step pass: scan_ms {span([r['scan_ms'] for r in runs])}; total {span(total)}; over the same run's level_loop "
             f"{span([t / r['loop_ms'] for t, r in zip(total, runs)], '{:.2f}')}; over the same run's coverage pass "
             f"{span([t / r['cover_ms'] for t, r in zip(total, runs)], '{:.2f}')}")
        for prop in runs[0]["min_ms"]:
            emit(f"    \"{prop}\": violations {runs[0]['violations'][prop]}, step_index {runs[0]['step_index'][prop]}, "
                 f"min_ms {span([r['min_ms'][prop] for r in runs])}")
        emit(json.dumps({"check": name, "unique": runs[0]["unique"], "repeats": a.repeats, "digest": N.build_digest(),
                         "loop_ms": [r["loop_ms"] for r in runs], "cover_ms": [r["cover_ms"] for r in runs],
                         "scan_ms": [r["scan_ms"] for r in runs], "min_ms": [r["min_ms"] for r in runs]}))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
