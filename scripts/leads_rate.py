#!/usr/bin/env python3
"""Cost of the leads-to check for one LeadsGraph.

    python scripts/leads_rate.py 24 2 1 2 0 1 7 --hint 16777216 --repeats 5
    python scripts/leads_rate.py 24 2 1 2 0 1 7 --hint 16777216 --fairness weak --repeats 5

Runs the check `repeats` times in the given mode (after one warm-up run) and prints min-max of: the search's
time (stats()["level_loop_sec"]: the pass is not part of it); per property the pass ran for its pass_ms; and
per leads-to property its seed_ms (the seed stage: the scan over the arena with its read-back, and, where a
state violates, the tie-break launches over the seed's level with theirs), the three counts and the seed's
depth. Next to them, from alternating runs of the same process: the pass_ms of `eventually "marked"` on the
same graph with p_mod = 1, where the condition holds everywhere, N_p is empty and the pass is live_mark over
the arena plus its read-backs and nothing else: the yardstick for a stage that reads what live_mark reads
and does not probe. One JSON line at the end."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import LeadsGraph  # noqa: E402


def builder(model, fairness):
    b = model.checker()
    if fairness == "weak":
        return b.weak_fairness()
    if fairness == "strong":
        return b.strong_fairness()
    return b.complete_liveness(fairness=None if fairness == "none" else fairness)


def run(model, fairness, order, hint):
    b = builder(model, fairness).order(order)
    if hint:
        b = b.capacity_hint(hint)
    c = b.spawn_bfs().join()
    st = c.stats()
    out = {"unique": c.unique_state_count(), "loop_sec": st["level_loop_sec"], "props": {}}
    for name, _ in c.properties():
        r = c.liveness(name)
        if r["ran"]:
            out["props"][name] = r
    return out


def span(xs, fmt="{:.3f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("args", type=int, nargs="+", help="n_bits degree seed p_mod t_mod roots q_mod [words [dup]]")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--order", default="auto", choices=["auto", "fifo", "fast"])
    ap.add_argument("--hint", type=int, default=0, help="capacity_hint (0: none)")
    ap.add_argument("--fairness", default="none", choices=["none", "progress", "weak", "strong"])
    a = ap.parse_args()
    model = LeadsGraph(*a.args)
    mark_only = LeadsGraph(*(a.args[:3] + [1] + a.args[4:6] + [0] + a.args[7:]))  # p_mod = 1: N_p is empty; q_mod = 0
    run(model, a.fairness, a.order, a.hint)
    run(mark_only, a.fairness, a.order, a.hint)
    runs, marks = [], []
    for _ in range(a.repeats):
        runs.append(run(model, a.fairness, a.order, a.hint))
        marks.append(run(mark_only, a.fairness, a.order, a.hint))
    unique = runs[0]["unique"]
    mark_ms = [x["props"]["marked"]["pass_ms"] for x in marks]
    print(f"leads_graph {a.args} order={a.order} hint={a.hint} fairness={a.fairness}: unique {unique}, {a.repeats} runs, min-max")
    print(f"  search: level_loop {span([x['loop_sec'] * 1e3 for x in runs])} ms")
    print(f"  live_mark alone (`marked` with p_mod = 1: |N| = {marks[0]['props']['marked']['not_p_states']}): pass_ms {span(mark_ms)}")
    out = {"args": a.args, "order": a.order, "hint": a.hint, "fairness": a.fairness, "unique": unique, "repeats": a.repeats,
           "digest": N.build_digest(), "loop_ms": [x["loop_sec"] * 1e3 for x in runs], "mark_only_pass_ms": mark_ms, "props": {}}
    for name in runs[0]["props"]:
        rs = [x["props"][name] for x in runs]
        r0 = rs[0]
        line = f"  pass \"{name}\": pass_ms {span([r['pass_ms'] for r in rs])}; |N| {r0['not_p_states']}, |F| {r0['surviving']}, witness {r0['witness_len']} steps"
        rec = {"pass_ms": [r["pass_ms"] for r in rs], "not_p_states": r0["not_p_states"], "surviving": r0["surviving"], "witness_len": r0["witness_len"]}
        if "leads" in r0:
            ld = r0["leads"]
            seed = [r["leads"]["seed_ms"] for r in rs]
            line += (f"; seed_ms {span(seed)} ({min(seed) / max(mark_ms):.2f}-{max(seed) / min(mark_ms):.2f} of live_mark alone); triggered "
                     f"{ld['triggered']}, pending {ld['pending']}, violating {ld['violating']}, depth {ld['trigger_depth']}")
            rec.update(seed_ms=seed, triggered=ld["triggered"], pending=ld["pending"], violating=ld["violating"], trigger_depth=ld["trigger_depth"])
        print(line)
        out["props"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
