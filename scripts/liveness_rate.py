#!/usr/bin/env python3
"""Cost of the complete `eventually` check (CheckerBuilder.complete_liveness) for one model.

    python scripts/liveness_rate.py live_graph 24 2 1 2 0 1 --repeats 5
    python scripts/liveness_rate.py pingpong 10 1 1 --repeats 5        (max_nat, lossy, duplicating)
    python scripts/liveness_rate.py 2pc_live 9 --fairness progress --repeats 5        (rm_count)

Runs the check `repeats` times without the option and `repeats` times with it, alternating run by run
so that drift hits both alike (after one warm-up run of each), and prints min-max of: the search's
time without the option and with it (stats()["level_loop_sec"]: the pass is not part of it), and per
`eventually` property the pass ran for its pass_ms, rounds, worklist entries examined and entries
per second, next to the search's own expanded parents per second (unique states / level_loop_sec).
One JSON line at the end. --order fast runs the search in FAST order (the default for a model with
`eventually` properties is the reference's FIFO order). --fairness progress runs the pass under progress
fairness (complete_liveness(fairness="progress")): a successor equal to its state is no successor."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import LiveGraph, TwoPhaseLiveSys  # noqa: E402

MODELS = {
    "live_graph": lambda a: LiveGraph(*a),  # (n_bits, degree, seed, p_mod, t_mod, roots[, words])
    "pingpong": lambda a: sr.PingPong(a[0], lossy=bool(a[1]), duplicating=bool(a[2])),
    "2pc_live": lambda a: TwoPhaseLiveSys(a[0]),  # (rm_count)
}


def run(model, on, order, hint, fairness=None):
    b = model.checker().complete_liveness(on, fairness=fairness).order(order)
    if hint:
        b = b.capacity_hint(hint)
    c = b.spawn_bfs().join()
    st = c.stats()
    out = {"unique": c.unique_state_count(), "loop_sec": st["level_loop_sec"], "total_sec": st["total_sec"], "props": {}}
    for name, exp in c.properties():
        r = c.liveness(name) if exp == sr.Expectation.Eventually else {"ran": 0}
        if r["ran"]:
            out["props"][name] = r
    return out


def span(xs, fmt="{:.3f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=sorted(MODELS))
    ap.add_argument("args", type=int, nargs="+")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--order", default="auto", choices=["auto", "fifo", "fast"])
    ap.add_argument("--hint", type=int, default=0, help="capacity_hint (0: none)")
    ap.add_argument("--fairness", default="none", choices=["none", "progress"])
    a = ap.parse_args()
    fairness = None if a.fairness == "none" else a.fairness
    model = MODELS[a.model](a.args)
    for on in (False, True):
        run(model, on, a.order, a.hint, fairness)
    off, on = [], []
    for _ in range(a.repeats):
        off.append(run(model, False, a.order, a.hint))
        on.append(run(model, True, a.order, a.hint, fairness))
    unique = on[0]["unique"]
    rate = [x["unique"] / x["loop_sec"] for x in off]
    print(f"{a.model} {a.args} order={a.order} hint={a.hint} fairness={a.fairness}: unique {unique}, {a.repeats} runs each, min-max")
    print(f"  search, option off: level_loop {span([x['loop_sec'] * 1e3 for x in off])} ms; "
          f"expanded parents/s {span(rate, '{:.3e}')}")
    print(f"  search, option on:  level_loop {span([x['loop_sec'] * 1e3 for x in on])} ms")
    out = {"model": a.model, "args": a.args, "order": a.order, "hint": a.hint, "fairness": a.fairness, "unique": unique, "repeats": a.repeats,
           "digest": N.build_digest(), "off_loop_ms": [x["loop_sec"] * 1e3 for x in off],
           "on_loop_ms": [x["loop_sec"] * 1e3 for x in on], "props": {}}
    for name in on[0]["props"]:
        rs = [x["props"][name] for x in on]
        eps = [r["examined"] / (r["pass_ms"] * 1e-3) for r in rs]
        r0 = rs[0]
        print(f"  pass \"{name}\": pass_ms {span([r['pass_ms'] for r in rs])}; rounds {span([r['rounds'] for r in rs], '{}')}; "
              f"examined {span([r['examined'] for r in rs], '{}')}; "
              f"entries/s {span(eps, '{:.3e}')}; |N| {r0['not_p_states']}, |F| {r0['surviving']}, witness {r0['witness_len']} "
              f"steps, loop_start {r0['loop_start']}, end_kind {r0['end_kind']}; entries/s over parents/s {min(eps) / max(rate):.2f}-{max(eps) / min(rate):.2f}")
        out["props"][name] = {"pass_ms": [r["pass_ms"] for r in rs], "rounds": [r["rounds"] for r in rs], "examined": [r["examined"] for r in rs],
                              "entries_per_s": eps, "not_p_states": r0["not_p_states"], "surviving": r0["surviving"],
                              "witness_len": r0["witness_len"], "loop_start": r0["loop_start"], "end_kind": r0["end_kind"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
