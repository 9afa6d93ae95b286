#!/usr/bin/env python3
"""Cost of the complete `eventually` check under weak fairness (CheckerBuilder.weak_fairness) next to the
progress mode of the same build, on LiveGraph(24, 2, 1, 3, 0, 1) and SpinLock(18) unless told otherwise.

    python scripts/liveness_weak_rate.py --repeats 5
    python scripts/liveness_weak_rate.py --mode progress --repeats 5       (runs on a tree without the weak mode too)
    python scripts/liveness_weak_rate.py --models spin_lock:10 live_graph:16,3,26,2,0,1

After one warm-up run of each mode, the modes alternate run by run so that drift hits both alike. Per
`eventually` property the pass ran for, min-max of: pass_ms of the whole pass in either mode, and in the
weak mode the part the mode adds (weak pass_ms), its rounds (component search, rank fixpoints), segments,
and entries per second: the states of N_p over the weak part's time (every kernel of the weak part runs
over a list of states of N_p, one entry per state). One JSON line per model at the end. To compare with
another commit, run this file with `--mode progress --root <that tree>`: it then imports the package
of that tree, whose progress mode is timed on the same graphs."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--models", nargs="+", default=["live_graph:24,2,1,3,0,1", "spin_lock:18"])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--mode", default="both", choices=["both", "progress"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package is measured (default: this one)")
ARGS = ap.parse_args()
sys.path.insert(0, ARGS.root)

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd import models as M  # noqa: E402


def make(spec):
    kind, _, args = spec.partition(":")
    args = [int(x) for x in args.split(",")]
    if kind == "live_graph":
        return M.LiveGraph(*args), 1 << args[0]
    if kind == "spin_lock":
        return M.SpinLockSys(*args), (args[0] + 1) << (args[0] + 1)
    raise SystemExit(f"unknown model {kind}")


def run(model, mode, hint):
    b = model.checker()
    b = b.weak_fairness() if mode == "weak" else b.complete_liveness(fairness="progress")
    c = b.capacity_hint(hint).spawn_bfs().join()
    out = {"unique": c.unique_state_count(), "loop_sec": c.stats()["level_loop_sec"], "props": {}}
    for name, exp in c.properties():
        r = c.liveness(name) if exp == sr.Expectation.Eventually else {"ran": 0}
        if r["ran"]:
            out["props"][name] = r
    return out


def span(xs, fmt="{:.2f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    modes = ["progress"] if ARGS.mode == "progress" else ["progress", "weak"]
    for spec in ARGS.models:
        model, hint = make(spec)
        runs = {m: [] for m in modes}
        for m in modes:
            run(model, m, hint)
        for _ in range(ARGS.repeats):
            for m in modes:
                runs[m].append(run(model, m, hint))
        first = runs[modes[0]][0]
        print(f"{spec}: unique {first['unique']}, {ARGS.repeats} runs each, min-max; digest {N.build_digest()}")
        out = {"model": spec, "unique": first["unique"], "repeats": ARGS.repeats, "digest": N.build_digest(), "props": {}}
        for name in first["props"]:
            rec = {}
            for m in modes:
                rs = [x["props"][name] for x in runs[m] if name in x["props"]]
                if not rs:
                    continue
                line = (f"  {m:8s} \"{name}\": pass_ms {span([r['pass_ms'] for r in rs])}; trim rounds {span([r['rounds'] for r in rs], '{}')}; "
                        f"|N| {rs[0]['not_p_states']}, |F'| {rs[0]['surviving']}, witness {rs[0]['witness_len']} steps, end_kind {rs[0]['end_kind']}")
                rec[m] = {"pass_ms": [r["pass_ms"] for r in rs], "rounds": [r["rounds"] for r in rs], "surviving": rs[0]["surviving"],
                          "witness_len": rs[0]["witness_len"], "end_kind": rs[0]["end_kind"]}
                if m == "weak":
                    ws = [r["weak"] for r in rs]
                    eps = [rs[0]["not_p_states"] / (w["pass_ms"] * 1e-3) for w in ws]
                    w0 = ws[0]
                    line += (f"\n           weak part: pass_ms {span([w['pass_ms'] for w in ws])}; scc_rounds {span([w['scc_rounds'] for w in ws], '{}')}; "
                             f"reach_rounds {span([w['reach_rounds'] for w in ws], '{}')}; segments {w0['segments']}; entries/s {span(eps, '{:.3e}')}; "
                             f"cyclic {w0['cyclic_states']}, components {w0['components']} ({w0['fair_components']} fair), goal {w0['goal_states']}, "
                             f"FairF {w0['fair_states']}, stem {w0['stem_len']}, loop {w0['loop_len']}")
                    rec[m].update({"weak_pass_ms": [w["pass_ms"] for w in ws], "scc_rounds": [w["scc_rounds"] for w in ws],
                                   "reach_rounds": [w["reach_rounds"] for w in ws], "segments": w0["segments"], "entries_per_s": eps,
                                   **{k: w0[k] for k in ("cyclic_states", "components", "fair_components", "goal_states", "fair_states",
                                                         "stem_len", "loop_len")}})
                print(line)
            out["props"][name] = rec
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
