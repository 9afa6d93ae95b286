#!/usr/bin/env python3
"""Cost of the complete `eventually` check under strong fairness (CheckerBuilder.strong_fairness) next to the
weak mode's pass on the same model and the same build: SpinLock(16) and (18) "every thread served" and
FairRings(28, 64, 2, 512) (503 296 states, 29 levels) unless told otherwise.

    python scripts/liveness_strong_rate.py --repeats 3 [--resources listing.txt] [--out profiles/liveness_strong.txt]
    python scripts/liveness_strong_rate.py --models spin_lock:10 fair_rings:12,16,2,64

After one warm-up run of each mode, the modes alternate run by run so that drift hits both alike. Per
`eventually` property the pass ran for, min-max of: pass_ms of the whole pass in either mode, the part the
mode adds (its own pass_ms), its levels (strong), its rounds (component search, rank fixpoints), and entries
per second: the states of N_p over that part's time. No target is set; the file records what the mode costs.
The output (stdout, and --out if given) is stamped with the source digest; --resources names a text file
(the kernel resource listing of scripts/kernel_resources.sh, before and after) that is put in front of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--models", nargs="+", default=["spin_lock:16", "spin_lock:18", "fair_rings:28,64,2,512"])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--resources", default=None)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, ROOT)

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd import models as M  # noqa: E402

LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def make(spec):
    """(model, capacity hint, the properties to report: None = every one the pass ran for)."""
    kind, _, args = spec.partition(":")
    args = [int(x) for x in args.split(",")]
    if kind == "spin_lock":
        return M.SpinLockSys(*args), (args[0] + 1) << (args[0] + 1), ["every thread served"]
    if kind == "fair_rings":
        d, w, _, lanes = args
        return M.FairRings(*args), lanes + sum((2 + j % d) * w for j in range(lanes)), None
    raise SystemExit(f"unknown model {kind}")


def run(model, mode, hint):
    b = model.checker()
    b = b.strong_fairness() if mode == "strong" else b.weak_fairness()
    c = b.capacity_hint(hint).spawn_bfs().join()
    out = {"unique": c.unique_state_count(), "props": {}}
    for name, exp in c.properties():
        r = c.liveness(name) if exp == sr.Expectation.Eventually else {"ran": 0}
        if r["ran"]:
            out["props"][name] = r
    return out


def span(xs, fmt="{:.2f}"):
    return fmt.format(min(xs)) + "-" + fmt.format(max(xs))


def main():
    say("The complete `eventually` check under strong fairness (sr_opts.liveness = 4, `strong_fairness()`): what the")
    say(f"mode costs next to the weak mode's pass of the same build. Source digest of this tree: {N.build_digest()}.")
    say()
    if ARGS.resources:
        with open(ARGS.resources) as f:
            for line in f.read().rstrip("\n").split("\n"):
                say(line)
        say()
    say("Cost of the pass (scripts/liveness_strong_rate.py; one MI355X; min-max over the runs; no target is set)")
    say("-" * 100)
    modes = ["weak", "strong"]
    for spec in ARGS.models:
        model, hint, names = make(spec)
        runs = {m: [] for m in modes}
        for m in modes:
            run(model, m, hint)
        for _ in range(ARGS.repeats):
            for m in modes:
                runs[m].append(run(model, m, hint))
        first = runs["strong"][0]
        say(f"{spec}: unique {first['unique']}, {ARGS.repeats} runs each")
        out = {"model": spec, "unique": first["unique"], "repeats": ARGS.repeats, "digest": N.build_digest(), "props": {}}
        for name in (names or list(first["props"])):
            rec = {}
            for m in modes:
                rs = [x["props"][name] for x in runs[m] if name in x["props"]]
                if not rs:
                    continue
                part = [r[m] for r in rs]
                eps = [rs[0]["not_p_states"] / (p["pass_ms"] * 1e-3) for p in part]
                p0 = part[0]
                levels = f"levels {p0['levels']}; " if m == "strong" else ""
                say(f"  {m:6s} \"{name}\": whole pass_ms {span([r['pass_ms'] for r in rs])}; the mode's part: pass_ms {span([p['pass_ms'] for p in part])}; "
                    f"{levels}scc_rounds {span([p['scc_rounds'] for p in part], '{}')}; reach_rounds {span([p['reach_rounds'] for p in part], '{}')}; "
                    f"entries/s {span(eps, '{:.3e}')}")
                say(f"         |N_p| {rs[0]['not_p_states']}, |F_p'| {rs[0]['surviving']}, cyclic {p0['cyclic_states']}, components {p0['components']} "
                    f"({p0['fair_components']} fair), goal {p0['goal_states']}, FairF {p0['fair_states']}, init {rs[0]['init_index']}, "
                    f"stem {p0['stem_len']}, loop {p0['loop_len']}, segments {p0['segments']}")
                rec[m] = {"pass_ms": [r["pass_ms"] for r in rs], "part_pass_ms": [p["pass_ms"] for p in part],
                          "scc_rounds": [p["scc_rounds"] for p in part], "reach_rounds": [p["reach_rounds"] for p in part],
                          "entries_per_s": eps, "levels": p0.get("levels"), "components": p0["components"],
                          "fair_components": p0["fair_components"], "init_index": rs[0]["init_index"]}
            out["props"][name] = rec
        say(json.dumps(out))
    if ARGS.out:
        with open(os.path.join(ROOT, ARGS.out) if not os.path.isabs(ARGS.out) else ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
