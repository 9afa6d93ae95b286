#!/usr/bin/env python3
"""Walk rate of the simulation checker (CheckerBuilder.spawn_simulation) for one model.

    python scripts/sim_rate.py 2pc 9 --walks 11000000 --max-depth 256 --repeats 5 --grids 0 256

Runs the check `repeats` times per form of the kernel (SR_SIM_REFILL=0 static, 1 persistent; the
persistent form once per grid cap of --grids: it refills only when a batch has more walks than its
grid has lanes), the forms alternating run by run so that drift hits all alike, and prints per form the median and the
range of steps/s and walks/s (steps = stats()["successors"], time = stats()["level_loop_sec"]: the
batch loop, launches and the per-batch counter read-back included). As context it prints the host's
single-thread rate of the same walks (sr_sim_walk over 10 000 walks). One JSON line at the end.

--loops measures every form twice, without and with loop detection (detect_loops=True, rows named
"<form>+loops"), all of them alternating in the same way: the cost of the mode is the ratio of a
form's two rows (profiles/sim_loop_rate.txt). With loop detection the walks are other walks (each is
cut at its first detected loop), so compare steps/s together with the steps and walks/s columns.

--unique measures every form twice, without and with the distinct-state count (count_unique=True, rows
named "<form>+unique"), alternating likewise: the walks are the same walks, so the cost of the mode is
the ratio of a form's two rows (profiles/sim_unique_rate.txt). --unique-capacity sizes the table
(default: the engine's own, min(walks * (max_depth + 1), 2**28)). The first counted run's
per-batch new-state counts are printed as well: how coverage grows over the batches of one run.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import stateright_amd as sr  # noqa: E402
from stateright_amd import _native as N  # noqa: E402

MODELS = {
    "2pc": lambda n: sr.TwoPhaseSys(n),
    "paxos": lambda n: sr.Paxos(n),
    "increment_lock": lambda n: sr.IncrementLock(n),
    "increment": lambda n: sr.Increment(n),
}


def run(model, seed, walks, depth, refill, grid, loops=False, unique=False, capacity=None):
    os.environ["SR_SIM_REFILL"] = str(refill)  # both read when the engine is created
    os.environ["SR_SIM_GRID"] = str(grid)
    kw = {"detect_loops": True} if loops else {}  # (an A/B library of older sources has no such option)
    if unique:
        kw.update(count_unique=True, unique_capacity=capacity)
    c = model.checker().spawn_simulation(seed, walks=walks, max_depth=depth, **kw).join()
    st = c.stats()
    ran = c.state_count() - st["successors"]  # walks started
    out = {"steps": st["successors"], "walks": ran, "sec": st["level_loop_sec"], "launches": st["expand_launches"],
           "longest": c.max_depth(), "discovered": sorted(c.discoveries())}
    if unique:
        out["unique"] = c.unique_info()
        out["batch_new"] = c.batch_new_states()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=sorted(MODELS))
    ap.add_argument("n", type=int)
    ap.add_argument("--walks", type=int, default=11_000_000)
    ap.add_argument("--max-depth", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-walks", type=int, default=10_000)
    ap.add_argument("--grids", type=int, nargs="*", default=[0],
                    help="persistent form: grid caps in workgroups of 256 lanes to measure (0 = the engine's own cap)")
    ap.add_argument("--loops", action="store_true", help="measure every form without and with loop detection")
    ap.add_argument("--unique", action="store_true", help="measure every form without and with the distinct-state count")
    ap.add_argument("--unique-capacity", type=int, default=None, help="--unique: distinct states the table is sized for")
    a = ap.parse_args()
    model = MODELS[a.model](a.n)

    t0 = time.perf_counter()
    hsteps = sum(N.sim_walk(model.MODEL_ID, model.params(), a.seed, i, a.max_depth, 1)["steps"] for i in range(a.host_walks))
    hsec = time.perf_counter() - t0
    print(f"host: {a.host_walks} walks, {hsteps} steps in {hsec:.3f} s: {hsteps / hsec:.3e} steps/s, "
          f"{a.host_walks / hsec:.3e} walks/s (one thread, through ctypes)")

    forms = [("static", 0, 0, False)] + [("persistent" + (f"/{g}" if g else ""), 1, g, False) for g in a.grids]
    if a.loops:
        forms = [f for name, refill, grid, _ in forms for f in ((name, refill, grid, False), (name + "+loops", refill, grid, True))]
    forms = [f + (False,) for f in forms]
    if a.unique:
        forms = [f for name, refill, grid, loops, _ in forms
                 for f in ((name, refill, grid, loops, False), (name + "+unique", refill, grid, loops, True))]
    for _, refill, grid, loops, unique in forms:  # warm-up: context, allocations, code objects
        run(model, a.seed, a.walks, a.max_depth, refill, grid, loops, unique, a.unique_capacity)
    rows = {f[0]: [] for f in forms}
    for _ in range(a.repeats):
        for name, refill, grid, loops, unique in forms:
            rows[name].append(run(model, a.seed, a.walks, a.max_depth, refill, grid, loops, unique, a.unique_capacity))
    out = {"model": a.model, "n": a.n, "walks": a.walks, "max_depth": a.max_depth, "repeats": a.repeats,
           "digest": N.build_digest(), "host_steps_per_s": hsteps / hsec}
    for name, _, _, _, unique in forms:
        r = rows[name]
        sps = [x["steps"] / x["sec"] for x in r]
        wps = [x["walks"] / x["sec"] for x in r]
        out[name] = {"steps_per_s_median": statistics.median(sps), "steps_per_s_min": min(sps), "steps_per_s_max": max(sps),
                     "walks_per_s_median": statistics.median(wps), "launches": r[0]["launches"], "steps": r[0]["steps"],
                     "walks_run": r[0]["walks"], "longest": r[0]["longest"], "discovered": r[0]["discovered"]}
        print(f"{name:15s}: steps/s median {out[name]['steps_per_s_median']:.3e} (min {min(sps):.3e}, max {max(sps):.3e}), "
              f"walks/s median {out[name]['walks_per_s_median']:.3e}; {r[0]['launches']} launches, {r[0]['walks']} walks, "
              f"{r[0]['steps']} steps, longest {r[0]['longest']}")
        if unique:
            u, new = r[0]["unique"], r[0]["batch_new"]
            out[name].update(unique=u, batch_new=new)
            print(f"{'':15s}  distinct {u['unique']} of {r[0]['steps'] + r[0]['walks']} visited, table {u['slots']} slots "
                  f"(capacity {u['capacity']}), overflow {u['overflow']}; new per batch: {new}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
