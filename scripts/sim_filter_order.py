#!/usr/bin/env python3
"""CPU simulation of expand_fast's duplicate filter on 2pc, per append order of the new states.

What it models (stateright_amd/csrc/kernels.hpp, expand_fast, narrow states):
  * a level's frontier is cut into chunks of 256 consecutive rows, a chunk into 4 waves of 64 parents;
  * a wave walks its successor map (parents in row order, each parent's enabled slots in ascending
    order, self-loops counted and dropped) in rounds of 64 successors;
  * a chunk has a 1024-entry direct-mapped filter: a successor whose slot holds its own key is a
    duplicate and is not probed; any other successor takes the slot and is probed (a "first probe");
    the waves of a chunk run their rounds side by side: round 0 of waves 0-3, round 1 of waves 0-3, ...;
  * a probed successor that is not in the visited set is new (the first in that order wins);
  * the new states of a chunk are appended to the next frontier in one of two orders:
      interleaved  by round, the waves interleaved (one stage shared by the workgroup's waves)
      grouped      by wave, each wave's in its own append order (one stage region per wave)
    and the chunks' blocks follow each other in chunk order (the order of whole blocks does not matter).

It prints, per order, the unique states, the generated states (the checker's state_count: the init
state and every enabled action, self-loops included), the successors that enter the filter, the
first probes and a per-level table. The counts of states are those of any BFS; the first probes are
the simulation's result. No GPU is used; numpy does the per-level work.

    scripts/sim_filter_order.py 8
    scripts/sim_filter_order.py 9 --orders grouped
"""
import argparse
import sys
import time

import numpy as np

CHUNK, WAVE, WPB, FILTER = 256, 64, 4, 1024
ORDERS = ("interleaved", "grouped")
U = np.uint64


def _u(x):
    return np.uint64(x)


class TwoPhase:
    """The 2pc model in the engine's encoding (models.hpp TwoPhaseT): rm_state 2 bits per rm at 0,
    tm_state at 2n, tm_prepared at 2n+2, Prepared{rm} at 3n+2, Commit at 4n+2, Abort at 4n+3.
    Slots: 0 TmCommit, 1 TmAbort, 2+5rm+k: TmRcvPrepared, RmPrepare, RmChooseToAbort, RmRcvCommitMsg,
    RmRcvAbortMsg."""

    def __init__(self, n):
        assert 1 <= n <= 12
        self.n = n
        self.slots = 2 + 5 * n
        clr, st = [], []
        for a in range(self.slots):
            tm = a < 2
            rm, k = (0, 0) if tm else divmod(a - 2, 5)
            fpos = 2 * n if tm else 2 * rm
            fval = a + 1 if tm else (1 if k == 1 else 2 if k == 3 else 3)
            fmask = (3 << fpos) if (tm or k != 0) else 0
            epos = 4 * n + 2 + a if tm else (2 * n + 2 if k == 0 else 3 * n + 2) + rm
            ebit = (1 << epos) if (tm or k <= 1) else 0
            clr.append(fmask)
            st.append(((fval << fpos) & fmask) | ebit)
        self.keep = ~np.array(clr, dtype=U)
        self.set = np.array(st, dtype=U)

    def init(self):
        return np.zeros(1, dtype=U)

    def enabled(self, s):
        """(enabled, moves): bool arrays [len(s), slots]; moves leaves out the self-loops."""
        n = self.n
        rmask = _u((1 << n) - 1)
        tm0 = ((s >> _u(2 * n)) & _u(3)) == 0
        prepared = (s >> _u(2 * n + 2)) & rmask
        msgp = (s >> _u(3 * n + 2)) & rmask
        commit = ((s >> _u(4 * n + 2)) & _u(1)) != 0
        abort = ((s >> _u(4 * n + 3)) & _u(1)) != 0
        en = np.zeros((len(s), self.slots), dtype=bool)
        loop = np.zeros((len(s), self.slots), dtype=bool)
        en[:, 0] = tm0 & (prepared == rmask)
        en[:, 1] = tm0
        for rm in range(n):
            r = (s >> _u(2 * rm)) & _u(3)
            b = 2 + 5 * rm
            en[:, b] = tm0 & (((msgp >> _u(rm)) & _u(1)) != 0)
            loop[:, b] = en[:, b] & (((prepared >> _u(rm)) & _u(1)) != 0)
            en[:, b + 1] = en[:, b + 2] = r == 0
            en[:, b + 3] = commit
            loop[:, b + 3] = commit & (r == 2)
            en[:, b + 4] = abort
            loop[:, b + 4] = abort & (r == 3)
        return en, en & ~loop

    def apply(self, s, a):
        return (s & self.keep[a]) | self.set[a]


def _mix(x):
    """The filter's slot hash (a 64-bit finaliser; any well-mixed hash gives the same pass rates)."""
    x = x.copy()
    x ^= x >> _u(33)
    x *= _u(0xFF51AFD7ED558CCD)
    x ^= x >> _u(33)
    x *= _u(0xC4CEB9FE1A85EC53)
    x ^= x >> _u(33)
    return x


def _chunk_passes(model, rows, first_row):
    """The successors of frontier rows `rows` (a whole number of chunks, first_row their rank).
    Returns (generated, entering, state, grouped_rank) of the successors that pass the filter, in
    the order in which the chunk's waves reach them; grouped_rank orders them by (chunk, wave, the
    wave's own order)."""
    en, mv = model.enabled(rows)
    generated = int(en.sum())
    p, a = np.nonzero(mv)  # row-major: parents in row order, slots ascending = the waves' maps
    if len(p) == 0:
        return generated, 0, np.zeros(0, dtype=U), np.zeros(0, dtype=np.int64)
    st = model.apply(rows[p], a)
    r = p + first_row
    wave = r // WAVE
    # position of each successor in its wave's map
    start = np.flatnonzero(np.r_[True, wave[1:] != wave[:-1]])
    pos = np.arange(len(p)) - np.repeat(start, np.diff(np.r_[start, len(p)]))
    chunk = r // CHUNK
    # the order in time: chunk, round, wave, lane (lexsort: last key first)
    when = np.lexsort((pos % WAVE, wave % WPB, pos // WAVE, chunk))
    st_t, chunk_t = st[when], chunk[when]
    slot = chunk_t * FILTER + (_mix(st_t) & _u(FILTER - 1)).astype(np.int64)
    by_slot = np.argsort(slot, kind="stable")
    s_sorted, k_sorted = slot[by_slot], st_t[by_slot]
    hit_sorted = np.r_[False, (s_sorted[1:] == s_sorted[:-1]) & (k_sorted[1:] == k_sorted[:-1])]
    hit = np.empty(len(p), dtype=bool)
    hit[by_slot] = hit_sorted
    keep = ~hit
    return generated, len(p), st_t[keep], (when[keep] + 0).astype(np.int64)


def simulate(n, order, block_chunks=256, out=None):
    """Runs the BFS of 2pc(n) with the given append order. Returns a dict of totals and `levels`."""
    assert order in ORDERS
    model = TwoPhase(n)
    frontier = model.init()
    visited = frontier.copy()
    tot = dict(n=n, order=order, unique=1, generated=1, entering=0, first_probes=0, levels=[])
    depth = 0
    while len(frontier):
        depth += 1
        gen = ent = 0
        states, ranks = [], []
        step = block_chunks * CHUNK
        base = 0  # successors before this block, so that grouped ranks are global
        for lo in range(0, len(frontier), step):
            rows = frontier[lo:lo + step]
            g, e, st, gr = _chunk_passes(model, rows, lo)
            gen += g
            ent += e
            states.append(st)
            ranks.append(gr + base)
            base += e
        st = np.concatenate(states)
        gr = np.concatenate(ranks)
        # new: the first pass (in time) of a state that is not visited yet
        uniq, first = np.unique(st, return_index=True)
        fresh = ~np.isin(uniq, visited, assume_unique=True)
        uniq, first = uniq[fresh], first[fresh]
        key = first if order == "interleaved" else gr[first]
        nxt = uniq[np.argsort(key, kind="stable")]
        lv = dict(level=depth, parents=len(frontier), generated=gen, entering=ent, first_probes=len(st), new=len(nxt))
        tot["levels"].append(lv)
        tot["generated"] += gen
        tot["entering"] += ent
        tot["first_probes"] += len(st)
        tot["unique"] += len(nxt)
        if out:
            print("  level %2d parents %8d entering %9d first probes %9d pass %.3f new %8d" % (
                depth, lv["parents"], ent, len(st), len(st) / ent if ent else 0.0, len(nxt)), file=out, flush=True)
        visited = np.union1d(visited, nxt)
        frontier = nxt
    tot["nlevels"] = depth
    return tot


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("n", type=int, help="resource managers of 2pc")
    ap.add_argument("--orders", default=",".join(ORDERS), help="comma-separated: " + ", ".join(ORDERS))
    a = ap.parse_args(argv)
    res = []
    for order in a.orders.split(","):
        t0 = time.time()
        print("2pc N=%d, append order %s" % (a.n, order), flush=True)
        r = simulate(a.n, order, out=sys.stdout)
        print("  unique %d generated %d entering the filter %d first probes %d (pass %.3f) levels %d  [%.0f s]" % (
            r["unique"], r["generated"], r["entering"], r["first_probes"],
            r["first_probes"] / max(1, r["entering"]), r["nlevels"], time.time() - t0), flush=True)
        res.append(r)
    if len(res) == 2:
        a0, a1 = res[0]["first_probes"], res[1]["first_probes"]
        print("first probes: %s %d, %s %d, change %+.1f %%" % (res[0]["order"], a0, res[1]["order"], a1,
                                                                100.0 * (a1 - a0) / a0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
