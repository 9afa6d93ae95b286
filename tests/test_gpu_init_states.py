"""Many, wide and duplicate init states on every code path that puts them into a check.

The single engine has three (csrc/engine.hpp Engine::run): `roots_start` while the k init states of
W words fit the kernel arguments (k W <= 32 words), `roots_fused` after a host copy up to 256 states,
and `insert_roots` + `eval_roots` + `publish_kernel` past that; the partitioned engine has two (the
replicated head, and `insert_roots_part` per partition with SR_HEAD_MAX=0); the simulation reads them
from the kernel arguments or, past 32 words, from device memory. Each case derives the path it must
take from k and W and asserts it from sr_stats.root_path.

The model is the Spread fixture with a list of init states (the subsets 0 .. R-1, then 0 .. D-1 again),
compared exactly with the Python restatement of the reference's search (oracle/pybfs.py: duplicates
are counted, queued and expanded again; level 0 is visited in reverse init order; a state keeps its
first generator) and with the closed forms; and a DGraph with 40 init nodes, compared with the C++
oracle. F = 12 throughout (4096 states)."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pybfs  # noqa: E402
from oracle_lib import DGRAPH, OracleRun, dgraph_params  # noqa: E402
from stateright_amd import DGraph, StateRecorder  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.distributed import Communicator  # noqa: E402
from stateright_amd.models import Spread  # noqa: E402
from stateright_amd.plugin import model_fingerprint  # noqa: E402

pytestmark = pytest.mark.gpu

F = 12
# 7 of 12 bits, root 3 inside it: from 4 roots on the shortest path starts at a root that is not 0
MARK = 0b010110011011
INLINE_WORDS = 32   # csrc/kernels.hpp ROOTS_INLINE_WORDS
FUSED_MAX = 256     # one workgroup of roots_fused
ALWAYS, EVENTUALLY, SOMETIMES = N.SR_ALWAYS, N.SR_EVENTUALLY, N.SR_SOMETIMES


def expected_root_path(words, k):
    if k * words <= INLINE_WORDS:
        return N.SR_ROOTS_INLINE
    return N.SR_ROOTS_FUSED if k <= FUSED_MAX else N.SR_ROOTS_LAUNCHES


def closed_form(roots, dup, loops):
    """(unique, state_count, max_depth) of Spread(.., F, loops, .., roots, dup): every duplicate root
    is popped and expanded a second time; a state's depth is the fewest bits it adds to a root inside it."""
    count = (roots + dup) + F * 2 ** (F - 1) + loops * 2 ** F + sum(F - bin(i).count("1") + loops for i in range(dup))
    depth = max(min(bin(x ^ r).count("1") for r in range(roots) if r & ~x == 0) for x in range(2 ** F))
    return 2 ** F, count, depth


@functools.lru_cache(maxsize=None)
def reference(words, bits, loops, roots, dup, mark=MARK):
    r = pybfs.spread_bfs(words, bits, F, loops, mark, roots, dup)
    assert (r["unique"], r["state_count"], r["max_depth"]) == closed_form(roots, dup, loops)
    r["multiset"] = collections.Counter(r["visits"])
    r["inits"] = [pybfs.spread_describe(words, bits, F, x) for x in pybfs.spread_inits(roots, dup)]
    # the shortest path starts at the largest root inside the mark: root 3 from 4 roots on
    inside = [x for x in range(roots) if x & ~mark == 0]
    assert len(r["discoveries"]["marked"]) - 1 == min(bin(mark ^ x).count("1") for x in inside)
    if roots >= 4 and mark == MARK:
        assert r["discoveries"]["marked"][0][0] != 0
    return r


def run(words, bits, loops, roots, dup, order, partitions=1, mark=MARK):
    b = Spread(words, bits, F, loops, mark, roots, dup).checker().order(order)
    rec = StateRecorder()
    b = b.visitor(rec)
    if partitions > 1:
        b = b.partitions(partitions)
    c = b.spawn_bfs().join()
    c.assert_properties()
    return c, rec


def check_counts(c, ref):
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (ref["unique"], ref["state_count"], ref["max_depth"])
    assert sorted(c.discoveries()) == ["marked"]


def check_path_replays(c, ref):
    """The discovery is a shortest path from an init state through reachable states, and replays from
    the position of its first state in the model's init order."""
    path = c.discovery("marked")
    assert len(path) == len(ref["actions"]["marked"])
    assert path.states[0] in ref["inits"] and path.last_state() == ref["discoveries"]["marked"][-1]
    assert all(s in ref["multiset"] for s in path.states)
    i = ref["inits"].index(path.states[0])
    replayed = c.replay(path.action_ids, init_index=i)
    assert replayed is not None and replayed[0] == path.states and replayed[1] == [1, 1]
    c.assert_discovery("marked", path.into_actions())


def check_single(words, bits, loops, roots, dup, order):
    ref = reference(words, bits, loops, roots, dup)
    k = roots + dup
    c, rec = run(words, bits, loops, roots, dup, order)
    assert c.stats()["root_path"] == expected_root_path(words, k), c.stats()
    check_counts(c, ref)
    path = c.discovery("marked")
    if order == "fifo":
        # the reversed level 0 with its duplicates, then every level in the reference's order
        assert rec.states[:k] == ref["inits"][::-1]
        assert rec.states == ref["visits"]
        assert path.states == ref["discoveries"]["marked"] and path.action_ids == ref["actions"]["marked"]
    else:
        assert collections.Counter(rec.states) == ref["multiset"]
    check_path_replays(c, ref)
    # (host side) the init states as the handle reports them: all k, the duplicates included, in init order
    assert c._lib.sr_gpu_bfs_init_count(c._h) == k == len(ref["inits"])
    for i, want in enumerate(ref["inits"]):
        assert c.replay([], init_index=i) == ([want], [1, 0])
    assert c.replay([], init_index=k) is None
    return c


# (words, key_bits, roots, dup): k = roots + dup on both sides of k W = 32 words and of k = 256, with
# duplicates on every path; (1, 150, 106) and (1, 200, 100) have duplicates past lane 63 of level 0
SWEEP = [
    (1, 45, 1, 0), (1, 45, 2, 0), (1, 32, 1, 1), (1, 44, 29, 3), (1, 64, 32, 0),      # inline (k <= 32)
    (1, 45, 33, 0), (1, 32, 64, 0), (1, 44, 60, 5), (1, 64, 150, 106),                # fused (33, 64, 65, 256)
    (1, 45, 257, 0), (1, 62, 200, 100),                                               # three launches (257, 300)
    (2, 79, 16, 0), (2, 128, 13, 3), (2, 79, 17, 0), (2, 60, 30, 10),                 # 16 | 17, 40
    (4, 128, 8, 0), (4, 50, 6, 2), (4, 128, 9, 0), (4, 78, 33, 7),                    # 8 | 9, 40
]


def test_sweep_sits_on_both_sides_of_every_threshold():
    ks = {w: sorted({r + d for ww, _, r, d in SWEEP if ww == w}) for w in (1, 2, 4)}
    assert ks == {1: [1, 2, 32, 33, 64, 65, 256, 257, 300], 2: [16, 17, 40], 4: [8, 9, 40]}
    with_dup = {expected_root_path(w, r + d) for w, _, r, d in SWEEP if d}
    assert with_dup == {N.SR_ROOTS_INLINE, N.SR_ROOTS_FUSED, N.SR_ROOTS_LAUNCHES}
    assert any(d > 64 for _, _, _, d in SWEEP)


@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("words,bits,roots,dup", SWEEP)
def test_root_paths(words, bits, roots, dup, order):
    check_single(words, bits, 1, roots, dup, order)


# (words, key_bits, roots, dup, mark): "marked" holds at an init state, so it is the roots' own
# evaluation that discovers it (inline, fused, three launches; 37 is also among the duplicates of the last)
MARKED_ROOTS = [(1, 45, 20, 5, 13), (2, 79, 10, 4, 2), (1, 45, 100, 20, 37), (4, 78, 33, 7, 21), (1, 62, 200, 100, 37),
                (1, 45, 300, 0, 290)]


@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("words,bits,roots,dup,mark", MARKED_ROOTS)
def test_discovery_is_a_root(words, bits, roots, dup, mark, order):
    ref = reference(words, bits, 1, roots, dup, mark)
    want = pybfs.spread_describe(words, bits, F, mark)
    assert ref["discoveries"]["marked"] == [want] and ref["actions"]["marked"] == []
    c, rec = run(words, bits, 1, roots, dup, order, mark=mark)
    assert c.stats()["root_path"] == expected_root_path(words, roots + dup)
    check_counts(c, ref)  # "in range" is never discovered, so the check explores everything all the same
    path = c.discovery("marked")
    assert path.states == [want] and path.action_ids == []
    assert c.discovery_fingerprints("marked") == [model_fingerprint(c.model(), list(want))]
    if order == "fifo":
        assert rec.states == ref["visits"]
    else:
        assert collections.Counter(rec.states) == ref["multiset"]
    assert c.replay([], init_index=mark) == ([want], [1, 1])
    c.assert_discovery("marked", [])


FEW = [(1, 62, 200, 100), (4, 78, 33, 7)]


@pytest.mark.parametrize("env", [{"SR_PIPELINE": "0"}, {"SR_GRID_MAX": "2"}, {"SR_GRID_MAX": "2", "SR_PIPELINE": "0"}],
                         ids=["nopipe", "grid2", "grid2-nopipe"])
@pytest.mark.parametrize("words,bits,roots,dup", FEW)
def test_level0_of_hundreds_few_workgroups(words, bits, roots, dup, env, monkeypatch):
    # level 0 is a frontier of k states: without level pipelining, and strided by two workgroups
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    check_single(words, bits, 2, roots, dup, "fast")


# ---- DGraph: 40 init nodes (W = 1, k = 40: the host copy, roots_fused, the `eventually` bits filled) ----
# Init nodes 100 .. 139, visited 139 first. 104 .. 139 step to the odd terminal 201; 111 and then 110
# step to the even terminal 202, which keeps the (cleared) bit of the odd 111 that generates it first, so
# the even 110 yields nothing (the reference's known false negative); 103 steps to the odd 203; 102, 101
# and 100 step to 150 and 150 to the even terminal 220: 102 generates 150 first, so the terminal state
# that still holds its bit is 220, on the path 102 -> 150 -> 220 from the 38th root visited.
DG_ROOTS = list(range(100, 140))
DG_PATHS = [[r, 201] for r in range(104, 140)] + [[111, 202], [110, 202], [103, 203], [102, 150, 220], [101, 150], [100, 150]]


def dgraph(expectation, paths, order=None):
    g = DGraph(expectation, paths)
    rec = StateRecorder()
    b = g.checker().visitor(rec)
    if order:
        b = b.order(order)
    return b.spawn_bfs().join(), rec


def check_against_oracle(expectation, paths, order=None):
    o = OracleRun(DGRAPH, dgraph_params(expectation, paths), record_visits=True)
    c, rec = dgraph(expectation, paths, order)
    st = c.stats()
    assert st["order_used"] == N.SR_ORDER_FIFO and st["root_path"] == N.SR_ROOTS_FUSED, st
    assert c._lib.sr_gpu_bfs_init_count(c._h) == 40
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (o.unique_state_count, o.state_count, o.max_depth)
    assert rec.states == o.visits()
    assert sorted(c.discoveries()) == o.discovery_names() == ["odd"]
    path = c.discovery("odd")
    assert path.into_states() == o.discovery_states("odd") and path.action_ids == o.discovery_actions("odd")
    c.assert_discovery("odd", path.action_ids)
    return c, rec, path


def test_eventually_bits_pending_on_forty_roots():
    c, rec, path = check_against_oracle(EVENTUALLY, DG_PATHS)
    assert [s[0] for s in rec.states[:40]] == DG_ROOTS[::-1]
    assert [s[0] for s in rec.states[40:]] == [201, 202, 203, 150, 220]
    # from a root that is neither the first nor the last init state, past the first 32 of level 0
    assert path.into_states() == [(102,), (150,), (220,)]


def test_discovery_among_forty_roots_has_the_reference_rank():
    # the first root in REVERSED init order that discovers: sometimes "odd" 141, 140, 138, [137];
    # always "odd" 141, 139, 137, [136]
    some = [[r, 200] for r in list(range(100, 137)) + [137, 138, 140]]
    _, rec, path = check_against_oracle(SOMETIMES, some, "fifo")
    assert path.into_states() == [(137,)] and [s[0] for s in rec.states] == [140, 138, 137]
    always = [[r, 201] for r in list(range(100, 138)) + [139, 141]]
    _, rec, path = check_against_oracle(ALWAYS, always, "fifo")
    assert path.into_states() == [(136,)] and [s[0] for s in rec.states] == [141, 139, 137, 136]


# ---- partitioned: the replicated head, and each partition taking the roots it owns ----
PARTITIONED = [(1, 44, 60, 5), (1, 62, 200, 100), (4, 78, 33, 7)]


@pytest.mark.parametrize("head", [None, "0"], ids=["head", "parts"])
@pytest.mark.parametrize("words,bits,roots,dup", PARTITIONED)
def test_partitioned(words, bits, roots, dup, head, monkeypatch):
    if head is not None:
        monkeypatch.setenv("SR_HEAD_MAX", head)
    ref = reference(words, bits, 1, roots, dup)
    c, rec = run(words, bits, 1, roots, dup, "fast", partitions=3)
    st = c.stats()
    assert st["root_path"] == (N.SR_ROOTS_HEAD if head is None else N.SR_ROOTS_PARTS), st
    assert c._lib.sr_gpu_bfs_init_count(c._h) == roots + dup
    check_counts(c, ref)
    assert collections.Counter(rec.states) == ref["multiset"]
    check_path_replays(c, ref)


@pytest.mark.parametrize("head", [None, "0"], ids=["head", "parts"])
def test_partitioned_discovery_is_a_root(head, monkeypatch):
    # "marked" holds at an init state (and at its duplicate): found by the evaluation of the roots
    if head is not None:
        monkeypatch.setenv("SR_HEAD_MAX", head)
    words, bits, roots, dup, mark = 1, 62, 200, 100, 37
    ref = reference(words, bits, 1, roots, dup, mark)
    want = pybfs.spread_describe(words, bits, F, mark)
    c, rec = run(words, bits, 1, roots, dup, "fast", partitions=3, mark=mark)
    assert c.stats()["root_path"] == (N.SR_ROOTS_HEAD if head is None else N.SR_ROOTS_PARTS)
    check_counts(c, ref)
    assert collections.Counter(rec.states) == ref["multiset"]
    path = c.discovery("marked")
    assert path.states == [want] and path.action_ids == []
    assert c.replay([], init_index=mark) == ([want], [1, 1])
    c.assert_discovery("marked", [])


def test_partitioned_ranks(monkeypatch):
    # two in-process ranks, every level partitioned: each rank takes the roots it owns
    monkeypatch.setenv("SR_HEAD_MAX", "0")
    words, bits, roots, dup = 1, 44, 60, 5
    ref = reference(words, bits, 1, roots, dup)
    comms = Communicator.local_group(2)
    cs = []
    try:
        for cm in comms:
            b = Spread(words, bits, F, 1, MARK, roots, dup).checker().order("fast").comm(cm)
            cs.append(b.spawn_bfs())
        for c in cs:
            c.join()
        for c in cs:
            assert c.stats()["root_path"] == N.SR_ROOTS_PARTS
            check_counts(c, ref)
            check_path_replays(c, ref)
        cs.clear()
    finally:
        cs.clear()
        for cm in comms:
            cm.close()


# ---- simulation: the init states read from device memory (k W > 32 words) ----
SIM_SEED = 20240607
SIM_DEPTH = 10
SIM_SPREAD = (4, 78, 10, 2)                                     # W = 4, k = 12: 48 words
SIM_DG_PATHS = [[r, 200 + r % 4] for r in DG_ROOTS] + [[100, 200, 230], [104, 200, 231], [101, 201, 230], [102, 202, 231]]


def sim_models():
    w, b, r, d = SIM_SPREAD
    return {"spread": Spread(w, b, F, 0, MARK, r, d), "dgraph": DGraph(SOMETIMES, SIM_DG_PATHS)}


@functools.lru_cache(maxsize=None)
def host_walks(name):
    m = sim_models()[name]
    return [N.sim_walk(m.MODEL_ID, m.params(), SIM_SEED, i, SIM_DEPTH, 2) for i in range(1000)]


@pytest.mark.parametrize("refill", ["0", "1"])
@pytest.mark.parametrize("name", ["spread", "dgraph"])
def test_simulation_starts_from_the_device_copy_of_the_init_states(name, refill, monkeypatch):
    monkeypatch.setenv("SR_SIM_REFILL", refill)
    monkeypatch.setenv("SR_SIM_GRID", "1")
    ws = host_walks(name)
    steps = np.array([w["steps"] for w in ws], dtype=np.uint32)
    end = np.array([w["end"] for w in ws], dtype=np.uint32)
    fp = np.array([w["final_fp"] for w in ws], dtype=np.uint64)
    m = sim_models()[name]
    for walks in (1, 65, 1000):
        c = m.checker().spawn_simulation(SIM_SEED, walks=walks, max_depth=SIM_DEPTH, record_walks=True).join()
        st = c.stats()
        assert st["root_path"] == N.SR_ROOTS_BUFFER, st
        assert c._lib.sr_gpu_bfs_init_count(c._h) == (12 if name == "spread" else 40)
        ds, de, df = c.walk_records_arrays()
        assert len(ds) == walks
        assert np.array_equal(ds, steps[:walks]) and np.array_equal(de, end[:walks]) and np.array_equal(df, fp[:walks])
        assert c.state_count() == int(steps[:walks].astype(np.int64).sum()) + walks
        assert c.max_depth() == int(steps[:walks].max())
        assert st["successors"] == c.state_count() - walks and st["levels"] == st["expand_launches"] == 1
    # apart from the shared walk definition: where the device's walks ended, from the model alone
    if name == "spread":
        w_, b_, r_, _ = SIM_SPREAD
        fp_of = {x: model_fingerprint(m, list(pybfs.spread_describe(w_, b_, F, x))) for x in range(2 ** F)}
        started = collections.Counter()
        for i, w in enumerate(ws):
            bits = sum(1 << a for a in w["actions"])
            assert bin(bits).count("1") == w["steps"] == int(ds[i])
            ends = [r for r in range(r_) if r & bits == 0 and fp_of[r | bits] == int(df[i])]
            assert len(ends) == 1, (i, w, ends)
            started[ends[0]] += 1
            full = ends[0] | bits == 2 ** F - 1
            assert int(de[i]) == (N.SIM_TERMINAL if full and w["steps"] < SIM_DEPTH else N.SIM_DEPTH)
        assert sorted(started) == list(range(r_))  # every root starts some walk
    else:
        edges = {(p[j], p[j + 1]) for p in SIM_DG_PATHS for j in range(len(p) - 1)}
        firsts = set()
        for i, w in enumerate(ws):
            a = w["actions"]
            assert any((r, a[0]) in edges for r in DG_ROOTS), (i, a)
            assert all(e in edges for e in zip(a, a[1:])), (i, a)
            assert int(de[i]) == N.SIM_TERMINAL and a[-1] in (203, 230, 231)
            firsts.add(a[0])
        assert firsts == {200, 201, 202, 203}
