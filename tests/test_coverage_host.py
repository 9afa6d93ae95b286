"""The coverage pass' host form (sr_coverage_host, csrc/cover.hpp; no device needed) against figures that
Python derives on its own from the reachable graph (`_native.host_graph`: per state the (action id,
successor) pairs of the taken slots and the mask of the conditions that hold).

From the graph alone: states, terminal, stutter_ends, out_degree, max_out_degree, holds, and taken / moved
per action id (the id-class models), per message kind (paxos: the kind is a field of the id), per
(Drop | Deliver | Timeout, destination) for the actor encodings (both are fields of the id). `enabled` is
not in the graph: it equals `taken` where every listed action yields a state (DGraph, 2pc, ...), and is
at least `taken` elsewhere."""
import ctypes
import functools

import pytest

sr = pytest.importorskip("stateright_amd")

from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import LiveGraph, Spread  # noqa: E402

ALWAYS, EVENTUALLY, SOMETIMES = N.SR_ALWAYS, N.SR_EVENTUALLY, N.SR_SOMETIMES


def dgraph(expectation, paths):
    g = sr.DGraph.with_property(expectation)
    for p in paths:
        g = g.with_path(p)
    return g


# (key, model, how a class index follows from an action id (None: only the sums are compared),
#  whether every listed action yields a state)
def by_id(i):
    return i


def paxos_kind(i):
    return i // 256 % 16


def actor_class(nact):
    def f(i):
        kind, code = i & 3, i >> 2
        if kind == 3:  # Timeout(code)
            return 2 * nact + code
        dst = code // 16 % 128
        return (1 if kind == 1 else 0) * nact + dst if dst < nact else 3 * nact
    return f


# The search stops once every property has a discovery, so on the GPU these have no figures (the host form
# has no such stop): Increment's one property is violated, and a search refutes `eventually` at a terminal state.
STOP_EARLY = ("increment_3", "dgraph_terminal", "live_graph_terminals")
UNREACHABLE = dgraph(ALWAYS, [[1, 3, 5]])  # node 7 is never an edge's target: class "7" has enabled == 0
MODELS = {
    "dgraph_one_state": (dgraph(ALWAYS, [[1]]), by_id, True),
    "dgraph_unreachable": (UNREACHABLE, by_id, True),
    "dgraph_cycle": (dgraph(EVENTUALLY, [[0, 2, 4, 2], [9, 9]]), by_id, True),
    "dgraph_terminal": (dgraph(EVENTUALLY, [[0, 2, 4, 2], [0, 6], [9, 9]]), by_id, True),
    "2pc_3": (sr.TwoPhaseSys(3), by_id, True),
    "increment_3": (sr.Increment(3), by_id, True),
    "increment_lock_3": (sr.IncrementLock(3), by_id, True),
    "spin_lock_3": (sr.SpinLockSys(3), by_id, True),
    "ping_pong_2_lossy": (sr.PingPong(2, lossy=True), actor_class(2), False),
    "ping_pong_3_history": (sr.PingPong(3, maintains_history=True, duplicating=False), actor_class(2), False),
    "ping_pong_wide_8": (sr.PingPong(8), actor_class(2), False),
    "paxos_1": (sr.Paxos(1), paxos_kind, True),
    "paxos_2": (sr.Paxos(2), paxos_kind, True),
    "single_copy_2": (sr.SingleCopyRegister(2, 1), actor_class(3), False),
    "abd_1_2": (sr.AbdRegister(1, 2), actor_class(3), False),
    "spread_roots_dup": (Spread(1, 20, 6, loops=2, mark=5, roots=5, dup=3), by_id, True),
    "spread_2_words": (Spread(2, 100, 5, loops=1, mark=3, roots=3, dup=3), by_id, True),
    "live_graph_dup": (LiveGraph(8, 2, 1, 1, 5, roots=7, dup=4), by_id, True),
    "live_graph_terminals": (LiveGraph(8, 2, 1, 3, 5, roots=7, dup=4), by_id, True),
    "live_graph_2_words": (LiveGraph(8, 3, 7, 1, 9, roots=3, words=2, dup=2), by_id, True),
    "live_graph_4_words": (LiveGraph(10, 2, 3, 2, 0, roots=2, words=4, dup=1), by_id, True),
}


@functools.lru_cache(maxsize=None)
def host(key):
    m = MODELS[key][0]
    return N.coverage_host(m.MODEL_ID, m.params())


@functools.lru_cache(maxsize=None)
def graph(key):
    m = MODELS[key][0]
    return N.host_graph(m.MODEL_ID, m.params())


def derive(succ, conds, nprops, nclasses, class_of):
    """The figures of the definition, from the graph alone."""
    out = {"states": len(succ), "terminal": 0, "stutter_ends": 0, "max_out_degree": 0, "out_degree": [0] * 64,
           "holds": [0] * nprops, "taken": [0] * nclasses, "moved": [0] * nclasses}
    for i, edges in enumerate(succ):
        deg = len(edges)
        mdeg = sum(1 for _, j in edges if j != i)
        out["terminal"] += deg == 0
        out["stutter_ends"] += deg > 0 and mdeg == 0
        out["out_degree"][min(deg, 63)] += 1
        out["max_out_degree"] = max(out["max_out_degree"], deg)
        for p in range(nprops):
            out["holds"][p] += conds[i] >> p & 1
        for a, j in edges:
            out["taken"][class_of(a)] += 1
            out["moved"][class_of(a)] += j != i
    return out


@pytest.mark.parametrize("key", sorted(MODELS))
def test_host_form_matches_the_graph(key):
    _, class_of, all_succeed = MODELS[key]
    cov = host(key)
    succ, inits, conds = graph(key)
    want = derive(succ, conds, cov["nprops"], cov["n_classes"], class_of)
    assert cov["ran"] == 1 and cov["states"] == want["states"] == len(succ)
    for f in ("terminal", "stutter_ends", "max_out_degree", "out_degree"):
        assert cov[f] == want[f], f
    assert list(cov["properties"].values()) == want["holds"]
    assert [c["taken"] for c in cov["classes"]] == want["taken"]
    assert [c["moved"] for c in cov["classes"]] == want["moved"]
    for c in cov["classes"]:
        assert c["enabled"] >= c["taken"] >= c["moved"], c
        if all_succeed:
            assert c["enabled"] == c["taken"], c
    # the identities
    assert sum(cov["out_degree"]) == cov["states"]
    if cov["max_out_degree"] < 63:
        assert sum(d * k for d, k in enumerate(cov["out_degree"])) == sum(c["taken"] for c in cov["classes"])
    assert len({c["name"] for c in cov["classes"]}) == cov["n_classes"] == len(cov["classes"])


def test_one_state_and_no_edge():
    cov = host("dgraph_one_state")
    assert (cov["states"], cov["terminal"], cov["stutter_ends"], cov["max_out_degree"]) == (1, 1, 0, 0)
    assert cov["n_classes"] == 256 and all(c["enabled"] == c["taken"] == c["moved"] == 0 for c in cov["classes"])
    assert cov["properties"] == {0: 1} and cov["out_degree"][0] == 1  # always "odd" holds at node 1


def test_a_class_never_enabled():
    cov = host("dgraph_unreachable")
    by_name = {c["name"]: c for c in cov["classes"]}
    assert by_name["3"]["enabled"] == by_name["5"]["enabled"] == 1 and by_name["7"]["enabled"] == 0
    assert sorted(n for n, c in by_name.items() if c["taken"]) == ["3", "5"]


def test_two_phase_commit_self_loops():
    cov = host("2pc_3")
    assert cov["states"] == 288 and cov["terminal"] == 0
    assert sum(c["taken"] for c in cov["classes"]) - sum(c["moved"] for c in cov["classes"]) == 384
    assert all(c["taken"] > 0 for c in cov["classes"])


def test_class_names_follow_the_hooks():
    assert [c["name"] for c in host("increment_3")["classes"]] == [f"{k}({t})" for t in range(3) for k in ("Read", "Write")]
    assert [c["name"] for c in host("increment_lock_3")["classes"]] == [
        f"{k}({t})" for t in range(3) for k in ("Lock", "Read", "Write", "Release")]
    assert [c["name"] for c in host("paxos_1")["classes"]] == list(sr.Paxos.KINDS)
    assert [c["name"] for c in host("ping_pong_2_lossy")["classes"]] == [
        "Drop(dst: Id(0))", "Drop(dst: Id(1))", "Deliver(dst: Id(0))", "Deliver(dst: Id(1))", "Timeout(Id(0))",
        "Timeout(Id(1))", "Drop(dst: no actor)"]
    # without a hook the classes are the slots: named as actions where the action ids are the slots
    # (LinearEquation), as slots where they are not (BinaryClock: one slot, two action ids)
    m = sr.LinearEquation(2, 4, 7)
    assert [c["name"] for c in N.coverage_host(m.MODEL_ID, m.params())["classes"]] == ["IncreaseX", "IncreaseY"]
    m = sr.BinaryClock()
    assert [c["name"] for c in N.coverage_host(m.MODEL_ID, m.params())["classes"]] == ["slot 0"]


def test_the_boundary_cuts_somewhere():
    # lossy ping-pong: a Deliver past max_nat is enabled and cut by within_boundary
    cov = host("ping_pong_2_lossy")
    assert any(c["enabled"] > c["taken"] for c in cov["classes"])
    assert sum(c["enabled"] for c in cov["classes"] if c["name"].startswith("Drop")) > 0


def test_wide_ping_pong_has_more_than_64_slots():
    m = MODELS["ping_pong_wide_8"][0]
    cov = host("ping_pong_wide_8")
    assert cov["states"] == len(graph("ping_pong_wide_8")[0]) > 1 and m.max_nat > 7


def test_duplicate_init_states_count_once():
    for key in ("spread_roots_dup", "live_graph_dup", "live_graph_2_words", "live_graph_4_words"):
        succ, inits, _ = graph(key)
        assert len(set(inits)) < len(inits)
        assert host(key)["states"] == len(succ)


def test_struct_sizes():
    assert ctypes.sizeof(N.sr_opts) == 72 and N.sr_opts.coverage.offset == 60
    assert ctypes.sizeof(N.sr_coverage) == 568 and N.sr_coverage.out_degree.offset == 56
    o = N.sr_opts()
    N.load().sr_opts_init(ctypes.byref(o))
    assert o.struct_size == 72 and o.coverage == 0


def _call(model_id, params, max_states, size=None):
    res = N.sr_coverage()
    res.struct_size = ctypes.sizeof(res) if size is None else size
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    st = N.load().sr_coverage_host(model_id, arr, len(params), max_states, ctypes.byref(res), None, None, None, 0, None, 0, None, 0)
    return st, res


def test_errors():
    m = sr.TwoPhaseSys(3)
    st, _ = _call(m.MODEL_ID, m.params(), 287)
    assert st == -3 and "max_states" in N.last_error()  # SR_ERR_CAPACITY
    st, res = _call(m.MODEL_ID, m.params(), 288)
    assert st == 288 and res.states == 288 and res.classes == 17
    st, _ = _call(999, [1], 100)
    assert st < 0
    st, _ = _call(m.MODEL_ID, m.params(), 0)
    assert st == -1
    with pytest.raises(ValueError, match="sr_coverage_host"):
        N.coverage_host(999, [1])
    # a caller with a shorter mirror: only its bytes are written
    st, res = _call(m.MODEL_ID, m.params(), 288, size=56)
    assert st == 288 and res.struct_size == 56 and res.states == 288 and list(res.out_degree) == [0] * 64
