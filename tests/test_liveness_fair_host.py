"""Progress fairness of the complete `eventually` check on the host (sr_liveness_host_fair, csrc/live.hpp):
the rule the kernels run, checked without a device against the independent Python restatement in
tests/live_fair_ref.py, in both modes: the sizes of N_p and F_p, the deterministic witness and how it
ends (terminal, loop, stutter end), on LiveGraph, DGraph with self-edges, ping-pong and 2pc with its two
`eventually` properties (TwoPhaseLiveSys)."""
import random

import pytest

import live_fair_ref as F
import live_ref
from oracle_lib import dgraph_params
from stateright_amd import _native as N
from stateright_amd.models import LiveGraph, PingPong, TwoPhaseLiveSys
from test_liveness_host import FIXME_CYCLE, PINGPONG_EVENTUALLY, random_graph

EVENTUALLY = N.SR_EVENTUALLY
MODES = (0, 1)  # sr_liveness_host_fair's `fairness`: none, progress

# LiveGraph parameters -> (|F| plain, |F| progress); the witness, or its absence, is the same in both modes
F_ANCHORS = {
    (12, 2, 1, 2, 0, 1): (475, 474),
    (12, 2, 3, 2, 0, 1): (104, 91),
    (12, 2, 1, 2, 0, 64): (477, 476),
    (16, 2, 1, 2, 0, 1): (1507, 1481),
    (10, 4, 11, 4, 0, 1): (771, 770),
    (6, 4, 9, 2, 8, 3): (27, 26),
}
STUTTER_ONLY = (4, 1, 3, 0, 0, 3)  # init state 2 has one action, which returns 2

# 2pc-live: N -> (|N|, |F|) of "every RM decides" in the plain mode (progress: |F| = 0), and (|N|, |F|,
# witness slots) of "every RM commits" under progress fairness (plain: [1, 3, 6, 6], loop_start 3)
STUTTER_ENDS = {1: 4, 2: 10, 3: 28, 4: 82}
DECIDES_PLAIN = {1: (7, 3), 2: (45, 45), 3: (259, 259), 4: (1485, 1485)}
COMMITS_PROGRESS = {
    1: (11, 10, [1, 3, 6]),
    2: (55, 52, [1, 3, 6, 8, 11]),
    3: (287, 280, [1, 3, 6, 8, 11, 13, 16]),
    4: (1567, 1552, [1, 3, 6, 8, 11, 13, 16, 18, 21]),
    5: (8831, 8800, [1, 3, 6, 8, 11, 13, 16, 18, 21, 23, 26]),
}


def random_live_graphs(count=40, seed=20250207):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n_bits = rng.randint(1, 10)
        out.append((n_bits, rng.randint(1, 4), rng.getrandbits(40), rng.choice([0, 1, 2, 2, 3, 3, 5]),
                    rng.choice([0, 0, 0, 3, 8, 16]), rng.randint(1, min(512, 2 ** n_bits))))
    return out


def random_self_graph(rng):
    """`random_graph` of tests/test_liveness_host.py with nodes doubled at random: paths like [0, 2, 2]."""
    out = []
    for p in random_graph(rng):
        q = []
        for v in p:
            q.extend([v, v] if rng.random() < 0.3 else [v])
        out.append(q)
    return out


def random_self_graphs(count=60, seed=4329):
    rng = random.Random(seed)
    return [random_self_graph(rng) for _ in range(count)]


def both_modes(graph):
    """The reference's answers (plain, progress); plain must be live_ref's."""
    plain, fair = F.check(*graph), F.check(*graph, skip_self=True)
    old = live_ref.check(*graph)
    assert {k: plain[k] for k in ("unique", "not_p_states", "surviving")} == {k: old[k] for k in ("unique", "not_p_states", "surviving")}
    assert (plain["witness"] is None) == (old["witness"] is None)
    if old["witness"] is not None:
        assert {k: plain["witness"][k] for k in old["witness"]} == old["witness"]
        assert plain["witness"]["end_kind"] == (F.END_LOOP if old["witness"]["loop_start"] >= 0 else F.END_TERMINAL)
    return plain, fair


def assert_matches(got, want, what):
    """got: liveness_host()'s dict; want: live_fair_ref.check() of the same graph and mode."""
    assert got["ran"] == 1, what
    assert (got["not_p_states"], got["surviving"]) == (want["not_p_states"], want["surviving"]), what
    w = want["witness"]
    if w is None:
        assert (got["init_index"], got["witness_len"], got["loop_start"], got["end_kind"], got["actions"]) == (-1, -1, -1, 0, []), what
    else:
        assert (got["init_index"], got["witness_len"], got["loop_start"], got["end_kind"]) == (
            w["init_index"], len(w["actions"]), w["loop_start"], w["end_kind"]), what
        assert got["actions"] == w["actions"], what
    assert got["rounds"] >= 1 and got["examined"] >= got["not_p_states"], what


def disagree(plain, fair):
    return (plain["surviving"], plain["witness"]) != (fair["surviving"], fair["witness"])


# ---- the random draws cover every outcome, on the reference alone -------------------------------------

def test_the_draws_cover_every_outcome_and_disagreements():
    for graphs in ([live_ref.live_graph(*p) for p in random_live_graphs()], [live_ref.dgraph(g) for g in random_self_graphs()]):
        kinds, differ = set(), 0
        for g in graphs:
            plain, fair = both_modes(g)
            kinds.add(F.outcome(fair))
            differ += disagree(plain, fair)
        assert kinds == {"none", "terminal", "stutter", "lasso"}
        assert differ >= 5


# ---- LiveGraph ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", sorted(live_ref.ANCHORS))
def test_anchor_parameters(params):
    for mode, want in zip(MODES, both_modes(live_ref.live_graph(*params))):
        got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, LiveGraph(*params).params(), fairness=mode)
        assert got["unique"] == want["unique"]
        assert_matches(got, want, (params, mode))


@pytest.mark.parametrize("params", sorted(F_ANCHORS))
def test_fixpoint_sizes_of_the_two_modes(params):
    plain, fair = both_modes(live_ref.live_graph(*params))
    assert (plain["surviving"], fair["surviving"]) == F_ANCHORS[params]
    assert (plain["witness"] and plain["witness"]["actions"]) == (fair["witness"] and fair["witness"]["actions"])
    for mode, want in zip(MODES, (plain, fair)):
        assert_matches(N.liveness_host(N.SR_MODEL_LIVE_GRAPH, list(params), fairness=mode), want, (params, mode))


def test_a_graph_that_only_stuttering_kept_alive():
    params = (6, 2, 5, 3, 0, 1)
    plain, fair = both_modes(live_ref.live_graph(*params))
    assert (plain["unique"], plain["not_p_states"], plain["surviving"], fair["surviving"]) == (49, 33, 19, 0)
    assert plain["witness"] is None and fair["witness"] is None
    for mode, want in zip(MODES, (plain, fair)):
        assert_matches(N.liveness_host(N.SR_MODEL_LIVE_GRAPH, list(params), fairness=mode), want, mode)


def test_a_stutter_only_state():
    graph = live_ref.live_graph(*STUTTER_ONLY)
    assert F.sinks(graph[0]) == ([], [2])
    plain, fair = both_modes(graph)
    for mode, want in zip(MODES, (plain, fair)):
        assert_matches(N.liveness_host(N.SR_MODEL_LIVE_GRAPH, list(STUTTER_ONLY), fairness=mode), want, mode)
    # init state 2 alone: the plain mode loops on it, progress fairness ends there
    one = ({2: graph[0][2]}, [2], graph[2])
    assert F.check(*one)["witness"]["states"] == [2, 2]
    assert F.check(*one, skip_self=True)["witness"] == {"init_index": 0, "states": [2], "actions": [], "loop_start": -1,
                                                        "end_kind": F.END_STUTTER}


def test_random_live_graphs():
    for params in random_live_graphs():
        for mode, want in zip(MODES, both_modes(live_ref.live_graph(*params))):
            got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, list(params), fairness=mode)
            assert got["unique"] == want["unique"], params
            assert_matches(got, want, (params, mode))


@pytest.mark.parametrize("words", [2, 4])
def test_wide_states_compare_every_word(words):
    for params in [(12, 2, 3, 2, 0, 1), (10, 4, 11, 4, 0, 1), (6, 2, 5, 3, 0, 1), STUTTER_ONLY]:
        for mode, want in zip(MODES, both_modes(live_ref.live_graph(*params))):
            got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, LiveGraph(*params, words=words).params(), fairness=mode)
            assert_matches(got, want, (params, words, mode))


# ---- DGraph: self-edges are kept ------------------------------------------------------------------------

def dgraph_host(paths, mode):
    return N.liveness_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, paths), fairness=mode)


def dgraph_states(paths, got):
    return [sorted({p[0] for p in paths})[got["init_index"]]] + got["actions"]


def test_the_engines_dgraph_keeps_self_edges():
    succ, inits, _ = N.host_graph(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, [[0, 2, 2]]))
    assert (inits, succ) == ([0], [[(2, 1)], [(2, 1)]])  # state number 1 is node 2, its own successor


def test_hand_cases():
    paths = [[0, 2, 2]]
    got = dgraph_host(paths, 0)
    assert dgraph_states(paths, got) == [0, 2, 2] and (got["loop_start"], got["end_kind"]) == (1, 2)
    got = dgraph_host(paths, 1)
    assert dgraph_states(paths, got) == [0, 2] and (got["loop_start"], got["end_kind"]) == (-1, 3)
    paths = [[0, 2, 2], [2, 1]]  # 2 can leave for 1, where "odd" holds
    assert dgraph_host(paths, 0)["init_index"] == 0 and dgraph_host(paths, 0)["witness_len"] == 2
    got = dgraph_host(paths, 1)
    assert (got["init_index"], got["witness_len"], got["surviving"], got["end_kind"]) == (-1, -1, 0, 0)
    for mode in MODES:  # a cycle through two distinct states refutes the property in both modes
        got = dgraph_host(FIXME_CYCLE, mode)
        assert dgraph_states(FIXME_CYCLE, got) == [0, 2, 4, 2] and (got["loop_start"], got["end_kind"]) == (1, 2)
    for paths in ([[0, 2, 2]], [[0, 2, 2], [2, 1]], FIXME_CYCLE):
        for mode, want in zip(MODES, both_modes(live_ref.dgraph(paths))):
            assert_matches(dgraph_host(paths, mode), want, (paths, mode))


def test_random_dgraphs_with_self_edges():
    for paths in random_self_graphs():
        for mode, want in zip(MODES, both_modes(live_ref.dgraph(paths))):
            got = dgraph_host(paths, mode)
            assert got["unique"] == want["unique"], paths
            assert_matches(got, want, (paths, mode))
            if want["witness"] is not None:
                assert dgraph_states(paths, got) == want["witness"]["states"], (paths, mode)


# ---- ping-pong through its host graph ------------------------------------------------------------------

@pytest.mark.parametrize("duplicating", [False, True])
@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("max_nat", [1, 3, 5])
def test_ping_pong_matches_the_fixpoint_over_its_host_graph(max_nat, lossy, duplicating):
    params = PingPong(max_nat, lossy=lossy, duplicating=duplicating).params()
    succ_l, inits, conds = N.host_graph(N.SR_MODEL_PINGPONG, params)
    succ = dict(enumerate(succ_l))
    for p in PINGPONG_EVENTUALLY:
        for mode, want in zip(MODES, both_modes((succ, inits, lambda s: conds[s] >> p & 1))):
            got = N.liveness_host(N.SR_MODEL_PINGPONG, params, prop=p, fairness=mode)
            assert got["unique"] == len(succ)
            assert_matches(got, want, (params, p, mode))


# ---- 2pc with `eventually` properties -------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_two_phase_live(n):
    succ, inits = F.two_phase(n)
    params = TwoPhaseLiveSys(n).params()
    # the restatement is the engine's graph: same states, same (action id, successor) lists in slot order
    succ_l, _, conds = N.host_graph(N.SR_MODEL_2PC_LIVE, params)
    assert len(succ_l) == len(succ) == {1: 12, 2: 56, 3: 288, 4: 1568, 5: 8832}[n]
    assert sorted(len(v) for v in succ_l) == sorted(len(v) for v in succ.values())
    assert sum(len(v) for v in succ_l) + 1 == {1: 20, 2: 154, 3: 1146, 4: 8258, 5: 58146}[n]
    terminal, stutter = F.sinks(succ)
    assert terminal == [] and len(stutter) == STUTTER_ENDS.get(n, len(stutter))
    assert sum(1 for i, v in enumerate(succ_l) if v and all(t == i for _, t in v)) == len(stutter)
    for p, (name, cond) in F.TWO_PHASE_LIVE_PROPS.items():
        assert sum(1 for c in conds if not c >> p & 1) == sum(1 for s in succ if not cond(s))
        for mode, want in zip(MODES, both_modes((succ, inits, cond))):
            got = N.liveness_host(N.SR_MODEL_2PC_LIVE, params, prop=p, fairness=mode)
            assert got["unique"] == len(succ)
            assert_matches(got, want, (n, name, mode))  # (2pc's action id is the slot)
    decides = [N.liveness_host(N.SR_MODEL_2PC_LIVE, params, prop=3, fairness=m) for m in MODES]
    if n in DECIDES_PLAIN:
        assert (decides[0]["not_p_states"], decides[0]["surviving"]) == DECIDES_PLAIN[n]
    assert decides[0]["init_index"] == 0  # refuted by stuttering
    assert (decides[1]["surviving"], decides[1]["init_index"], decides[1]["end_kind"]) == (0, -1, 0)  # holds
    commits = [N.liveness_host(N.SR_MODEL_2PC_LIVE, params, prop=4, fairness=m) for m in MODES]
    assert (commits[0]["actions"], commits[0]["loop_start"], commits[0]["end_kind"]) == ([1, 3, 6, 6], 3, 2)
    assert (commits[1]["not_p_states"], commits[1]["surviving"], commits[1]["actions"]) == COMMITS_PROGRESS[n]
    assert (commits[1]["loop_start"], commits[1]["end_kind"]) == (-1, 3)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_models_self_loop_hook_and_the_state_compare_agree(n, monkeypatch):
    """2pc's `enabled_moves` names its self-loops exactly, so the rule takes its slot mask and compares no
    state; SR_LIVE_MOVES=0 makes it compare the words, as it does for every other model."""
    params = TwoPhaseLiveSys(n).params()
    for p in (3, 4):
        monkeypatch.delenv("SR_LIVE_MOVES", raising=False)
        mask = N.liveness_host(N.SR_MODEL_2PC_LIVE, params, prop=p, fairness=1)
        monkeypatch.setenv("SR_LIVE_MOVES", "0")
        compare = N.liveness_host(N.SR_MODEL_2PC_LIVE, params, prop=p, fairness=1)
        for k in ("not_p_states", "surviving", "init_index", "witness_len", "loop_start", "end_kind", "actions", "unique"):
            assert mask[k] == compare[k], (n, p, k)


def test_two_phase_live_validates_like_two_phase():
    for bad in ([], [0], [15]):
        with pytest.raises(ValueError):
            N.liveness_host(N.SR_MODEL_2PC_LIVE, bad, prop=3)
    with pytest.raises(ValueError, match="not an `eventually` property"):
        N.liveness_host(N.SR_MODEL_2PC_LIVE, [3], prop=2)
    p = (N.ctypes.c_int64 * 1)(3)
    assert N.load().sr_selftest_describe(N.SR_MODEL_2PC_LIVE, p, 1, 1 << 20) == 288, N.last_error()


# ---- the ABI -------------------------------------------------------------------------------------------

def test_the_result_struct_kept_its_layout():
    r = N.sr_live_result
    assert N.ctypes.sizeof(r) == 64
    assert [(n, getattr(r, n).offset) for n, _ in r._fields_] == [
        ("ran", 0), ("init_index", 4), ("not_p_states", 8), ("surviving", 16), ("examined", 24), ("rounds", 32),
        ("end_kind", 36), ("witness_len", 40), ("loop_start", 48), ("pass_ms", 56)]
    assert (N.SR_LIVENESS_COMPLETE, N.SR_LIVENESS_PROGRESS, N.SR_MODEL_2PC_LIVE) == (1, 2, 16)


def test_the_old_entry_is_the_new_one_without_fairness():
    lib = N.load()
    cases = [(N.SR_MODEL_LIVE_GRAPH, [12, 2, 3, 2, 0, 1], 0), (N.SR_MODEL_LIVE_GRAPH, [12, 2, 1, 3, 16, 1], 0),
             (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, [[0, 2, 2]]), 0), (N.SR_MODEL_2PC_LIVE, [3], 4)]
    for model, params, prop in cases:
        arr = (N.ctypes.c_int64 * len(params))(*params)
        old, new = N.sr_live_result(), N.sr_live_result()
        a_old, a_new = (N.ctypes.c_int64 * 64)(), (N.ctypes.c_int64 * 64)()
        n_old = lib.sr_liveness_host(model, arr, len(params), prop, 1 << 20, N.ctypes.byref(old), a_old, 64)
        n_new = lib.sr_liveness_host_fair(model, arr, len(params), prop, 0, 1 << 20, N.ctypes.byref(new), a_new, 64)
        assert n_old == n_new > 0
        for name, _ in N.sr_live_result._fields_:
            if name != "pass_ms":
                assert getattr(old, name) == getattr(new, name), (model, name)
        assert list(a_old) == list(a_new)
        assert old.end_kind == (0 if old.witness_len < 0 else 2 if old.loop_start >= 0 else 1)  # filled in the plain mode too
    with pytest.raises(ValueError, match="fairness must be 0"):
        N.liveness_host(N.SR_MODEL_LIVE_GRAPH, [8, 2, 1, 3, 0, 1], fairness=2)


def test_the_builder_option():
    from stateright_amd import TwoPhaseLiveSys as Sys
    b = Sys(3).checker()
    assert b.complete_liveness()._opts.liveness == 1
    assert b.complete_liveness(fairness="progress")._opts.liveness == 2
    assert b.complete_liveness(False, fairness="progress")._opts.liveness == 0
    assert b.complete_liveness(True)._opts.liveness == 1
    for bad in ("nonsense", "weak", 2, True, ""):
        with pytest.raises(ValueError, match="fairness"):
            b.complete_liveness(fairness=bad)
    assert b._opts.liveness == 1  # a refused call changes nothing
