"""Strong fairness of the complete `eventually` check on the host (sr_liveness_host_strong, csrc/live.hpp
live_host_strong), checked without a device against the independent Python restatement in
tests/live_strong_ref.py: every unique figure (|N_p|, |F_p'|, the cyclic states, the tree's depth, its nodes
and fair nodes, the goal set, FairF, the first init state), the stem action by action, how the witness ends,
and the validity of the closed walk (closed, inside N_p and its fair node, no self step, strongly fair). The
restatement itself is checked first: against the issue's anchors, FairRings' closed forms, and a brute-force
enumeration of the strongly fair subsets on graphs small enough for it.

Not compared: `rounds`, `examined` and the three round counters of sr_live_strong (implementation details)
and the wall times."""
import ctypes
import random

import pytest

import live_fair_ref as LF
import live_strong_ref as LS
import live_weak_ref as LW
from stateright_amd import _native as N
from stateright_amd.models import FairRings, Paxos, PingPong, SpinLockSys
from test_liveness_weak_host import model_of as weak_model_of, params_of as weak_params_of, prop_of as weak_prop_of

STRONG_KEYS = LS.STRONG_KEYS

_CHECKED = {}


def model_of(case, words=1):
    return FairRings(*case[1]) if case[0] == "rings" else weak_model_of(case, words)


def params_of(case, words=1):
    return list(case[1]) if case[0] == "rings" else weak_params_of(case, words)


def prop_of(case):
    return 0 if case[0] == "rings" else weak_prop_of(case)


def reference(case):
    """(graph, live_strong_ref.check of it), computed once per case and shared."""
    if case not in _CHECKED:
        graph = LS.graph_of(case)
        _CHECKED[case] = (graph, LS.check(*graph))
    return _CHECKED[case]


def assert_strong_matches(got, graph, want, what):
    """got: liveness_host_strong()'s dict (or a device result in the same form); want: live_strong_ref.check()."""
    succ, inits, cond, nslots = graph
    g = got["strong"]
    assert "weak" not in got, what
    assert got["ran"] == 1 and g["ran"] == 1, what
    if "unique" in got:
        assert got["unique"] == want["unique"], what
    assert (got["not_p_states"], got["surviving"]) == (want["not_p_states"], want["surviving"]), what
    assert {k: g[k] for k in STRONG_KEYS} == {k: want[k] for k in STRONG_KEYS}, what
    assert got["init_index"] == want["init_index"], what
    if want["init_index"] < 0:
        assert (got["witness_len"], got["loop_start"], got["end_kind"], got["actions"]) == (-1, -1, 0, []), what
        assert (g["stem_len"], g["loop_len"]) == (-1, -1), what
        return
    stem = want["stem"]
    assert g["stem_len"] == len(stem) and got["actions"][:len(stem)] == stem, what
    assert got["end_kind"] == want["end_kind"], what
    assert got["witness_len"] == g["stem_len"] + g["loop_len"] == len(got["actions"]), what
    if want["end_kind"] == LF.END_LOOP:
        assert got["loop_start"] == g["stem_len"] and g["loop_len"] >= 2, what
        assert 1 <= g["segments"] <= nslots + 1, what
        loop = got["actions"][len(stem):]
        assert LS.loop_problems(succ, cond, nslots, want["stem_states"][-1], loop, inside=want["node"]) == [], what
    else:
        assert (got["loop_start"], g["loop_len"], g["segments"]) == (-1, 0, 0), what


def host(case, words=1):
    return N.liveness_host_strong(model_of(case, words).MODEL_ID, params_of(case, words), prop=prop_of(case))


# ---- the restatement: the anchors, the closed forms, the definition ------------------------------------

@pytest.mark.parametrize("case", list(LS.ANCHORS), ids=[repr(c) for c in LS.ANCHORS])
def test_the_restatement_reproduces_the_anchors(case):
    _, want = reference(case)
    anchor = LS.ANCHORS[case]
    assert tuple(want[k] for k in LS.ANCHOR_KEYS) == anchor[:8], case
    assert want["not_p_states"] == want["surviving"] or case[0] != "rings", case
    if anchor[8] is not None:
        assert len(want["stem"]) == anchor[8], case
    assert want["end_kind"] == anchor[9], case
    if case in LS.WITNESSES:
        assert want["stem"] == LS.WITNESSES[case][0], case


def test_weak_fairness_refutes_what_strong_fairness_protects():
    """The contrast the mode exists for: SpinLock's "every thread served" is refuted from init 0 under weak
    fairness (a starvation lasso) and holds under strong fairness."""
    for n in (3, 10):
        case = ("spin", n, 1)
        assert LW.check(*LW.graph_of(case))["init_index"] == 0
        assert reference(case)[1]["init_index"] == -1


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("core", [0, 1, 2])
@pytest.mark.parametrize("lanes", [1, 2, 5])
def test_the_restatement_on_fair_rings_closed_forms(d, w, core, lanes):
    graph = LS.fair_rings(d, w, core, lanes)
    want = LS.check(*graph)
    forms = LS.fair_rings_closed_forms(d, w, core, lanes)
    assert {k: want[k] for k in forms} == forms
    weak = LW.check(*graph)  # every lane is one weakly fair component
    assert (weak["components"], weak["fair_components"], weak["init_index"]) == (lanes, lanes, 0)


def tiny_random_graphs(count, seed=20261021):
    """(succ, inits, cond, nslots): up to 10 states, up to 4 slots, slot-labelled edges, self steps included."""
    rng = random.Random(seed)
    for _ in range(count):
        n, nslots = rng.randint(2, 10), rng.randint(1, 4)
        density = rng.choice((0.3, 0.5, 0.8))
        succ = {s: [(a, rng.randrange(n)) for a in range(nslots) if rng.random() < density] for s in range(n)}
        marked = {s for s in range(n) if rng.random() < 0.2}
        yield succ, [0], (lambda s, marked=marked: s in marked), nslots


@pytest.mark.parametrize("case", LS.STARRED, ids=[repr(c) for c in LS.STARRED])
def test_brute_force_agrees_on_the_starred_rows(case):
    (succ, _, cond, _), _ = reference(case)
    _, f = LF.fixpoint(succ, cond, skip_self=True)
    assert LS.brute_force_fair_states(succ, f) == LS.fair_node_states(succ, f)


def tiny_nested_graphs(count, seed=20261022):
    """Random draws hardly ever nest, so these are planted: an inner cycle 0 .. k-1 by slot 0; a state o that
    slot 1 reaches from inside and that returns by slot 0, so that the cycle and o are one component; slot 2,
    which only o moves on, leaves it; in half of the draws slot 1 also stays inside the inner cycle (which is
    then a fair node inside an unfair component); then every state gets a few random edges."""
    rng = random.Random(seed)
    for _ in range(count):
        k = rng.randint(2, 4)
        o, z, n, nslots = k, k + 1, k + 2 + rng.randint(0, 3), rng.randint(3, 5)
        edges = {s: {} for s in range(n)}
        for s in range(k):
            edges[s][0] = (s + 1) % k
        edges[1][1], edges[o][0], edges[o][2] = o, 0, z
        if rng.random() < 0.5:
            edges[0][1] = 1
        for s in range(n):
            for a in range(nslots):
                if a not in edges[s] and rng.random() < 0.1:
                    edges[s][a] = rng.randrange(n)
        marked = {s for s in range(k + 1, n) if rng.random() < 0.3}
        yield {s: sorted(edges[s].items()) for s in range(n)}, [0], (lambda s, marked=marked: s in marked), nslots


def test_brute_force_agrees_on_random_tiny_graphs():
    nested = fair = 0
    for succ, inits, cond, nslots in list(tiny_random_graphs(300)) + list(tiny_nested_graphs(150)):
        _, f = LF.fixpoint(succ, cond, skip_self=True)
        nodes = LS.tree(succ, f)
        assert LS.brute_force_fair_states(succ, f) == LS.fair_node_states(succ, f), succ
        nested += any(d > 1 and ok for d, _, ok in nodes)
        fair += any(ok for _, _, ok in nodes)
    assert nested >= 10 and fair >= 30  # (the draw does hold fair nodes inside unfair components)


def test_the_flat_graphs_equal_the_weak_mode():
    """None of these graphs nests: the strong mode's figures are the weak mode's, with at most one level."""
    for case in LS.FLAT:
        graph = LW.graph_of(case)
        strong, weak = LS.check(*graph), LW.check(*graph)
        for key in ("cyclic_states", "components", "fair_components", "goal_states", "fair_states", "init_index", "stem", "end_kind"):
            assert strong[key] == weak[key], (case, key)
        assert strong["levels"] <= 1, case


# ---- the host form against the restatement ---------------------------------------------------------------

ALL_ANCHORS = list(LS.ANCHORS) + LS.FLAT


@pytest.mark.parametrize("case", ALL_ANCHORS, ids=[repr(c) for c in ALL_ANCHORS])
def test_host_form_on_the_anchors(case):
    graph, want = reference(case)
    got = host(case)
    assert_strong_matches(got, graph, want, case)
    if case in LS.WITNESSES:
        stem, loop = LS.WITNESSES[case]
        assert got["actions"] == stem + loop, case


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("prop", [0, 1])
def test_host_form_on_spin_lock(n, prop):
    case = ("spin", n, prop)
    graph, want = reference(case)
    assert want["init_index"] == -1 and want["fair_components"] == 0  # both properties hold under strong fairness
    assert_strong_matches(host(case), graph, want, case)


def test_host_form_on_spin_lock_10_some():
    case = ("spin", 10, 0)
    graph, want = reference(case)
    assert_strong_matches(host(case), graph, want, case)


@pytest.mark.parametrize("words", [2, 4])
@pytest.mark.parametrize("params", [(12, 2, 26, 2, 0, 1), (12, 2, 1, 3, 16, 1), (8, 3, 26, 2, 0, 1)])
def test_host_form_on_wide_states(params, words):
    case = ("live", params)
    graph, want = reference(case)
    assert_strong_matches(host(case, words), graph, want, (case, words))


def test_host_form_with_duplicate_roots():
    graph = LW.dup_roots_graph()
    want = LS.check(*graph)
    assert len(graph[1]) == 80 and want["init_index"] == 10
    got = N.liveness_host_strong(N.SR_MODEL_LIVE_GRAPH, list(LW.DUP_ROOTS[0]) + [1, LW.DUP_ROOTS[1]], prop=0)
    assert_strong_matches(got, graph, want, LW.DUP_ROOTS)


def test_host_form_ends_at_a_terminal_state_the_search_does_not_flag():
    graph, want = reference(LW.LATE_TERMINAL)
    assert (want["stem"], want["end_kind"], want["components"], want["levels"]) == ([2, 4, 8, 6], LF.END_TERMINAL, 0, 0)
    assert_strong_matches(host(LW.LATE_TERMINAL), graph, want, LW.LATE_TERMINAL)


@pytest.mark.parametrize("params", [(1, 4, 2, 3), (3, 5, 1, 4), (3, 4, 2, 7), (5, 7, 2, 12)])
def test_host_form_on_fair_rings(params):
    case = ("rings", params)
    graph, want = reference(case)
    forms = LS.fair_rings_closed_forms(*params)
    assert {k: want[k] for k in forms} == forms
    assert_strong_matches(host(case), graph, want, case)


def test_host_form_with_and_without_the_moves_hook(monkeypatch):
    case = ("2pc", 3, 4)
    graph, want = reference(case)
    with_hook = host(case)
    monkeypatch.setenv("SR_LIVE_MOVES", "0")  # compare the states instead of asking `enabled_moves`
    compared = host(case)
    assert_strong_matches(with_hook, graph, want, case)
    assert_strong_matches(compared, graph, want, case)
    assert with_hook["actions"] == compared["actions"]


# ---- refusals, the ABI, the builder ------------------------------------------------------------------------

def test_models_whose_slots_are_no_fairness_classes_are_unsupported():
    with pytest.raises(ValueError, match=r"slots are not fairness classes.*status -4"):
        N.liveness_host_strong(N.SR_MODEL_PINGPONG, PingPong(2).params(), prop=0)
    with pytest.raises(ValueError, match=r"slots are not fairness classes.*status -4"):
        N.liveness_host_strong(N.SR_MODEL_PAXOS, Paxos(1).params(), prop=0)


def test_not_an_eventually_property_and_bad_parameters():
    with pytest.raises(ValueError, match="eventually"):
        N.liveness_host_strong(N.SR_MODEL_2PC_LIVE, [2], prop=0)
    for params in ([0, 4, 0, 1], [29, 4, 0, 1], [1, 3, 0, 1], [1, 65, 0, 1], [1, 4, 3, 1], [1, 4, 0, 0], [1, 4, 0, 513], [1, 4, 0]):
        with pytest.raises(ValueError):
            N.liveness_host_strong(N.SR_MODEL_FAIR_RINGS, params, prop=0)
    with pytest.raises(ValueError):
        FairRings(1, 3, 0, 1)
    with pytest.raises(ValueError, match="max_states"):
        N.liveness_host_strong(N.SR_MODEL_FAIR_RINGS, [2, 8, 1, 4], prop=0, max_states=20)


def test_the_struct_and_the_mode_value():
    assert N.SR_LIVENESS_STRONG == 4 and N.SR_MODEL_FAIR_RINGS == 18
    s = N.sr_live_strong
    assert ctypes.sizeof(s) == 88
    offsets = {name: getattr(s, name).offset for name, _ in s._fields_}
    assert offsets == {"ran": 0, "levels": 4, "cyclic_states": 8, "components": 16, "fair_components": 24, "goal_states": 32,
                       "fair_states": 40, "stem_len": 48, "loop_len": 56, "scc_rounds": 64, "reach_rounds": 68, "segments": 72,
                       "reserved1": 76, "pass_ms": 80}
    assert ctypes.sizeof(N.sr_live_weak) == 88  # unchanged
    assert ctypes.sizeof(N.sr_live_result) == 64 and ctypes.sizeof(N.sr_opts) == 72


def test_the_builder_sets_and_clears_the_mode():
    b = SpinLockSys(2).checker()
    assert b._opts.liveness == 0
    assert b.strong_fairness()._opts.liveness == 4
    assert b.strong_fairness(False)._opts.liveness == 0
    assert b.weak_fairness()._opts.liveness == 3
    assert b.strong_fairness(on=True)._opts.liveness == 4
    assert b.complete_liveness()._opts.liveness == 1


def test_the_mode_values_leave_five_and_up_alone():
    """Only 2, 3 and 4 name fair modes; the values from 5 up stay "read as COMPLETE" (tests/test_gpu_liveness_strong.py
    spawns a check with 7 and finds the plain mode's answer)."""
    assert (N.SR_LIVENESS_OFF, N.SR_LIVENESS_COMPLETE, N.SR_LIVENESS_PROGRESS, N.SR_LIVENESS_WEAK, N.SR_LIVENESS_STRONG) == (0, 1, 2, 3, 4)
    b = SpinLockSys(2).checker().complete_liveness()
    b._opts.liveness = 7
    assert b.strong_fairness(False)._opts.liveness == 0
