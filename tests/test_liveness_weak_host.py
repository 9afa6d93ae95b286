"""Weak fairness of the complete `eventually` check on the host (sr_liveness_host_weak, csrc/live.hpp
live_host_weak), checked without a device against the independent Python restatement in
tests/live_weak_ref.py: every unique figure (|N_p|, |F_p'|, the cyclic states, the components and the fair
ones, the goal set, FairF, the first init state), the stem action by action, how the witness ends, and the
validity of the closed walk (closed, inside N_p and its component, no self step, weakly fair), on the
issue's anchors (DGraph, LiveGraph, SpinLock, 2pc-live), SpinLock(1..4, 10), LiveGraph on 2 and 4 words
and random draws.

Not compared: `rounds`, `examined` (the sum of the worklist sizes over those rounds: states leave in place,
so both depend on the order) and the three round counters of sr_live_weak, which are implementation
details, and the wall times."""
import pytest

import live_fair_ref as LF
import live_weak_ref as LW
from oracle_lib import dgraph_params
from stateright_amd import _native as N
from stateright_amd.models import DGraph, LiveGraph, PingPong, SpinLockSys, TwoPhaseLiveSys
from test_liveness_fair_host import random_live_graphs, random_self_graphs

WEAK_KEYS = ("cyclic_states", "components", "fair_components", "goal_states", "fair_states")

_CHECKED = {}


def model_of(case, words=1):
    if case[0] == "dgraph":
        return DGraph(N.SR_EVENTUALLY, [list(p) for p in case[1]])
    if case[0] == "live":
        return LiveGraph(*case[1], words=words)
    if case[0] == "spin":
        return SpinLockSys(case[1])
    return TwoPhaseLiveSys(case[1])


def prop_of(case):
    return case[2] if case[0] in ("spin", "2pc") else 0


def params_of(case, words=1):
    if case[0] == "dgraph":
        return dgraph_params(N.SR_EVENTUALLY, [list(p) for p in case[1]])
    return model_of(case, words).params()


def reference(case):
    """(graph, live_weak_ref.check of it), computed once per case and shared."""
    if case not in _CHECKED:
        graph = LW.graph_of(case)
        _CHECKED[case] = (graph, LW.check(*graph))
    return _CHECKED[case]


def assert_weak_matches(got, graph, want, what):
    """got: liveness_host_weak()'s dict (or a device result in the same form); want: live_weak_ref.check()."""
    succ, inits, cond, nslots = graph
    w = got["weak"]
    assert got["ran"] == 1 and w["ran"] == 1, what
    if "unique" in got:
        assert got["unique"] == want["unique"], what
    assert (got["not_p_states"], got["surviving"]) == (want["not_p_states"], want["surviving"]), what
    assert {k: w[k] for k in WEAK_KEYS} == {k: want[k] for k in WEAK_KEYS}, what
    assert got["init_index"] == want["init_index"], what
    if want["init_index"] < 0:
        assert (got["witness_len"], got["loop_start"], got["end_kind"], got["actions"]) == (-1, -1, 0, []), what
        assert (w["stem_len"], w["loop_len"]) == (-1, -1), what
        return
    stem = want["stem"]
    assert w["stem_len"] == len(stem) and got["actions"][:len(stem)] == stem, what
    assert got["end_kind"] == want["end_kind"], what
    assert got["witness_len"] == w["stem_len"] + w["loop_len"] == len(got["actions"]), what
    if want["end_kind"] == LF.END_LOOP:
        assert got["loop_start"] == w["stem_len"] and w["loop_len"] >= 2, what
        assert w["segments"] >= 1 and w["segments"] <= nslots + 1, what
        loop = got["actions"][len(stem):]
        assert LW.loop_problems(succ, cond, nslots, want["stem_states"][-1], loop, inside=want["comp"]) == [], what
    else:
        assert (got["loop_start"], w["loop_len"], w["segments"]) == (-1, 0, 0), what


# ---- the restatement reproduces the issue's anchors ------------------------------------------------------

@pytest.mark.parametrize("case", list(LW.ANCHORS), ids=[repr(c) for c in LW.ANCHORS])
def test_the_restatement_reproduces_the_anchors(case):
    _, want = reference(case)
    anchor = LW.ANCHORS[case]
    for key, figure in zip(LW.ANCHOR_KEYS, anchor):
        if figure is not None:
            assert want[key] == figure, (case, key)
    if anchor[8] is not None:
        assert len(want["stem"]) == anchor[8], case
    if anchor[9] is not None:
        assert want["end_kind"] == anchor[9], case
    elif want["init_index"] >= 0:
        assert want["end_kind"] == LF.END_LOOP, case  # "refuted, stem k" into a fair component


def test_what_spin_lock_shows():
    """ "some thread served": the plain and the progress mode refute it by the Tick cycle, weak fairness does
    not; "every thread served" stays refuted, by a starvation lasso."""
    succ, inits = LW.spin_lock(3)
    for skip_self in (False, True):
        w = LF.check(succ, inits, LW.some_served, skip_self)["witness"]
        assert w is not None and w["end_kind"] == LF.END_LOOP and w["actions"][w["loop_start"]:] == [6, 6]
    for fairness in (0, 1):
        got = N.liveness_host(N.SR_MODEL_SPIN_LOCK, [3], prop=0, fairness=fairness)
        assert (got["init_index"], got["end_kind"], got["actions"][got["loop_start"]:]) == (0, LF.END_LOOP, [6, 6])
    assert N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [3], prop=0)["init_index"] == -1
    got = N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [3], prop=1)
    assert (got["init_index"], got["end_kind"]) == (0, LF.END_LOOP)
    assert {3, 4, 5} - set(got["actions"])  # some thread never releases: it starves while another is served


# ---- the host form against the restatement ---------------------------------------------------------------

@pytest.mark.parametrize("case", list(LW.ANCHORS), ids=[repr(c) for c in LW.ANCHORS])
def test_host_form_on_the_anchors(case):
    graph, want = reference(case)
    got = N.liveness_host_weak(model_of(case).MODEL_ID, params_of(case), prop=prop_of(case))
    assert_weak_matches(got, graph, want, case)


def test_host_form_ends_at_a_terminal_state_the_search_does_not_flag():
    graph, want = reference(LW.LATE_TERMINAL)
    assert (want["stem"], want["end_kind"], want["components"]) == ([2, 4, 8, 6], LF.END_TERMINAL, 0)
    got = N.liveness_host_weak(N.SR_MODEL_DGRAPH, params_of(LW.LATE_TERMINAL), prop=0)
    assert_weak_matches(got, graph, want, LW.LATE_TERMINAL)


def test_host_form_with_duplicate_roots():
    graph = LW.dup_roots_graph()
    want = LW.check(*graph)
    plain = reference(("live", LW.DUP_ROOTS[0]))[1]
    assert len(graph[1]) == 80 and want["init_index"] == 10
    assert {k: v for k, v in want.items() if k != "comp"} == {k: v for k, v in plain.items() if k != "comp"}
    got = N.liveness_host_weak(N.SR_MODEL_LIVE_GRAPH, list(LW.DUP_ROOTS[0]) + [1, LW.DUP_ROOTS[1]], prop=0)
    assert_weak_matches(got, graph, want, LW.DUP_ROOTS)
    with pytest.raises(ValueError, match="dup"):
        N.liveness_host_weak(N.SR_MODEL_LIVE_GRAPH, [4, 2, 1, 2, 0, 3, 1, 4], prop=0)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("prop", [0, 1])
def test_host_form_on_spin_lock(n, prop):
    case = ("spin", n, prop)
    graph, want = reference(case)
    assert want["unique"] == (n + 1) * 2 ** n * 2
    assert_weak_matches(N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [n], prop=prop), graph, want, case)


def test_host_form_on_spin_lock_10_some():
    case = ("spin", 10, 0)
    graph, want = reference(case)
    assert want["init_index"] == -1  # holds
    assert_weak_matches(N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [10], prop=0), graph, want, case)


@pytest.mark.parametrize("words", [2, 4])
@pytest.mark.parametrize("params", [(12, 2, 26, 2, 0, 1), (12, 2, 1, 3, 16, 1), (8, 3, 26, 2, 0, 1)])
def test_host_form_on_wide_states(params, words):
    case = ("live", params)
    graph, want = reference(case)
    got = N.liveness_host_weak(N.SR_MODEL_LIVE_GRAPH, params_of(case, words), prop=0)
    assert_weak_matches(got, graph, want, (case, words))


def test_host_form_on_random_live_graphs():
    kinds = set()
    for params in random_live_graphs(30):
        case = ("live", params)
        graph = LW.graph_of(case)
        want = LW.check(*graph)
        kinds.add(want["end_kind"])
        assert_weak_matches(N.liveness_host_weak(N.SR_MODEL_LIVE_GRAPH, list(params), prop=0), graph, want, case)
    assert {LF.END_NONE, LF.END_LOOP} <= kinds


def test_host_form_on_random_dgraphs():
    kinds = set()
    for paths in random_self_graphs(60):
        case = ("dgraph", tuple(tuple(p) for p in paths))
        graph = LW.graph_of(case)
        want = LW.check(*graph)
        kinds.add(want["end_kind"])
        assert_weak_matches(N.liveness_host_weak(N.SR_MODEL_DGRAPH, params_of(case), prop=0), graph, want, case)
    assert {LF.END_NONE, LF.END_TERMINAL, LF.END_STUTTER, LF.END_LOOP} <= kinds


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("prop", [3, 4])
def test_two_phase_with_and_without_the_moves_hook(n, prop, monkeypatch):
    case = ("2pc", n, prop)
    graph, want = reference(case)
    with_hook = N.liveness_host_weak(N.SR_MODEL_2PC_LIVE, [n], prop=prop)
    assert_weak_matches(with_hook, graph, want, case)
    monkeypatch.setenv("SR_LIVE_MOVES", "0")  # compare the states instead of asking `enabled_moves`
    compared = N.liveness_host_weak(N.SR_MODEL_2PC_LIVE, [n], prop=prop)
    assert_weak_matches(compared, graph, want, case)
    drop = ("pass_ms", "rounds", "examined", "weak")
    assert {k: v for k, v in with_hook.items() if k not in drop} == {k: v for k, v in compared.items() if k not in drop}
    assert {k: with_hook["weak"][k] for k in WEAK_KEYS} == {k: compared["weak"][k] for k in WEAK_KEYS}


# ---- refusals, the ABI, the builder ------------------------------------------------------------------------

def test_a_model_whose_slots_are_no_fairness_classes_is_unsupported():
    with pytest.raises(ValueError, match=r"slots are not fairness classes.*status -4"):
        N.liveness_host_weak(N.SR_MODEL_PINGPONG, PingPong(2).params(), prop=0)


def test_the_progress_entry_point_still_refuses_two():
    with pytest.raises(ValueError):
        N.liveness_host(N.SR_MODEL_SPIN_LOCK, [2], prop=0, fairness=2)


def test_not_an_eventually_property_and_bad_parameters():
    with pytest.raises(ValueError, match="eventually"):
        N.liveness_host_weak(N.SR_MODEL_2PC_LIVE, [2], prop=0)
    with pytest.raises(ValueError):
        N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [21], prop=0)
    with pytest.raises(ValueError):
        SpinLockSys(0)
    with pytest.raises(ValueError, match="max_states"):
        N.liveness_host_weak(N.SR_MODEL_SPIN_LOCK, [4], prop=0, max_states=100)


def test_the_struct_and_the_mode_value():
    import ctypes
    assert N.SR_LIVENESS_WEAK == 3 and N.SR_MODEL_SPIN_LOCK == 17
    assert ctypes.sizeof(N.sr_live_weak) == 88
    assert ctypes.sizeof(N.sr_live_result) == 64 and ctypes.sizeof(N.sr_opts) == 72  # (64 + the certificate pass' option)


def test_the_builder_sets_and_clears_the_mode():
    b = SpinLockSys(2).checker()
    assert b._opts.liveness == 0
    assert b.weak_fairness()._opts.liveness == 3
    assert b.weak_fairness(False)._opts.liveness == 0
    assert b.complete_liveness(fairness="progress")._opts.liveness == 2
    assert b.weak_fairness(on=True)._opts.liveness == 3
    with pytest.raises(ValueError):
        b.complete_liveness(fairness="weak")
