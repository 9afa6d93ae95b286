"""The step pass on the host (sr_step_host, csrc/step.hpp), checked without a device against the independent
Python restatement in tests/step_ref.py: the three counts, the seed (depth, source, slot) and the witness along
the FIFO tree, action by action. The restatement itself is checked first against the issue's anchors.

Not compared: the wall times."""
import ctypes

import pytest

import step_ref as S
from stateright_amd import _native as N
from stateright_amd.models import StepDGraph, StepGraph, TwoPhaseStepSys, TwoPhaseSys

_GRAPHS, _CHECKED = {}, {}
TM_ABORT = 1  # 2pc's canonical action id of TmAbort

# Hand-drawn graphs: name -> (forbidden pairs, paths, (edges, violations, sources), witness actions or None, init_index)
HAND = {
    "a violation only on a self-loop": ([(1, 1)], [[0, 1, 1]], (2, 1, 1), [1, 1], 0),
    "a violation only at an init state": ([(0, 1)], [[0, 1, 2]], (2, 1, 1), [1], 0),
    "a violation only on a slot past 64": ([(3, 130)], [[1, 3, 130], [1, 3, 7]], (3, 1, 1), [3, 130], 0),
    # level 1 is found as 5 (from init state 1, visited first) and then 3: the seed's source is 3, the lower state
    "two violating sources of one level": ([(5, 7), (3, 7)], [[0, 3, 7], [1, 5, 7]], (4, 2, 2), [3, 7], 0),
    "a forbidden pair that is no edge": ([(0, 2), (2, 1)], [[0, 1, 2]], (2, 0, 0), None, -1),
}


def graph_of(row, dup=0):
    if (row, dup) not in _GRAPHS:
        _GRAPHS[row, dup] = S.step_graph(*row, dup=dup)
    return _GRAPHS[row, dup]


def reference(row, prop, dup=0):
    """step_ref.check of StepGraph(*row)'s property `prop`, computed once and shared (the GPU tests use it too)."""
    if (row, prop, dup) not in _CHECKED:
        succ, inits, props = graph_of(row, dup)
        _CHECKED[row, prop, dup] = S.check(succ, inits, props[prop])
    return _CHECKED[row, prop, dup]


def assert_step_matches(got, want, what, fifo=True):
    """got: step_host()'s dict, or a device result in the same form (`actions`: the discovery's action ids, []
    without one); want: step_ref.check(). fifo=False (a device run in FAST order): the path to the seed's source
    is the search's own tree path, which is not the FIFO one; everything else is the same."""
    assert got["ran"] == 1, what
    if "unique" in got:
        assert got["unique"] == want["unique"], what
    assert (got["edges"], got["violations"], got["sources"]) == (want["edges"], want["violations"], want["sources"]), what
    if want["seed"] is None:
        assert (got["step_index"], got["step_action"], got["init_index"], got["witness_len"], got["actions"]) == (-1, -1, -1, -1, []), what
        return
    assert got["step_index"] == want["depth"] and got["witness_len"] == want["depth"] + 1 == len(got["actions"]), what
    assert got["step_action"] == got["actions"][-1] == want["actions"][-1], what
    if fifo:
        assert got["actions"] == want["actions"] and got["init_index"] == want["init_index"], what


def host(model, prop):
    return N.step_host(model.MODEL_ID, model.params(), prop)


# ---- the restatement against the issue's anchors ---------------------------------------------------------------

@pytest.mark.parametrize("row", list(S.ANCHORS), ids=[repr(r) for r in S.ANCHORS])
def test_the_restatement_reproduces_the_anchors(row):
    unique, edges, forbidden, down = S.ANCHORS[row]
    for prop, (violations, sources, seed) in enumerate((forbidden, down)):
        want = reference(row, prop)
        assert (want["unique"], want["edges"], want["violations"], want["sources"]) == (unique, edges, violations, sources), (row, prop)
        assert (None if want["seed"] is None else (want["depth"], want["seed"], want["slot"])) == seed, (row, prop)
        if seed is not None:  # the witness: depth + 1 actions that replay, the last through the seed's slot to t
            states = S.replay(graph_of(row)[0], graph_of(row)[1][want["init_index"]], want["actions"])
            assert states == want["states"] and len(want["actions"]) == seed[0] + 1 and states[-2] == seed[1], (row, prop)


# ---- the host form against the restatement -----------------------------------------------------------------------

@pytest.mark.parametrize("row", list(S.ANCHORS), ids=[repr(r) for r in S.ANCHORS])
def test_host_form_equals_the_restatement(row):
    for prop in (0, 1):
        assert_step_matches(host(StepGraph(*row), prop), reference(row, prop), (row, prop))


@pytest.mark.parametrize("words", [2, 4])
@pytest.mark.parametrize("row", [(8, 2, 1, 7, 0, 1), (12, 2, 1, 50, 16, 1), (12, 2, 1, 300, 0, 64)], ids=repr)
def test_host_form_on_padded_states(row, words):
    for prop in (0, 1):
        assert_step_matches(host(StepGraph(*row, words=words), prop), reference(row, prop), (row, words, prop))


def test_host_form_counts_a_repeated_init_state_once():
    row = (12, 2, 1, 300, 0, 64)
    for prop in (0, 1):
        want = reference(row, prop, dup=5)
        assert (want["edges"], want["violations"]) == (reference(row, prop)["edges"], reference(row, prop)["violations"])
        assert_step_matches(host(StepGraph(*row, dup=5), prop), want, (row, prop))


@pytest.mark.parametrize("name", list(HAND))
def test_hand_drawn_graphs(name):
    forbidden, paths, figures, actions, init_index = HAND[name]
    succ, inits, props = S.step_dgraph(forbidden, paths)
    want = S.check(succ, inits, props[0])
    assert (want["edges"], want["violations"], want["sources"]) == figures, name
    assert (want.get("actions"), want.get("init_index", -1)) == (actions, init_index), name
    got = host(StepDGraph(forbidden, paths), 0)
    assert_step_matches(got, want, name)
    if name == "a violation only at an init state":
        assert (got["step_index"], got["witness_len"]) == (0, 1)


def test_two_phase_commit():
    m = TwoPhaseStepSys(3)
    stays, aborts = host(m, 3), host(m, 4)
    edges = sum(c["taken"] for c in N.coverage_host(m.MODEL_ID, m.params())["classes"])
    assert edges == sum(c["taken"] for c in N.coverage_host(TwoPhaseSys(3).MODEL_ID, [3])["classes"])
    assert (stays["unique"], stays["edges"], stays["violations"], stays["sources"], stays["actions"]) == (288, edges, 0, 0, [])
    assert aborts["edges"] == edges and aborts["violations"] == aborts["sources"] > 0  # (TmAbort is one slot)
    # the witness replays on the model's own graph, and its last action is the TM's abort out of a state with a prepared rm
    assert aborts["actions"][-1] == aborts["step_action"] == TM_ABORT and aborts["witness_len"] == aborts["step_index"] + 1 == 2
    succ, inits, _ = N.host_graph(m.MODEL_ID, m.params())
    state = inits[aborts["init_index"]]
    for a in aborts["actions"]:
        state = dict(succ[state])[a]  # (KeyError: the action is not enabled there)


def test_what_is_no_step_property_is_refused():
    with pytest.raises(ValueError, match="no step property"):
        N.step_host(TwoPhaseSys(3).MODEL_ID, [3], 0)
    with pytest.raises(ValueError, match="not a step property"):
        host(TwoPhaseStepSys(3), 2)
    with pytest.raises(ValueError, match="max_states"):
        N.step_host(N.SR_MODEL_STEP_GRAPH, StepGraph(12, 2, 1, 64).params(), 0, max_states=100)


def test_a_smaller_struct_size_is_honoured():
    m = StepGraph(8, 2, 1, 7)
    full = host(m, 0)
    part = N.step_host(m.MODEL_ID, m.params(), 0, struct_size=24)  # struct_size, ran, edges, violations
    assert (part["struct_size"], part["ran"], part["edges"], part["violations"]) == (24, 1, full["edges"], full["violations"])
    assert part["sources"] == 0xEEEEEEEEEEEEEEEE and part["witness_len"] == ctypes.c_int64(0xEEEEEEEEEEEEEEEE).value
    assert ctypes.sizeof(N.sr_step_result) == 80


def test_the_options_keep_their_size():
    # (the step pass added no option; the 8 bytes past 64 are the certificate pass' `certify` and its padding)
    assert ctypes.sizeof(N.sr_opts) == 72 and N.sr_opts.certify.offset == 64
