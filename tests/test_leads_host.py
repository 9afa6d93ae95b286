"""The leads-to check on the host (sr_liveness_host_leads, csrc/live.hpp LEADS-TO), checked without a device
against the independent Python restatement in tests/leads_ref.py in all four modes: the three counts, the
seed and its depth, the FIFO prefix action by action, the mode's own witness from the seed (the whole walk
in the plain and the progress mode, the stem in the fair modes), how it ends, and the acceptance rule over
the whole path (for loops through loop_problems of the weak and strong restatements). The restatement
itself is checked first against the issue's anchors.

Not compared: `rounds`, `examined`, the wall times."""
import pytest

import leads_ref as L
import live_fair_ref as LF
import live_strong_ref as LS
import live_weak_ref as LW
from stateright_amd import _native as N
from stateright_amd.models import LeadsDGraph, LeadsGraph, LiveGraph, ReqLock

_GRAPHS, _CHECKED = {}, {}


def graph_of(row):
    if row not in _GRAPHS:
        _GRAPHS[row] = L.leads_graph(*row)
    return _GRAPHS[row]


def reference(row, prop, mode):
    """leads_ref.check of LeadsGraph(*row)'s property `prop` in `mode`, computed once and shared."""
    k = (row, prop, mode)
    if k not in _CHECKED:
        succ, inits, cond, trig, nslots = graph_of(row)
        _CHECKED[k] = L.check(succ, inits, cond, trig[prop], mode, nslots)
    return _CHECKED[k]


def assert_leads_matches(got, succ, inits, cond, trig, nslots, mode, want, what, fifo=True):
    """got: liveness_host_leads()'s dict (or a device result in the same form); want: leads_ref.check().
    fifo=False (a device run in FAST order): the prefix is some replayable path of the seed's depth, not the
    FIFO one, and init_index is whatever init state it starts at."""
    ld = got["leads"]
    assert got["ran"] == 1 and ld["ran"] == 1, what
    if "unique" in got:
        assert got["unique"] == want["unique"], what
    assert (ld["triggered"], ld["pending"], ld["violating"]) == (want["triggered"], want["pending"], want["violating"]), what
    if want["seed"] is None:
        assert (got["init_index"], got["witness_len"], got["loop_start"], got["end_kind"], got["actions"]) == (-1, -1, -1, 0, []), what
        assert (ld["trigger_index"], ld["trigger_depth"]) == (-1, -1), what
        return
    ti = ld["trigger_index"]
    assert ti == ld["trigger_depth"] == want["depth"], what
    acts = got["actions"]
    assert got["witness_len"] == len(acts), what
    if fifo:
        assert got["init_index"] == want["init_index"] and acts[:ti] == want["prefix_actions"], what
    states = L.replay(succ, inits[got["init_index"]], acts)
    assert states is not None and states[ti] == want["seed"], what
    assert got["end_kind"] == want["end_kind"], what
    if mode in ("none", "progress"):
        assert acts[ti:] == want["suffix_actions"] and states[ti:] == want["suffix_states"], what
        assert got["loop_start"] == (ti + want["loop_start"] if want["loop_start"] >= 0 else -1), what
    else:
        stem = want["stem"]
        assert acts[ti:ti + len(stem)] == stem, what
        if "stem_len" in got.get(mode, {}):
            assert got[mode]["stem_len"] == len(stem), what
        if want["end_kind"] == LF.END_LOOP:
            assert got["loop_start"] == ti + len(stem), what
            loop = acts[got["loop_start"]:]
            check = LW.loop_problems if mode == "weak" else LS.loop_problems
            assert check(succ, cond, nslots, want["stem_states"][-1], loop, inside=want["comp"]) == [], what
        else:
            assert got["loop_start"] == -1 and len(acts) == ti + len(stem), what
    assert L.problems(succ, inits, cond, trig, mode, nslots, got["init_index"], acts, ti, got["loop_start"], got["end_kind"]) == [], what


def host(model, prop, mode):
    return N.liveness_host_leads(model.MODEL_ID, model.params(), prop, L.FAIRNESS[mode])


# ---- the restatement against the issue's anchors ---------------------------------------------------------------

@pytest.mark.parametrize("row", list(L.GRAPH_ANCHORS), ids=[repr(r) for r in L.GRAPH_ANCHORS])
def test_the_restatement_reproduces_the_anchors(row):
    unique, triggered, pending, by_mode, always = L.GRAPH_ANCHORS[row]
    for mode in L.MODES:
        want = reference(row, 1, mode)
        assert (want["unique"], want["triggered"], want["pending"]) == (unique, triggered, pending), (row, mode)
        violating, seed, depth = by_mode[mode]
        assert want["violating"] == violating, (row, mode)
        if seed is not None:
            assert (want["seed"], want["depth"]) == (seed, depth), (row, mode)
        assert (want["seed"] is None) == (violating == 0), (row, mode)
    want = reference(row, 2, "none")
    assert (want["violating"], want["seed"], want["depth"]) == always, row
    assert want["triggered"] == unique and want["violating"] == want["x"], row


def test_eventually_holds_where_leads_to_is_refuted():
    """The point of the feature: on the first row `eventually "marked"` has no counterexample (no init state
    is in F_p) while "armed ~> marked" has one, at depth 5."""
    row = (12, 2, 1, 2, 0, 1, 7)
    ev = N.liveness_host(LiveGraph(*row[:6]).MODEL_ID, list(row[:6]))
    assert ev["init_index"] == -1 and ev["witness_len"] == -1
    ev = N.liveness_host(LeadsGraph(*row).MODEL_ID, list(row), prop=0)
    assert ev["init_index"] == -1 and ev["surviving"] == 475
    got = host(LeadsGraph(*row), 1, "none")
    assert got["leads"]["violating"] == 68 and got["leads"]["trigger_depth"] == 5 and got["witness_len"] > 5


# ---- the host form against the restatement ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("prop", [1, 2])
@pytest.mark.parametrize("row", L.SMALL_ROWS, ids=[repr(r) for r in L.SMALL_ROWS])
def test_the_host_form_matches_the_restatement(row, prop, mode):
    succ, inits, cond, trig, nslots = graph_of(row)
    want = reference(row, prop, mode)
    got = host(LeadsGraph(*row), prop, mode)
    assert_leads_matches(got, succ, inits, cond, trig[prop], nslots, mode, want, (row, prop, mode))
    if prop == 2:  # always-eventually: every state triggers, so the violating states are X_Q itself
        assert got["leads"]["triggered"] == got["unique"], (row, mode)
        if mode in ("none", "progress"):
            assert got["leads"]["violating"] == got["surviving"], (row, mode)
        else:
            flat = (N.liveness_host_weak if mode == "weak" else N.liveness_host_strong)(LeadsGraph(*row).MODEL_ID, list(row), prop=0)
            assert got["leads"]["violating"] == flat[mode]["fair_states"] == want["x"], (row, mode)


@pytest.mark.parametrize("mode", L.MODES)
def test_the_large_row(mode):
    """The 16-bit row (61 K states) in every mode: against its anchor and against the restatement."""
    row = (16, 3, 7, 4, 0, 1, 9)
    succ, inits, cond, trig, nslots = graph_of(row)
    unique, triggered, pending, by_mode, always = L.GRAPH_ANCHORS[row]
    for prop in (1, 2):
        got = host(LeadsGraph(*row), prop, mode)
        ld = got["leads"]
        assert_leads_matches(got, succ, inits, cond, trig[prop], nslots, mode, reference(row, prop, mode), (row, prop, mode))
        if prop == 1:
            assert (got["unique"], ld["triggered"], ld["pending"], ld["violating"]) == (unique, triggered, pending, by_mode[mode][0]), mode
        elif mode in ("none", "progress"):
            assert ld["violating"] == got["surviving"], mode
        else:
            flat = (N.liveness_host_weak if mode == "weak" else N.liveness_host_strong)(LeadsGraph(*row).MODEL_ID, list(row), prop=0)
            assert ld["violating"] == flat[mode]["fair_states"], mode


@pytest.mark.parametrize("words", [2, 4])
def test_wide_states_change_nothing(words):
    row = (12, 2, 1, 2, 0, 1, 7)
    for mode in L.MODES:
        one, wide = host(LeadsGraph(*row), 1, mode), host(LeadsGraph(*row, words=words), 1, mode)
        for d in (one, wide):
            d.pop("pass_ms"), d["leads"].pop("seed_ms"), d.pop("rounds"), d.pop("examined")
        assert one == wide, (words, mode)


def test_duplicate_roots_count_once():
    row = (12, 2, 1, 2, 0, 64, 7)
    succ, inits, cond, trig, nslots = L.leads_graph(*row, dup=16)
    for mode in L.MODES:
        for prop in (1, 2):
            want = L.check(succ, inits, cond, trig[prop], mode, nslots)
            assert want["violating"] == reference(row, prop, mode)["violating"]
            got = host(LeadsGraph(*row, dup=16), prop, mode)
            assert_leads_matches(got, succ, inits, cond, trig[prop], nslots, mode, want, (prop, mode))


# ---- ReqLock: the textbook result ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3])
def test_req_lock(n):
    succ, inits = L.req_lock(n)
    assert len(succ) == L.req_lock_states(n) == {1: 6, 2: 16, 3: 40}[n]
    key = lambda s: L.req_lock_word(s, n)
    nslots = 3 * n + 1
    for p in range(n):
        cond, trig = (lambda s, p=p: s[0] == p + 1), (lambda s, p=p: bool(s[1] >> p & 1))
        for mode in L.MODES:
            want = L.check(succ, inits, cond, trig, mode, nslots, key)
            got = host(ReqLock(n), p, mode)
            assert_leads_matches(got, succ, inits, cond, trig, nslots, mode, want, (n, p, mode))
            ld = got["leads"]
            assert ld["triggered"] == ld["pending"] == {1: 2, 2: 6, 3: 16}[n], (n, p, mode)
            refuted = mode in ("none", "progress") or (mode == "weak" and n >= 2)
            assert (ld["violating"] > 0) == refuted, (n, p, mode)
            if mode in ("none", "progress"):  # the clock's cycle: every pending state violates
                assert ld["violating"] == ld["pending"], (n, p, mode)
                assert (want["seed"], ld["trigger_depth"]) == ((0, 1 << p, 0), 1), (n, p, mode)
    # eventually "some thread holds": the existing check, on the same model
    some = lambda s: s[0] != 0
    for fairness, refuted in ((0, True), (1, True)):
        assert (N.liveness_host(ReqLock(n).MODEL_ID, [n], prop=n, fairness=fairness)["init_index"] == 0) == refuted
    assert LW.check(succ, inits, some, nslots)["init_index"] == -1
    assert N.liveness_host_weak(ReqLock(n).MODEL_ID, [n], prop=n)["init_index"] == -1
    assert N.liveness_host_strong(ReqLock(n).MODEL_ID, [n], prop=n)["init_index"] == -1


# ---- LeadsDGraph: hand-drawn graphs ----------------------------------------------------------------------------------

def dgraph_host(paths, triggers, mode="none"):
    model = LeadsDGraph(triggers, paths)
    succ, inits, cond, trig, nslots = L.leads_dgraph(paths, triggers)
    got = host(model, 0, mode)
    want = L.check(succ, inits, cond, trig, mode, nslots)
    assert_leads_matches(got, succ, inits, cond, trig, nslots, mode, want, (paths, triggers, mode))
    states = L.replay(succ, inits[got["init_index"]], got["actions"]) if got["init_index"] >= 0 else None
    return got, states


def test_dgraph_the_prefix_may_pass_the_condition():
    got, states = dgraph_host([[0, 1, 2, 4, 2]], [2])
    assert states == [0, 1, 2, 4, 2] and (got["leads"]["trigger_index"], got["loop_start"]) == (2, 2)


def test_dgraph_a_trigger_where_the_condition_holds_is_not_pending():
    got, _ = dgraph_host([[0, 1, 2, 4, 2]], [1])
    assert (got["leads"]["triggered"], got["leads"]["pending"], got["leads"]["violating"], got["init_index"]) == (1, 0, 0, -1)


def test_dgraph_the_loop_closes_on_the_suffix():
    got, states = dgraph_host([[0, 2, 4, 2]], [4])
    assert states == [0, 2, 4, 2, 4] and (got["leads"]["trigger_index"], got["loop_start"]) == (2, 2)


def test_dgraph_a_terminal_end():
    got, states = dgraph_host([[0, 2, 4], [1, 4, 6]], [4])
    assert states[-1] == 6 and got["end_kind"] == LF.END_TERMINAL and got["loop_start"] == -1


@pytest.mark.parametrize("mode", L.MODES)
def test_dgraph_in_every_mode(mode):
    for paths, triggers in (([[0, 1, 2, 4, 2]], [2]), ([[0, 2, 4, 2]], [4]), ([[0, 2, 4], [1, 4, 6]], [4]),
                            ([[0, 2, 4, 2], [2, 6, 6]], [0, 4])):
        dgraph_host(paths, triggers, mode)


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals():
    row = (12, 2, 1, 2, 0, 1, 7)
    with pytest.raises(ValueError, match="not a leads-to property"):
        host(LeadsGraph(*row), 0, "none")
    with pytest.raises(ValueError, match="not an `eventually` property"):
        N.liveness_host(LeadsGraph(*row).MODEL_ID, list(row), prop=1)
    with pytest.raises(ValueError, match="no leads-to property"):
        N.liveness_host_leads(LiveGraph(*row[:6]).MODEL_ID, list(row[:6]), 0, 0)
    with pytest.raises(ValueError, match="fairness must be"):
        N.liveness_host_leads(LeadsGraph(*row).MODEL_ID, list(row), 1, 4)
    with pytest.raises(ValueError, match="max_states"):
        N.liveness_host_leads(LeadsGraph(*row).MODEL_ID, list(row), 1, 0, max_states=100)
