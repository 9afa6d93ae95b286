"""Leads-to properties on the GPU (`P ~> Q`; csrc/kernels_live.hpp live_leads_scan / live_leads_min,
Engine::live_leads_seed): in all four modes of the complete check and in both visit orders, the device's
counts, seed, depth, suffix (states and actions), end kind and loop offset equal the host form
(sr_liveness_host_leads) exactly; the prefix equals the host form's in FIFO order and is a replayable path
of the seed's depth in FAST order; the result is also held against the Python restatement
(tests/leads_ref.py). Sizes: LeadsGraph of 12 bits (3 K states: several workgroups, levels that are no
multiple of a wave) with one, 64 and duplicate roots, two and four words, a 16-bit row (61 K states, a
614-step suffix), ReqLock(3) and hand-drawn LeadsDGraphs.

Compared: sr_live_result without `rounds`, `examined`, `pass_ms`; sr_live_leads without `seed_ms`."""
import functools
import io

import pytest

import leads_ref as L
import live_fair_ref as LF
import stateright_amd as sr
from stateright_amd import _native as N, build
from stateright_amd.models import LeadsDGraph, LeadsGraph, LiveGraph, ReqLock
from stateright_amd.plugin import Plugin
from test_leads_host import assert_leads_matches, graph_of, reference

pytestmark = pytest.mark.gpu

FIELDS = ("ran", "not_p_states", "surviving", "end_kind", "witness_len")
LEADS_FIELDS = ("ran", "triggered", "pending", "violating", "trigger_index", "trigger_depth")
ORDERS = ("fifo", "fast")


def builder(model, mode, order=None, hint=None):
    b = model.checker()
    if mode == "none":
        b = b.complete_liveness()
    elif mode == "progress":
        b = b.complete_liveness(fairness="progress")
    elif mode == "weak":
        b = b.weak_fairness()
    elif mode == "strong":
        b = b.strong_fairness()
    if order:
        b = b.order(order)
    if hint:
        b = b.capacity_hint(hint)
    return b


def spawn(model, mode, order=None, hint=None):
    return builder(model, mode, order, hint).spawn_bfs().join()


@functools.lru_cache(maxsize=None)
def host_answer(model_id, params, prop, mode):
    return N.liveness_host_leads(model_id, list(params), prop, L.FAIRNESS[mode])


def rejected(c, name, actions, **kw):
    try:
        c.assert_discovery(name, actions, **kw)
    except AssertionError as e:
        return str(e)
    return None


def assert_device_is_host(c, model, prop, mode, order, graph, what):
    """c: a joined check in `mode`. graph: (succ, inits) of tests/leads_ref.py, to replay the paths on. Returns the
    device's result in the host form's shape."""
    succ, inits = graph
    name = c.properties()[prop][0]
    assert c.properties()[prop][1] == sr.Expectation.LeadsTo and c.is_done(), what
    r, found = c.liveness(name), c.discovery(name)
    host = host_answer(model.MODEL_ID, tuple(model.params()), prop, mode)
    assert c.unique_state_count() == host["unique"], what
    assert {k: r[k] for k in FIELDS} == {k: host[k] for k in FIELDS}, what
    assert {k: r["leads"][k] for k in LEADS_FIELDS} == {k: host["leads"][k] for k in LEADS_FIELDS}, what
    got = dict(r, actions=[] if found is None else found.action_ids)
    if host["init_index"] < 0:
        assert found is None and r["init_index"] == -1 and c.trigger_index(name) is None and c.loop_start(name) is None, what
        c.assert_no_discovery(name)
        return got
    ti = r["leads"]["trigger_index"]
    assert c.trigger_index(name) == ti, what
    assert r["loop_start"] - ti == host["loop_start"] - ti and (r["loop_start"] >= ti or r["loop_start"] == -1), what
    for fair in ("weak", "strong"):
        if mode == fair:
            assert r[fair]["ran"] == 1 and r["loop_start"] in (-1, ti + r[fair]["stem_len"]), what
            assert r["witness_len"] == ti + r[fair]["stem_len"] + r[fair]["loop_len"], what
    acts = got["actions"]
    mine = L.replay(succ, inits[r["init_index"]], acts)
    theirs = L.replay(succ, inits[host["init_index"]], host["actions"])
    assert mine is not None and len(mine) == len(theirs), what
    assert (acts[ti:], mine[ti:]) == (host["actions"][ti:], theirs[ti:]), what  # the seed and the suffix
    if order == "fifo":
        assert (r["init_index"], acts) == (host["init_index"], host["actions"]), what
    else:  # some shortest path: the seed's depth is its breadth-first distance
        assert len(acts[:ti]) == ti == host["leads"]["trigger_depth"] and mine[ti] == theirs[ti], what
    ls = r["loop_start"] if r["loop_start"] >= 0 else None
    assert c.loop_start(name) == ls, what
    c.assert_discovery(name, acts)
    c.assert_discovery(name, acts, trigger_index=ti, loop_start=ls)
    if ls is not None:  # the same path with the loop closing on the prefix is no counterexample
        why = rejected(c, name, acts, trigger_index=ti, loop_start=ti - 1)
        assert why is not None and "loop_start" in why, what
    return got


def check_row(row, mode, order, model=None, restated=True, props=(1, 2), hint=None):
    model = model or LeadsGraph(*row)
    succ, inits, cond, trig, nslots = graph_of(row)
    c = spawn(model, mode, order, hint)
    for prop in props:
        what = (row, prop, mode, order)
        got = assert_device_is_host(c, model, prop, mode, order, (succ, inits), what)
        if restated:
            assert_leads_matches(got, succ, inits, cond, trig[prop], nslots, mode, reference(row, prop, mode), what, fifo=order == "fifo")
    return c


# ---- the anchors, every mode, both orders ---------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("row", L.SMALL_ROWS, ids=[repr(r) for r in L.SMALL_ROWS])
def test_device_on_the_anchors(row, mode, order):
    c = check_row(row, mode, order)
    unique, triggered, pending, by_mode, always = L.GRAPH_ANCHORS[row]
    armed = c.liveness("armed ~> marked")
    assert (c.unique_state_count(), armed["leads"]["triggered"], armed["leads"]["pending"]) == (unique, triggered, pending)
    assert armed["leads"]["violating"] == by_mode[mode][0]
    # always-eventually: every state triggers, so the violating states are the mode's set for "marked" itself, which
    # the property's own pass reports (on every row; the `eventually` property's pass reports the same set where it
    # ran: not where the search discovered "marked" itself at a terminal state)
    ae = c.liveness("always eventually marked")
    assert ae["leads"]["triggered"] == unique, (row, mode)
    assert ae["leads"]["violating"] == (ae["surviving"] if mode in ("none", "progress") else ae[mode]["fair_states"]), (row, mode)
    ev = c.liveness("marked")
    if ev["ran"]:
        assert ev["surviving"] == ae["surviving"] and (mode in ("none", "progress") or ev[mode]["fair_states"] == ae[mode]["fair_states"])
    if mode == "none":
        assert ae["leads"]["violating"] == always[0] and ae["leads"]["trigger_depth"] == (always[2] if always[0] else -1)


def test_eventually_holds_where_leads_to_is_refuted():
    row = (12, 2, 1, 2, 0, 1, 7)
    c = spawn(LeadsGraph(*row), "none")
    assert c.discovery("marked") is None and c.liveness("marked")["init_index"] == -1
    assert c.discovery("armed ~> marked") is not None and c.trigger_index("armed ~> marked") == 5
    with pytest.raises(AssertionError, match="armed ~> marked"):
        c.assert_properties()
    out = io.StringIO()
    c.report(out)
    assert 'Discovered "armed ~> marked" counterexample' in out.getvalue()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", L.MODES)
def test_device_on_sixteen_bits(mode, order):
    """The row whose levels span many workgroups: in FIFO order the prefix is the host form's, level after level."""
    row = (16, 3, 7, 4, 0, 1, 9)
    c = check_row(row, mode, order, hint=1 << 17)
    unique, triggered, pending, by_mode, always = L.GRAPH_ANCHORS[row]
    ld = c.liveness("armed ~> marked")["leads"]
    assert (c.unique_state_count(), ld["triggered"], ld["pending"], ld["violating"]) == (unique, triggered, pending, by_mode[mode][0])
    ae = c.liveness("always eventually marked")
    assert ae["leads"]["violating"] == (ae["surviving"] if mode in ("none", "progress") else ae[mode]["fair_states"])
    if mode == "none":
        assert (ae["leads"]["violating"], ae["leads"]["trigger_depth"]) == (always[0], always[2])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("words", [2, 4])
def test_wide_states(words, order):
    """One tie-break round per word: the seed of a W-word state is the one of the one-word graph."""
    for row in ((12, 2, 1, 2, 0, 1, 7), (12, 2, 1, 2, 0, 64, 7)):
        for mode in ("none", "strong"):
            check_row(row, mode, order, model=LeadsGraph(*row, words=words))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", L.MODES)
def test_duplicate_roots(mode, order):
    """Level 0 of the arena holds the init states as given: equal ones count once, in every mode."""
    row = (12, 2, 1, 2, 0, 64, 7)
    model = LeadsGraph(*row, dup=16)
    succ, inits, cond, trig, nslots = L.leads_graph(*row, dup=16)
    c = spawn(model, mode, order)
    for prop in (1, 2):
        got = assert_device_is_host(c, model, prop, mode, order, (succ, inits), (prop, mode, order))
        assert got["leads"]["violating"] == reference(row, prop, mode)["violating"]
        if prop == 2:
            assert got["leads"]["triggered"] == c.unique_state_count()


@pytest.mark.parametrize("mode", L.MODES)
def test_the_witness_in_several_launches(mode, monkeypatch):
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "3")
    check_row((12, 2, 1, 2, 0, 64, 7), mode, "fifo")


@pytest.mark.parametrize("order", ORDERS)
def test_a_table_that_grows(order, monkeypatch):
    monkeypatch.setenv("SR_TABLE_LOG2", "10")
    row = (12, 2, 1, 2, 0, 1, 7)
    model = LeadsGraph(*row)
    succ, inits, cond, trig, nslots = graph_of(row)
    for mode in ("none", "weak"):
        c = builder(model, mode, order).counters().spawn_bfs().join()
        assert c.stats()["table_capacity"] > 1 << 10
        for prop in (1, 2):
            assert_device_is_host(c, model, prop, mode, order, (succ, inits), (prop, mode, order))
        a = c.table_audit()
        assert a["ran"] == 1 and a["occupied"] == a["arena_states"] == c.unique_state_count()
        assert (a["misplaced"], a["duplicates"], a["arena_missing"], a["arena_shared"], a["meta_wrong"]) == (0, 0, 0, 0, 0)


# ---- ReqLock -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", L.MODES)
def test_req_lock(mode, order):
    n = 3
    model = ReqLock(n)
    succ, inits = L.req_lock(n)
    c = spawn(model, mode, order)
    assert c.unique_state_count() == L.req_lock_states(n) == 40
    for p in range(n):
        name = f"thread {p} waiting ~> thread {p} holds"
        got = assert_device_is_host(c, model, p, mode, order, (succ, inits), (p, mode, order))
        assert got["leads"]["triggered"] == got["leads"]["pending"] == 16
        assert (c.discovery(name) is not None) == (mode != "strong")
        if mode in ("none", "progress"):
            assert got["leads"]["violating"] == 16 and got["leads"]["trigger_depth"] == 1
            assert c.discovery(name).states[1] == (0, 1 << p, 0)
    assert (c.discovery("some thread holds") is not None) == (mode in ("none", "progress"))
    out = io.StringIO()
    c.report(out)
    if mode == "strong":
        c.assert_properties()
        assert 'Leads-to "thread 0 waiting ~> thread 0 holds": holds (triggered 16 states)' in out.getvalue()


def test_liveness_off_leaves_the_property_unchecked():
    n = 3
    for order in ORDERS:
        c = ReqLock(n).checker().order(order).spawn_bfs().join()
        assert c.unique_state_count() == L.req_lock_states(n) and c.is_done()
        succ, inits = L.req_lock(n)  # the search explored everything: every successor of every state is counted
        assert c.state_count() == 1 + sum(len(v) for v in succ.values()) and c.max_depth() == max(L.fifo_tree(succ, inits)[0].values())
        name = "thread 1 waiting ~> thread 1 holds"
        r = c.liveness(name)
        assert r["ran"] == 0 and "leads" not in r and c.discovery(name) is None and c.trigger_index(name) is None
        out = io.StringIO()
        c.report(out)
        assert f'Leads-to "{name}": not checked' in out.getvalue()
        with pytest.raises(AssertionError, match="was not checked"):
            c.assert_properties()
        with pytest.raises(AssertionError, match="was not checked"):
            c.assert_no_discovery(name)


def test_vacuous_and_report():
    row = (12, 2, 1, 2, 0, 1, 0)
    c = spawn(LeadsGraph(*row), "none")
    ld = c.liveness("armed ~> marked")["leads"]
    assert (ld["triggered"], ld["pending"], ld["violating"]) == (0, 0, 0) and c.discovery("armed ~> marked") is None
    c.assert_no_discovery("armed ~> marked")
    out = io.StringIO()
    c.report(out)
    assert 'Leads-to "armed ~> marked": holds vacuously (never triggered)' in out.getvalue()
    assert c.properties() == [("marked", sr.Expectation.Eventually), ("armed ~> marked", sr.Expectation.LeadsTo),
                              ("always eventually marked", sr.Expectation.LeadsTo)]


# ---- LeadsDGraph ---------------------------------------------------------------------------------------------------------

DGRAPHS = [([[0, 1, 2, 4, 2]], [2], [0, 1, 2, 4, 2], 2, 2), ([[0, 1, 2, 4, 2]], [1], None, None, None),
           ([[0, 2, 4, 2]], [4], [0, 2, 4, 2, 4], 2, 2), ([[0, 2, 4], [1, 4, 6]], [4], None, None, -1)]


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("case", DGRAPHS, ids=repr)
def test_dgraph_hand_cases(case, mode):
    paths, triggers, states, ti, ls = case
    model = LeadsDGraph(triggers, paths)
    succ, inits, cond, trig, nslots = L.leads_dgraph(paths, triggers)
    c = spawn(model, mode)
    got = assert_device_is_host(c, model, 0, mode, "fifo", (succ, inits), (case, mode))
    assert_leads_matches(got, succ, inits, cond, trig, nslots, mode, L.check(succ, inits, cond, trig, mode, nslots), (case, mode))
    found = c.discovery("trigger ~> odd")
    if states is not None:
        assert [s[0] for s in found.states] == states and (c.trigger_index("trigger ~> odd"), c.loop_start("trigger ~> odd")) == (ti, ls)
    elif ls == -1:
        assert found.states[-1] == (6,) and got["end_kind"] == LF.END_TERMINAL and c.loop_start("trigger ~> odd") is None
    else:
        assert found is None and got["leads"]["pending"] == 0


# ---- other checkers accept the model and leave the property unchecked; what liveness refuses -------------------------------

def test_other_checkers_leave_it_unchecked():
    row = (12, 2, 1, 2, 0, 1, 7)
    model = LeadsGraph(*row)
    for c in (model.checker().spawn_dfs().join(), model.checker().partitions(2).spawn_bfs().join()):
        assert c.is_done() and c.discovery("armed ~> marked") is None and c.discovery("always eventually marked") is None
        assert "leads" not in c.liveness("armed ~> marked")
    assert model.checker().spawn_dfs().join().unique_state_count() == 3278
    cov = model.checker().coverage().spawn_bfs().join().coverage()
    succ, inits, cond, trig, nslots = graph_of(row)
    marked = sum(1 for s in succ if cond(s))
    assert cov["properties"] == {"marked": marked, "armed ~> marked": marked, "always eventually marked": marked}
    sim = model.checker().spawn_simulation(seed=1, walks=256, max_depth=64).join()
    assert sim.discovery("armed ~> marked") is None and sim.discovery("always eventually marked") is None
    out = io.StringIO()
    sim.report(out)
    assert 'Leads-to "armed ~> marked": not checked' in out.getvalue()


def test_refusals():
    model = LeadsGraph(12, 2, 1, 2, 0, 1, 7)
    with pytest.raises(sr.CheckerError, match="liveness with a partitioned search"):
        model.checker().complete_liveness().partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        model.checker().weak_fairness().target_state_count(10).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with symmetry"):
        model.checker().complete_liveness().symmetry_canonical().spawn_bfs()
    with pytest.raises(sr.CheckerError, match=r"more than 2\^32 - 1 unique states"):
        ReqLock(2).checker().strong_fairness().capacity_hint(2 ** 32).spawn_bfs()
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    with pytest.raises(sr.CheckerError, match="liveness with a plugin model"):
        puzzle.model(1, 4, 2, 3, 5, 8, 6, 7, 0).checker().complete_liveness().spawn_bfs()


def test_an_eventually_only_check_is_what_it_was():
    """LiveGraph has no leads-to property: the pass reports no leads-to figures for it, and its results are those
    of LeadsGraph's property 0 on the same graph (the same kernels on the same arena)."""
    row = (12, 2, 3, 2, 0, 1, 7)
    for mode in L.MODES:
        old, new = spawn(LiveGraph(*row[:6]), mode), spawn(LeadsGraph(*row), mode)
        a, b = old.liveness("marked"), new.liveness("marked")
        assert "leads" not in a and "leads" not in b
        ld = N.sr_live_leads()
        assert old._lib.sr_gpu_bfs_liveness_leads(old._h, 0, N.ctypes.byref(ld)) == 0 and ld.ran == 0
        for d in (a, b):
            d.pop("pass_ms"), d.pop("rounds"), d.pop("examined")
            for fair in ("weak", "strong"):
                if fair in d:
                    d[fair] = {k: v for k, v in d[fair].items() if k not in ("pass_ms", "scc_rounds", "reach_rounds")}
        assert a == b, mode
        assert old.discovery("marked") == new.discovery("marked")
        assert (old.unique_state_count(), old.state_count(), old.max_depth()) == (new.unique_state_count(), new.state_count(), new.max_depth())


def test_a_model_of_leads_to_properties_only_with_liveness_off():
    """With the pass off the search has nothing to await: it ends at its first pop as for a model without
    properties (no early exit inside a level, so no second run in FIFO order), and the property is unchecked."""
    model = LeadsDGraph([4], [[0, 2, 4, 2], [1, 4, 6]])
    c = model.checker().spawn_bfs().join()
    assert c.is_done() and (c.unique_state_count(), c.state_count(), c.max_depth()) == (2, 2, 0)
    assert c.stats()["order_used"] == N.SR_ORDER_FAST
    assert c.discovery("trigger ~> odd") is None and "leads" not in c.liveness("trigger ~> odd")
    with pytest.raises(AssertionError, match="was not checked"):
        c.assert_properties()
    on = model.checker().complete_liveness().spawn_bfs().join()  # with the pass on it explores everything
    assert on.unique_state_count() == 5 and on.liveness("trigger ~> odd")["leads"]["violating"] == 1
