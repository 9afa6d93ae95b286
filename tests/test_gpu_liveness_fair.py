"""Progress fairness of the complete `eventually` check on the MI355X
(`CheckerBuilder.complete_liveness(fairness="progress")`; csrc/live.hpp, the FAIR instantiations of
live_trim and live_walk in csrc/kernels_live.hpp) against the host form of the same rule
(sr_liveness_host_fair) and the independent Python restatement (tests/live_fair_ref.py), in both modes.

Sizes: the DGraph hand cases (2-3 states), LiveGraph n_bits 4-12 (a wave to several workgroups with a
tail) and one of 16 bits (52 k states, ~100 shrinking worklists), 2- and 4-word states for the
multi-word compare and the walk's cross-lane copy, 2pc-live N = 3, 4, 5 (288 to 8 832 states; N = 5
spreads the witness' slots over both mask words of the wave's shared scan)."""
import functools

import pytest

sr = pytest.importorskip("stateright_amd")

import live_fair_ref as F  # noqa: E402
import live_ref  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import LiveGraph, TwoPhaseLiveSys  # noqa: E402
from test_liveness_fair_host import COMMITS_PROGRESS, F_ANCHORS, STUTTER_ONLY  # noqa: E402
from test_liveness_host import FIXME_CYCLE  # noqa: E402

pytestmark = pytest.mark.gpu

EVENTUALLY = N.SR_EVENTUALLY
MODES = [None, "progress"]
FIELDS = ("not_p_states", "surviving", "init_index", "witness_len", "loop_start", "end_kind")


def spawn(model, fairness, order="auto", on=True):
    return model.checker().complete_liveness(on, fairness=fairness).order(order).spawn_bfs().join()


def dgraph(paths):
    g = sr.DGraph.with_property(EVENTUALLY)
    for p in paths:
        g = g.with_path(p)
    return g


@functools.lru_cache(maxsize=None)
def live_graph(params):
    return live_ref.live_graph(*params)


@functools.lru_cache(maxsize=None)
def live_graph_ref(params, fair):
    return F.check(*live_graph(params), skip_self=fair)


@functools.lru_cache(maxsize=None)
def two_phase_graph(n):
    return F.two_phase(n)


@functools.lru_cache(maxsize=None)
def two_phase_ref(n, p, fair):
    succ, inits = two_phase_graph(n)
    return F.check(succ, inits, F.TWO_PHASE_LIVE_PROPS[p][1], skip_self=fair)


def rejected(c, name, actions):
    try:
        c.assert_discovery(name, actions)
    except AssertionError:
        return True
    return False


def ref_accepts(graph, actions, fair):
    """Whether, on the reference graph, the actions are a counterexample from SOME init state: the condition
    holds nowhere on the path, which ends at a terminal state, at a state equal to an earlier one or (fair)
    at a stutter end. (`assert_discovery` tries every init state: with several, a witness cut short can be
    a counterexample of its own from another one, as [2] is from init state 2 of [[0, 2, 2], [2, 1]].)"""
    succ, inits, cond = graph
    for s in inits:
        states = [s]
        for a in actions:
            nxt = [t for b, t in succ[states[-1]] if b == a]
            if not nxt:
                break
            states.append(nxt[0])
        else:
            last = states[-1]
            sink = not succ[last] or (fair and all(t == last for _, t in succ[last]))
            if not any(cond(x) for x in states) and (sink or last in states[:-1]):
                return True
    return False


def assert_check(c, model, name, prop, fairness, want, what, graph):
    """c: a joined check of `model` with the option on in mode `fairness`; want: live_fair_ref.check() of
    its graph in that mode. Returns whether the pass made the answer (a terminal counterexample may be
    the search's own discovery; it is then only checked for validity)."""
    r = c.liveness(name)
    found = c.discovery(name)
    w = want["witness"]
    if not r["ran"]:
        assert found is not None and w is not None, what
        c.assert_discovery(name, found.action_ids)
        return False
    host = N.liveness_host(model.MODEL_ID, model.params(), prop=prop, fairness=int(fairness == "progress"))
    assert {k: r[k] for k in FIELDS} == {k: host[k] for k in FIELDS}, what
    assert (r["not_p_states"], r["surviving"]) == (want["not_p_states"], want["surviving"]), what
    assert c.unique_state_count() == host["unique"] == want["unique"] and c.is_done(), what
    if w is None:
        assert found is None and r["end_kind"] == 0, what
        return True
    assert found is not None, what
    assert found.action_ids == w["actions"] == host["actions"], what
    assert (r["init_index"], r["loop_start"], r["end_kind"]) == (w["init_index"], w["loop_start"], w["end_kind"]), what
    assert c.loop_start(name) == (w["loop_start"] if w["loop_start"] >= 0 else None), what
    states = found.into_states()
    assert len(states) == len(w["actions"]) + 1, what
    if fairness == "progress":
        assert all(a != b for a, b in zip(states, states[1:])), what  # no step returns its own state
    c.assert_discovery(name, found.action_ids)
    if w["actions"]:  # one step short: no sink and no closed loop from the witness' own init state
        short = found.action_ids[:-1]
        assert not ref_accepts((graph[0], [graph[1][w["init_index"]]], graph[2]), short, fairness == "progress"), what
        assert rejected(c, name, short) == (not ref_accepts(graph, short, fairness == "progress")), what
    return True


# ---- DGraph: the hand cases -------------------------------------------------------------------------------

def test_a_self_edge_is_a_lasso_without_fairness_and_a_stutter_end_with_it():
    paths = [[0, 2, 2]]
    c = spawn(dgraph(paths), None)
    assert c.discovery("odd").into_states() == [(0,), (2,), (2,)]
    assert (c.loop_start("odd"), c.liveness("odd")["end_kind"]) == (1, 2)
    assert rejected(c, "odd", [2])  # a stutter end is no counterexample with the mode off
    assert assert_check(c, dgraph(paths), "odd", 0, None, F.check(*live_ref.dgraph(paths)), paths, live_ref.dgraph(paths))
    c = spawn(dgraph(paths), "progress")
    assert c.discovery("odd").into_states() == [(0,), (2,)]
    assert (c.loop_start("odd"), c.liveness("odd")["end_kind"], c.liveness("odd")["loop_start"]) == (None, 3, -1)
    c.assert_discovery("odd", [2])
    c.assert_discovery("odd", [2, 2])  # (the lasso is still a path on which "odd" never holds)
    assert rejected(c, "odd", [])
    assert assert_check(c, dgraph(paths), "odd", 0, "progress", F.check(*live_ref.dgraph(paths), skip_self=True), paths, live_ref.dgraph(paths))


def test_a_state_that_can_leave_its_self_loop_is_no_counterexample():
    paths = [[0, 2, 2], [2, 1]]
    c = spawn(dgraph(paths), None)
    assert c.discovery("odd").into_states() == [(0,), (2,), (2,)]
    assert assert_check(c, dgraph(paths), "odd", 0, None, F.check(*live_ref.dgraph(paths)), paths, live_ref.dgraph(paths))
    c = spawn(dgraph(paths), "progress")
    assert c.discovery("odd") is None and c.liveness("odd")["surviving"] == 0
    c.assert_properties()
    assert assert_check(c, dgraph(paths), "odd", 0, "progress", F.check(*live_ref.dgraph(paths), skip_self=True), paths, live_ref.dgraph(paths))


@pytest.mark.parametrize("fairness", MODES)
def test_a_cycle_through_two_states_refutes_in_both_modes(fairness):
    c = spawn(dgraph(FIXME_CYCLE), fairness)
    assert c.discovery("odd").into_states() == [(0,), (2,), (4,), (2,)] and c.loop_start("odd") == 1
    want = F.check(*live_ref.dgraph(FIXME_CYCLE), skip_self=fairness == "progress")
    assert assert_check(c, dgraph(FIXME_CYCLE), "odd", 0, fairness, want, FIXME_CYCLE, live_ref.dgraph(FIXME_CYCLE))


# ---- LiveGraph ---------------------------------------------------------------------------------------------

LIVE_GRAPHS = sorted(F_ANCHORS) + [(6, 2, 5, 3, 0, 1), STUTTER_ONLY]


@pytest.mark.parametrize("fairness", MODES)
@pytest.mark.parametrize("params", LIVE_GRAPHS)
def test_live_graph_anchors(params, fairness):
    fair = fairness == "progress"
    want = live_graph_ref(params, fair)
    if params in F_ANCHORS:
        assert want["surviving"] == F_ANCHORS[params][fair]
    model = LiveGraph(*params)
    assert_check(spawn(model, fairness), model, "marked", 0, fairness, want, (params, fairness), live_graph(params))


# graphs whose witness under progress fairness ends at a stutter end: after 8 steps from init state 2, after
# 2 steps (degree 2), at init state 11 itself (no step), at a state whose three actions all return it
STUTTER_WITNESSES = [(6, 1, 1046708790864, 3, 0, 40), (2, 2, 754802668508, 2, 0, 4), (5, 1, 789375578745, 5, 0, 17),
                     (1, 3, 392951442463, 2, 0, 1)]


@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("params", STUTTER_WITNESSES)
def test_witnesses_that_end_at_a_stutter_end(params, order):
    model = LiveGraph(*params)
    want = live_graph_ref(params, True)
    assert F.outcome(want) == "stutter" and F.outcome(live_graph_ref(params, False)) == "lasso"
    assert assert_check(spawn(model, "progress", order), model, "marked", 0, "progress", want, (params, order), live_graph(params))
    assert assert_check(spawn(model, None, order), model, "marked", 0, None, live_graph_ref(params, False), (params, order), live_graph(params))


@pytest.mark.parametrize("fairness", MODES)
@pytest.mark.parametrize("words", [2, 4])
def test_wide_states(words, fairness, monkeypatch):
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "7")  # the 20-step witness takes three launches
    params = (12, 2, 3, 2, 0, 1)
    model = LiveGraph(*params, words=words)
    c = spawn(model, fairness)
    assert c.stats()["words_per_state"] == words
    assert assert_check(c, model, "marked", 0, fairness, live_graph_ref(params, fairness == "progress"), (words, fairness), live_graph(params))
    assert c.liveness("marked")["witness_len"] == 20


def test_a_grown_table_gives_the_same_answer(monkeypatch):
    params = (16, 2, 1, 2, 0, 1)
    model = LiveGraph(*params)
    want = live_graph_ref(params, True)
    c = model.checker().complete_liveness(fairness="progress").spawn_bfs().join()  # no capacity hint
    assert assert_check(c, model, "marked", 0, "progress", want, params, live_graph(params))
    monkeypatch.setenv("SR_DISP_LIMIT", "2")  # a probe limit of two slots: the table doubles in the middle of the check
    c = model.checker().complete_liveness(fairness="progress").spawn_bfs().join()
    assert c.stats()["table_doublings"] > 0
    assert assert_check(c, model, "marked", 0, "progress", want, params, live_graph(params))
    c = model.checker().complete_liveness(fairness="progress").capacity_hint(1 << 16).spawn_bfs().join()
    assert assert_check(c, model, "marked", 0, "progress", want, params, live_graph(params))


# ---- 2pc with `eventually` properties ------------------------------------------------------------------------

@pytest.mark.parametrize("fairness", MODES)
@pytest.mark.parametrize("n", [3, 4, 5])
def test_two_phase_live(n, fairness):
    fair = fairness == "progress"
    model = TwoPhaseLiveSys(n)
    c = spawn(model, fairness)
    assert [name for name, _ in c.properties()][3:] == ["every RM decides", "every RM commits"]
    for p, (name, _) in F.TWO_PHASE_LIVE_PROPS.items():
        assert assert_check(c, model, name, p, fairness, two_phase_ref(n, p, fair), (n, name, fairness),
                            two_phase_graph(n) + (F.TWO_PHASE_LIVE_PROPS[p][1],))
    decides, commits = c.liveness("every RM decides"), c.liveness("every RM commits")
    if fair:
        assert c.discovery("every RM decides") is None and decides["surviving"] == 0  # it holds
        assert (commits["not_p_states"], commits["surviving"], c.discovery("every RM commits").action_ids) == COMMITS_PROGRESS[n]
        assert (commits["end_kind"], commits["loop_start"]) == (3, -1)
        assert c.discovery("every RM commits").last_state()[:n] == (3,) * n  # every rm Aborted
    else:
        assert decides["surviving"] == decides["not_p_states"] and decides["end_kind"] == 2  # refuted by stuttering
        assert (c.discovery("every RM commits").action_ids, commits["loop_start"]) == ([1, 3, 6, 6], 3)
    for name in ("abort agreement", "commit agreement"):
        assert c.discovery(name) is not None and c.liveness(name)["ran"] == 0
    assert c.discovery("consistent") is None


@pytest.mark.parametrize("order", ["fifo", "fast"])
def test_two_phase_live_counts_are_two_phases(order):
    base = sr.TwoPhaseSys(3).checker().order(order).spawn_bfs().join()
    assert (base.unique_state_count(), base.state_count()) == (288, 1146)
    for on, fairness in [(False, None), (True, None), (True, "progress")]:
        c = spawn(TwoPhaseLiveSys(3), fairness, order, on=on)
        assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (288, 1146, base.max_depth())
        for name in ("abort agreement", "commit agreement"):
            c.assert_discovery(name, c.discovery(name).action_ids)
            if order == "fifo":
                assert c.discovery(name) == base.discovery(name)
        assert c.discovery("consistent") is None
        if not on:  # 2pc has no terminal state: the search refutes no `eventually` property
            assert c.discovery("every RM decides") is None and c.discovery("every RM commits") is None
            assert c.liveness("every RM commits")["ran"] == 0


# ---- the option ------------------------------------------------------------------------------------------------

def test_progress_fairness_meets_the_same_refusals():
    from stateright_amd import build
    from stateright_amd.plugin import Plugin
    b = TwoPhaseLiveSys(3).checker().complete_liveness(fairness="progress")
    assert b._opts.liveness == 2
    with pytest.raises(sr.CheckerError, match="liveness with a partitioned search"):
        b.partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        TwoPhaseLiveSys(3).checker().complete_liveness(fairness="progress").target_state_count(10).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with symmetry"):
        sr.TwoPhaseSys(3).checker().complete_liveness(fairness="progress").symmetry_canonical().spawn_bfs()
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    with pytest.raises(sr.CheckerError, match="liveness with a plugin model"):
        puzzle.model(1, 4, 2, 3, 5, 8, 6, 7, 0).checker().complete_liveness(fairness="progress").spawn_bfs()
    with pytest.raises(sr.CheckerError, match=r"more than 2\^32 - 1 unique states"):
        TwoPhaseLiveSys(3).checker().complete_liveness(fairness="progress").capacity_hint(2 ** 32).spawn_bfs()
    with pytest.raises(ValueError, match="fairness"):
        TwoPhaseLiveSys(3).checker().complete_liveness(fairness="nonsense")
    # any other value of sr_opts.liveness is the plain mode, as it always was
    b = dgraph([[0, 2, 2]]).checker().complete_liveness()
    b._opts.liveness = 7
    c = b.spawn_bfs().join()
    assert c.discovery("odd").into_states() == [(0,), (2,), (2,)] and c.liveness("odd")["end_kind"] == 2
