"""The step pass on the MI355X (csrc/step.hpp, csrc/kernels_step.hpp step_scan / step_min) against the
independent Python restatement in tests/step_ref.py (itself checked against the issue's anchors, and the host
form against it, in tests/test_step_host.py): the three counts, the seed (depth, source, slot) and the witness.

In FIFO order the witness is the restatement's, action by action. In FAST order the figures, the seed, the
violating step and the witness' length are the same, but the path to the seed's source is that search's own tree
path: some replayable path of the seed's depth (the parent of a state is whichever state claimed it first).

Sizes: 44 states (less than a wave), 209 (less than a workgroup), 3146 .. 3306 (a partial last workgroup; with
the grid held at 2 workgroups, several strides), 52 k and 62 k (every wave of a stride busy), 64 init states
with 5 repeated, 4-word states, terminal states, and a table that grew before the pass."""
import io

import pytest

sr = pytest.importorskip("stateright_amd")

import step_ref as S  # noqa: E402
from stateright_amd import build  # noqa: E402
from stateright_amd.models import StepDGraph, StepGraph, TwoPhaseStepSys  # noqa: E402
from stateright_amd.plugin import Plugin  # noqa: E402
from test_step_host import HAND, TM_ABORT, assert_step_matches, graph_of, reference  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = ("fifo", "fast")
NAMES = ("no forbidden step", "never down")


def spawn(model, order="auto", hint=None):
    b = model.checker().order(order)
    if hint:
        b = b.capacity_hint(hint)
    return b.spawn_bfs().join()


def device_result(c, name):
    """The step pass' figures of a joined check in step_host()'s form, with the discovery's action ids."""
    got = c.step(name)
    assert got is not None, name
    path = c.discovery(name)
    got["actions"] = path.action_ids if path is not None else []
    got["unique"] = c.unique_state_count()
    return got


def check_graph(c, row, order, dup=0, what=None):
    """Every step property of a joined StepGraph check against the restatement; returns the results."""
    succ, inits, props = graph_of(row, dup)
    out = []
    for prop, name in enumerate(NAMES):
        want = reference(row, prop, dup)
        got = device_result(c, name)
        assert_step_matches(got, want, (what or row, order, name), fifo=order == "fifo")
        if want["seed"] is not None:  # the path replays on the restatement's graph and ends with the seed's step
            states = S.replay(succ, inits[got["init_index"]], got["actions"])
            assert states is not None and states[-2:] == want["states"][-2:], (row, order, name)
            assert [s[0] for s in c.discovery(name).into_states()] == states, (row, order, name)
            assert c.step_index(name) == want["depth"]
            c.assert_discovery(name, got["actions"])
        else:
            assert c.discovery(name) is None and c.step_index(name) is None
            c.assert_no_discovery(name)
        out.append(got)
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("row", list(S.ANCHORS), ids=[repr(r) for r in S.ANCHORS])
def test_anchors(row, order):
    c = spawn(StepGraph(*row), order, hint=S.ANCHORS[row][0])
    assert c.is_done() and c.unique_state_count() == S.ANCHORS[row][0]
    check_graph(c, row, order)


def test_both_orders_agree():
    """What does not depend on the visit order is identical: the figures, the seed's step and the last two states."""
    row = (16, 3, 7, 20000, 0, 1)
    a, b = (spawn(StepGraph(*row), order, hint=61630) for order in ORDERS)
    for name in NAMES:
        ra, rb = a.step(name), b.step(name)
        for k in ("edges", "violations", "sources", "step_index", "step_action", "init_index", "witness_len"):
            assert ra[k] == rb[k], (name, k)
        assert a.discovery(name).into_states()[-2:] == b.discovery(name).into_states()[-2:], name


@pytest.mark.parametrize("order", ORDERS)
def test_several_strides(order, monkeypatch):
    monkeypatch.setenv("SR_STEP_GRID", "2")  # 3146 states on 512 lanes: 7 strides, the last one partial
    row = (12, 2, 1, 50, 16, 1)  # (t_mod > 0: terminal states, which have no edge)
    check_graph(spawn(StepGraph(*row), order, hint=3146), row, order)


@pytest.mark.parametrize("order", ORDERS)
def test_repeated_init_states_count_once(order):
    row = (12, 2, 1, 300, 0, 64)
    c = spawn(StepGraph(*row, dup=5), order, hint=3306)
    assert c.state_count() > c.unique_state_count() == 3306
    with_dup = check_graph(c, row, order, dup=5)
    without = check_graph(spawn(StepGraph(*row), order, hint=3306), row, order)
    for x, y in zip(with_dup, without):
        assert (x["edges"], x["violations"], x["sources"]) == (y["edges"], y["violations"], y["sources"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("words", [2, 4])
def test_padded_states(words, order):
    row = (12, 2, 1, 300, 0, 64)
    check_graph(spawn(StepGraph(*row, words=words), order, hint=3306), row, order, what=(row, words))


@pytest.mark.parametrize("order", ORDERS)
def test_a_table_that_grows(order, monkeypatch):
    monkeypatch.setenv("SR_TABLE_LOG2", "10")
    row = (12, 2, 1, 64, 0, 1)
    c = spawn(StepGraph(*row), order)  # no capacity hint
    assert c.stats()["table_capacity"] > 1 << 10
    check_graph(c, row, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_drawn_graphs(name, order):
    forbidden, paths, figures, actions, init_index = HAND[name]
    succ, inits, props = S.step_dgraph(forbidden, paths)
    c = spawn(StepDGraph(forbidden, paths), order)
    got = device_result(c, "no forbidden step")
    assert_step_matches(got, S.check(succ, inits, props[0]), (name, order))  # (these graphs have one tree)
    assert (got["edges"], got["violations"], got["sources"]) == figures
    if actions is None:
        c.assert_properties()
    else:
        assert (got["actions"], got["init_index"]) == (actions, init_index)
        c.assert_discovery("no forbidden step", actions)


def test_dfs_takes_the_pass_too():
    row = (12, 2, 1, 64, 0, 1)
    check_graph(StepGraph(*row).checker().spawn_dfs().join(), row, "fast")


def test_two_phase_commit_beside_the_other_passes():
    stays, aborts = "a decided RM stays decided", "the TM never aborts once an RM is prepared"
    plain = spawn(TwoPhaseStepSys(4))
    cov = TwoPhaseStepSys(4).checker().coverage().spawn_bfs().join()
    both = TwoPhaseStepSys(4).checker().coverage().complete_liveness().spawn_bfs().join()
    ref = sr.TwoPhaseSys(4).checker().spawn_bfs().join()
    edges = sum(k["taken"] for k in cov.coverage()["classes"])
    assert edges == sum(k["taken"] for k in both.coverage()["classes"])
    for c in (plain, cov, both):
        assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (ref.unique_state_count(), ref.state_count(), ref.max_depth())
        s, a = c.step(stays), c.step(aborts)
        assert (s["edges"], s["violations"], s["sources"], s["witness_len"]) == (edges, 0, 0, -1)
        assert a["edges"] == edges and a["violations"] == a["sources"] > 0 and (a["step_index"], a["step_action"]) == (1, TM_ABORT)
        assert c.discovery(stays) is None and c.discovery(aborts).action_ids[-1] == TM_ABORT
        assert sorted(c.discoveries()) == sorted(["abort agreement", "commit agreement", aborts])
        c.assert_discovery(aborts, c.discovery(aborts).into_actions())
        c.assert_no_discovery(stays)
        out = io.StringIO()
        c.report(out)
        assert f'Step "{stays}": holds ({edges} edges)' in out.getvalue() and f'Discovered "{aborts}" counterexample' in out.getvalue()
    assert both.liveness("consistent")["ran"] == 0  # (no `eventually` property: the liveness pass had nothing to decide)


def test_assert_discovery_wants_a_violating_last_step():
    c = spawn(TwoPhaseStepSys(3))
    name = "the TM never aborts once an RM is prepared"
    c.assert_discovery(name, ["RmPrepare(2)", "TmRcvPrepared(2)", "TmAbort"])  # (any replayable path, not only the one found)
    with pytest.raises(AssertionError, match="does not violate"):
        c.assert_discovery(name, ["RmPrepare(0)", "RmPrepare(1)"])
    with pytest.raises(AssertionError, match="does not violate"):
        c.assert_discovery(name, ["TmAbort"])  # (no rm is prepared yet)
    with pytest.raises(AssertionError, match="cannot be replayed"):
        c.assert_discovery(name, ["TmAbort", "TmAbort"])
    with pytest.raises(AssertionError, match="Unexpected"):
        c.assert_properties()


def not_checked(c, names):
    for name in names:
        assert c.step(name) is None and c.step_index(name) is None and c.discovery(name) is None
        out = io.StringIO()
        c.report(out)
        assert f'Step "{name}": not checked' in out.getvalue()
        with pytest.raises(AssertionError):
            c.assert_no_discovery(name)
    with pytest.raises(AssertionError):
        c.assert_properties()


def test_where_the_property_is_not_checked():
    """No error at spawn, the search stops as if the property were absent, and the asserts say why."""
    two = ("a decided RM stays decided", "the TM never aborts once an RM is prepared")
    ref = sr.TwoPhaseSys(4).checker().spawn_bfs().join()
    part = TwoPhaseStepSys(4).checker().partitions(2).spawn_bfs().join()
    assert (part.unique_state_count(), part.state_count()) == (ref.unique_state_count(), ref.state_count())
    not_checked(part, two)
    with pytest.raises(AssertionError, match="was not checked"):
        part.assert_no_discovery(two[0])
    sym = TwoPhaseStepSys(4).checker().symmetry_canonical().spawn_bfs().join()
    assert sym.unique_state_count() == sr.TwoPhaseSys(4).checker().symmetry_canonical().spawn_bfs().join().unique_state_count()
    not_checked(sym, two)
    row = (12, 2, 1, 64, 0, 1)
    early = StepGraph(*row).checker().target_state_count(100).spawn_bfs().join()
    assert early.unique_state_count() < 3278
    not_checked(early, NAMES)
    sim = StepGraph(*row).checker().spawn_simulation(seed=1, walks=256, max_depth=64).join()
    not_checked(sim, NAMES)


def test_the_plugin_example():
    counter = Plugin(build.plugin_path("step_counter"), "step_counter")
    name = "no action takes the counter down"
    for order in ORDERS:
        c = counter.model(1001).checker().order(order).spawn_bfs().join()
        assert c.unique_state_count() == 1002 and c.properties() == [(name, sr.Expectation.AlwaysStep)]
        got = c.step(name)
        assert (got["edges"], got["violations"], got["sources"]) == (1001 + 1000 + 1, 1, 1)
        assert (got["step_index"], got["witness_len"], got["init_index"]) == (501, 502, 0)  # ceil(1001 / 2) steps up
        path = c.discovery(name)
        assert path.into_actions()[-1] == "Wrap" and path.into_states()[-2:] == [(1001,), (0,)]
        c.assert_discovery(name, ["Inc"] * 1001 + ["Wrap"])
