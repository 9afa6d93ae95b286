"""The complete `eventually` check on the MI355X (`CheckerBuilder.complete_liveness()`, csrc/live.hpp,
csrc/kernels_live.hpp) against the independent Python restatement (tests/live_ref.py) and the host
form of the same rule (sr_liveness_host): the sizes of N_p and F_p, which properties get a discovery,
and the deterministic witness, state by state.

Sizes: LiveGraph n_bits 8 (a few waves), 12 (several workgroups and a wave tail) and 16 (52 k states,
about 100 shrinking worklists), the smallest that cross those boundaries."""
import functools
import random

import pytest

sr = pytest.importorskip("stateright_amd")

import live_ref  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd import build  # noqa: E402
from stateright_amd.models import LiveGraph  # noqa: E402
from stateright_amd.plugin import Plugin  # noqa: E402
from test_liveness_host import (CAN_VALIDATE, FIXME_CYCLE, FIXME_JOIN, PINGPONG_EVENTUALLY, random_graph,  # noqa: E402
                                random_live_graphs)

pytestmark = pytest.mark.gpu

EVENTUALLY = N.SR_EVENTUALLY


@functools.lru_cache(maxsize=None)
def live_graph_ref(params):
    return live_ref.check(*live_ref.live_graph(*params))


def spawn(model, order="auto", on=True):
    b = model.checker().complete_liveness(on)
    if order == "dfs":
        return b.spawn_dfs().join()
    return b.order(order).spawn_bfs().join()


def dgraph(paths):
    g = sr.DGraph.with_property(EVENTUALLY)
    for p in paths:
        g = g.with_path(p)
    return g


def validity(c, name, actions):
    try:
        c.assert_discovery(name, actions)
        return None
    except AssertionError as e:
        return str(e).split(", but a valid one")[0].replace(" and closes no loop", "")


def assert_check(c, name, want, what, states_of=lambda s: s, off=None):
    """c: a joined check with the option on; want: live_ref.check() of its model (or a dict with the
    same keys from the host form, `states` None). Returns whether the pass made the answer.
    off: the same check with the option off, for a model on which the search's own discovery need not
    pass `assert_discovery`, as in the reference: with several properties the search goes on after
    the discovery of an `eventually` property, `discoveries.insert` overwrites and a discovered
    property's bit is no longer cleared, so a later terminal state is reported on whose path the
    property held; and `assert_discovery` takes a state at the boundary, whose listed actions all
    lead nowhere, for nonterminal. The pass keeps the search's discovery as it is: the path must be
    the one the check gives with the option off, and as valid or invalid as there."""
    r = c.liveness(name)
    found = c.discovery(name)
    w = want["witness"]
    if not r["ran"]:
        # the search itself discovered it: a valid counterexample, which only exists if an init state is in F
        assert found is not None and w is not None, what
        if off is None:
            c.assert_discovery(name, found.action_ids)
        else:
            assert off.discovery(name) == found, what
            assert validity(c, name, found.action_ids) == validity(off, name, found.action_ids), what
        return False
    assert (r["not_p_states"], r["surviving"]) == (want["not_p_states"], want["surviving"]), what
    assert c.is_done(), what
    if w is None:
        assert found is None and (r["init_index"], r["witness_len"], r["loop_start"]) == (-1, -1, -1), what
        assert c.loop_start(name) is None, what
        return True
    assert found is not None, what
    assert (r["init_index"], r["witness_len"], r["loop_start"]) == (w["init_index"], len(w["actions"]), w["loop_start"]), what
    assert found.action_ids == w["actions"], what
    if w.get("states") is not None:
        assert found.into_states() == [states_of(s) for s in w["states"]], what
    assert c.loop_start(name) == (w["loop_start"] if w["loop_start"] >= 0 else None), what
    assert len(c.discovery_fingerprints(name)) == len(w["actions"]) + 1, what
    c.assert_discovery(name, found.action_ids)
    return True


# ---- the LiveGraph fixture ------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["fifo", "fast", "dfs"])
@pytest.mark.parametrize("params", sorted(live_ref.ANCHORS))
def test_live_graph_anchors(params, order):
    want = live_graph_ref(params)
    c = spawn(LiveGraph(*params), order)
    if assert_check(c, "marked", want, (params, order), lambda v: (v,)):
        assert c.unique_state_count() == want["unique"]
        assert c.stats()["order_used"] == (1 if order == "fifo" else 2)


def test_live_graph_random_parameters():
    ran = 0
    for params in random_live_graphs():
        ran += assert_check(spawn(LiveGraph(*params)), "marked", live_graph_ref(params), params, lambda v: (v,))
    assert ran >= 20  # (the search itself discovers only terminal counterexamples)


def test_witness_over_several_launches(monkeypatch):
    # 614 steps in launches of at most 100: each goes on from the last state of the one before
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "100")
    params = (16, 3, 7, 4, 0, 1)
    assert assert_check(spawn(LiveGraph(*params)), "marked", live_graph_ref(params), params, lambda v: (v,))


@pytest.mark.parametrize("params", [(16, 2, 1, 2, 0, 1), (16, 3, 7, 4, 0, 1)])
def test_table_growth_and_doublings_give_the_same_answer(params, monkeypatch):
    want = live_graph_ref(params)
    c = spawn(LiveGraph(*params))  # no capacity hint
    assert assert_check(c, "marked", want, params, lambda v: (v,)) and c.unique_state_count() == want["unique"]
    assert c.stats()["table_doublings"] == 0
    # a probe limit of two slots: levels overflow it and the table doubles in the middle of the check
    monkeypatch.setenv("SR_DISP_LIMIT", "2")
    c = spawn(LiveGraph(*params))
    assert assert_check(c, "marked", want, params, lambda v: (v,)) and c.unique_state_count() == want["unique"]
    assert c.stats()["table_doublings"] > 0


# ---- wide states with cycles: the witness walk copies W words across lanes and stores them ---------

@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("words", [2, 4])
def test_wide_live_graph_witnesses(words, order, monkeypatch):
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "250")  # the 614-step witness takes three launches
    made = 0
    for params in [(8, 2, 1, 3, 0, 1), (12, 2, 3, 2, 0, 1), (12, 2, 1, 3, 16, 1), (12, 2, 1, 2, 0, 64), (16, 3, 7, 4, 0, 1)]:
        want = live_graph_ref(params)
        c = spawn(LiveGraph(*params, words=words), order)
        assert c.stats()["words_per_state"] == words
        if assert_check(c, "marked", want, (params, words, order), lambda v: (v,)):
            assert c.unique_state_count() == want["unique"]
            made += c.discovery("marked") is not None
    assert made >= 4  # lassos, found by the pass (the terminal one may be the search's own in FAST order)


def test_discovery_buffers_regrow(monkeypatch):
    # a witness longer than the first buffers of discovery() / discovery_fingerprints()
    params = (16, 3, 7, 4, 0, 1)
    c = spawn(LiveGraph(*params))
    whole, fps = c.discovery("marked"), c.discovery_fingerprints("marked")
    assert len(whole) == 614 and len(fps) == 615
    monkeypatch.setattr(sr.GpuBfsChecker, "PATH_BUFFER", 7)
    assert c.discovery("marked") == whole and c.discovery_fingerprints("marked") == fps
    assert assert_check(c, "marked", live_graph_ref(params), params, lambda v: (v,))


def test_a_caller_with_the_old_struct_size_has_the_option_off():
    # sr_opts was 56 bytes with 4 bytes of tail padding; whatever they and the bytes behind them hold,
    # a struct_size of 56 is read as liveness = 0
    import ctypes
    b = dgraph(FIXME_CYCLE).checker().complete_liveness()
    b._opts.reserved0 = -1
    b._opts.struct_size = 56
    c = b.spawn_bfs().join()
    assert c.discovery("odd") is None and c.liveness("odd")["ran"] == 0
    b._opts.struct_size = ctypes.sizeof(N.sr_opts)
    assert b.spawn_bfs().join().liveness("odd")["ran"] == 1
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        b.target_state_count(5).spawn_bfs()
    b._opts.struct_size = 56
    b.spawn_bfs().join()  # (nor does such a caller meet the option's refusals)


# ---- the reference's DGraph fixture ---------------------------------------------------------------

@pytest.mark.parametrize("order", ["fifo", "fast", "dfs"])
def test_fixme_graphs_give_the_paths_the_reference_asks_for(order):
    # src/checker.rs:400-413
    c = spawn(dgraph(FIXME_CYCLE), order)
    assert c.discovery("odd").into_states() == [(0,), (2,), (4,), (2,)] and c.loop_start("odd") == 1
    assert assert_check(c, "odd", live_ref.check(*live_ref.dgraph(FIXME_CYCLE)), FIXME_CYCLE, lambda v: (v,))
    c = spawn(dgraph(FIXME_JOIN), order)
    want = live_ref.check(*live_ref.dgraph(FIXME_JOIN))
    if assert_check(c, "odd", want, FIXME_JOIN, lambda v: (v,)):  # (FAST order may find the join's other side itself)
        assert c.discovery("odd").into_states() == [(0,), (2,), (4,), (6,)] and c.loop_start("odd") is None
    if order == "fifo":
        assert c.liveness("odd")["ran"] == 1


def test_can_validate_graphs_have_no_discovery():
    for paths in [CAN_VALIDATE] + [[p] for p in CAN_VALIDATE]:
        c = spawn(dgraph(paths))
        assert assert_check(c, "odd", live_ref.check(*live_ref.dgraph(paths)), paths, lambda v: (v,))
        c.assert_properties()


def test_random_dgraphs():
    rng = random.Random(1234 + EVENTUALLY)
    ran = 0
    for _ in range(60):
        paths = random_graph(rng)
        ran += assert_check(spawn(dgraph(paths)), "odd", live_ref.check(*live_ref.dgraph(paths)), paths, lambda v: (v,))
    assert ran >= 20


# ---- ping-pong: wide states (9 and 17 words), fingerprint mode ----------------------------------------

def host_want(model, p):
    h = N.liveness_host(model.MODEL_ID, model.params(), prop=p)
    w = None
    if h["init_index"] >= 0:
        w = {"init_index": h["init_index"], "actions": h["actions"], "loop_start": h["loop_start"], "states": None}
    return {"unique": h["unique"], "not_p_states": h["not_p_states"], "surviving": h["surviving"], "witness": w}


# the CPU list (tests/test_liveness_host.py), and max_nat 8: the 17-word encoding
PINGPONG_CASES = [(n, lossy, dup) for n in (1, 3, 5) for lossy in (False, True) for dup in (False, True)] + [(8, False, True)]


@pytest.mark.parametrize("max_nat,lossy,duplicating", PINGPONG_CASES)
def test_ping_pong_matches_the_host_answer(max_nat, lossy, duplicating):
    model = sr.PingPong(max_nat, lossy=lossy, duplicating=duplicating)
    c = spawn(model)
    off = spawn(model, on=False)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (off.unique_state_count(), off.state_count(), off.max_depth())
    assert c.stats()["words_per_state"] == (9 if max_nat <= 7 else 17)
    names = [n for n, _ in c.properties()]
    for p in PINGPONG_EVENTUALLY:
        assert c.properties()[p][1] == sr.Expectation.Eventually
        assert_check(c, names[p], host_want(model, p), (max_nat, lossy, duplicating, p), off=off)


# ---- the option off: nothing changes ----------------------------------------------------------------

def test_option_off_changes_nothing():
    for paths in (FIXME_CYCLE, FIXME_JOIN):
        off = spawn(dgraph(paths), on=False)
        plain = dgraph(paths).checker().spawn_bfs().join()
        assert off.discovery("odd") is None and plain.discovery("odd") is None
        assert off.liveness("odd")["ran"] == 0 and off.loop_start("odd") is None
        on = spawn(dgraph(paths))
        counts = (plain.unique_state_count(), plain.state_count(), plain.max_depth())
        assert (off.unique_state_count(), off.state_count(), off.max_depth()) == counts
        assert (on.unique_state_count(), on.state_count(), on.max_depth()) == counts
    params = (12, 2, 3, 2, 0, 1)
    off, on = spawn(LiveGraph(*params), on=False), spawn(LiveGraph(*params))
    assert off.discovery("marked") is None and off.liveness("marked")["ran"] == 0 and off.is_done()
    assert (off.unique_state_count(), off.state_count(), off.max_depth()) == (
        on.unique_state_count(), on.state_count(), on.max_depth())
    assert off.unique_state_count() == live_graph_ref(params)["unique"]


def test_assert_discovery_accepts_a_lasso_only_with_the_option_on():
    # 0 -> 6 is a terminal counterexample the search finds itself; 0 -> 2 -> 4 -> 2 closes a loop
    paths = [[0, 2, 4, 2], [0, 6]]
    off = spawn(dgraph(paths), on=False)
    off.assert_discovery("odd", [6])
    with pytest.raises(AssertionError, match="is nonterminal"):
        off.assert_discovery("odd", [2, 4, 2])
    on = spawn(dgraph(paths))
    assert on.liveness("odd")["ran"] == 0  # the search's own discovery is kept
    on.assert_discovery("odd", [6])
    on.assert_discovery("odd", [2, 4, 2])
    with pytest.raises(AssertionError, match="closes no loop"):
        on.assert_discovery("odd", [2, 4])


# ---- what the option cannot be combined with ----------------------------------------------------------

def test_refusals():
    b = dgraph(FIXME_CYCLE).checker().complete_liveness()
    with pytest.raises(sr.CheckerError, match="liveness with a partitioned search"):
        b.partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        dgraph(FIXME_CYCLE).checker().complete_liveness().target_state_count(10).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with symmetry"):
        sr.TwoPhaseSys(3).checker().complete_liveness().symmetry_canonical().spawn_bfs()
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    with pytest.raises(sr.CheckerError, match="liveness with a plugin model"):
        puzzle.model(1, 4, 2, 3, 5, 8, 6, 7, 0).checker().complete_liveness().spawn_bfs()
    with pytest.raises(sr.CheckerError, match=r"more than 2\^32 - 1 unique states"):
        dgraph(FIXME_CYCLE).checker().complete_liveness().capacity_hint(2 ** 32).spawn_bfs()
    # a model without an `eventually` property: the option is accepted and the pass has nothing to do
    c = sr.TwoPhaseSys(3).checker().complete_liveness().spawn_bfs().join()
    c.assert_properties()
    assert all(c.liveness(n)["ran"] == 0 for n, _ in c.properties())
