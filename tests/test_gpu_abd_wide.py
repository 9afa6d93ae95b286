"""The ABD register past 3 clients / 3 servers on the GPU (stateright_amd/csrc/abd_wide.hpp: 16 or
32 network slots, the history in the state) against the CPU oracle (oracle/actor.hpp AbdSys), and
the encoding-overflow error (kernels.hpp ERR_MODEL): a state whose network does not fit its slots
ends the check with SR_ERR_UNSUPPORTED instead of counts that only look exact."""
import json
import os

import pytest

from actor_golden import ABD, ABD_VALUE_CHOSEN_PATH
from oracle_lib import OracleRun, replay

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")

SR_ERR_UNSUPPORTED = -4
FAULT = "abd: a state exceeded its encoding (network slots)"
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abd_counts.json")) as _f:
    GOLDEN = {(r["client_count"], r["server_count"]): r for r in json.load(_f)["cases"]}

_oracle = {}


def oracle(params, **kw):
    key = (tuple(params), tuple(sorted(kw.items())))
    if key not in _oracle:
        _oracle[key] = OracleRun(ABD, params, **kw)
    return _oracle[key]


def counts(c):
    return c.unique_state_count(), c.state_count(), c.max_depth()


@pytest.fixture(autouse=True)
def no_override(monkeypatch):
    monkeypatch.delenv("SR_ABD_SLOTS", raising=False)


# ---- (1, 4): the smallest shape on the new server layout (three peers: the shared response / acks
# bits) and on the 16-slot network (6 envelopes) ----

@pytest.mark.parametrize("order", ["fifo", "fast", "auto"])
def test_1_4_counts_match_oracle(order):
    o = oracle([1, 4])
    c = sr.AbdRegister(1, 4).checker().order(order).spawn_bfs().join()
    assert counts(c) == (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()
    assert c.is_done() == o.is_done


def test_1_4_fifo_visits_and_path_identical():
    o = oracle([1, 4], record_visits=True)
    rec = sr.StateRecorder()
    c = sr.AbdRegister(1, 4).checker().order("fifo").visitor(rec).spawn_bfs().join()
    assert rec.states == o.visits()
    assert c.discovery("value chosen").action_ids == o.discovery_actions("value chosen")
    assert c.discovery("value chosen").states == o.discovery_states("value chosen")


@pytest.mark.parametrize("order", ["fast", "fifo"])
def test_1_4_on_32_slots(order, monkeypatch):
    # a full-space check of the 32-slot instantiation (its descriptions are 16 values wider than
    # the oracle's: counts only)
    monkeypatch.setenv("SR_ABD_SLOTS", "32")
    o = oracle([1, 4])
    c = sr.AbdRegister(1, 4).checker().order(order).spawn_bfs().join()
    assert counts(c) == (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()


@pytest.mark.parametrize("parts", [2, 3])
def test_1_4_partitioned(parts, monkeypatch):
    monkeypatch.setenv("SR_HEAD_MAX", "0")  # partitioned from level 0 (no replicated head)
    o = oracle([1, 4])
    c = sr.AbdRegister(1, 4).checker().partitions(parts).spawn_bfs().join()
    assert counts(c) == (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()


# ---- (4, 2): the smallest 4-client space that is not degenerate ((4, 1) has 5 states), against
# the oracle's recorded counts (the oracle needs half a minute on 16 threads for it) ----

@pytest.mark.parametrize("order", ["fast", "fifo"])
def test_4_2_counts_and_path(order):
    g = GOLDEN[(4, 2)]
    c = sr.AbdRegister(4, 2).checker().order(order).spawn_bfs().join()
    assert counts(c) == (g["unique_state_count"], g["state_count"], g["max_depth"])
    assert sorted(c.discoveries()) == g["discoveries"]
    c.assert_properties()
    _, holds = replay(ABD, [4, 2], c.discovery("value chosen").action_ids)
    assert holds[1] == 1


# ---- prefixes of the larger spaces (the reference's target_state_count stop), 16 and 32 slots ----

PREFIX = [([c, s], t) for c, s in [(6, 2), (2, 3), (3, 3), (2, 4), (4, 3), (3, 4)] for t in (20_000, 200_000)] + \
    [([4, 3], 1_000_000)]


@pytest.mark.parametrize("params,target", PREFIX, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_prefix_matches_oracle(params, target):
    o = oracle(params, target=target)
    c = sr.AbdRegister(*params).checker().order("auto").target_state_count(target).spawn_bfs().join()
    assert (c.unique_state_count(), c.state_count()) == (o.unique_state_count, o.state_count)
    assert c.is_done() == o.is_done


# ---- the hook: (2, 3) needs 10 slots; forced onto 8 the check ends with an ordinary error ----

def run_8_slots_on_2_3(build):
    c = build(sr.AbdRegister(2, 3).checker()).spawn_bfs()
    with pytest.raises(sr.CheckerError) as e:
        c.join()
    assert e.value.code == SR_ERR_UNSUPPORTED
    assert FAULT in str(e.value)
    assert c.stats()["restarts"] == 0


@pytest.mark.parametrize("order", ["fast", "fifo"])
def test_overflow_ends_the_check(order, monkeypatch):
    monkeypatch.setenv("SR_ABD_SLOTS", "8")
    run_8_slots_on_2_3(lambda ch: ch.order(order))
    monkeypatch.delenv("SR_ABD_SLOTS")
    assert sr.AbdRegister(2, 2).checker().order(order).spawn_bfs().join().unique_state_count() == 544


@pytest.mark.parametrize("head", ["default", "0"])
def test_overflow_ends_the_partitioned_check(head, monkeypatch):
    if head != "default":
        monkeypatch.setenv("SR_HEAD_MAX", head)  # partitioned from level 0 (no replicated head)
    monkeypatch.setenv("SR_ABD_SLOTS", "8")
    run_8_slots_on_2_3(lambda ch: ch.partitions(2))
    monkeypatch.delenv("SR_ABD_SLOTS")
    assert sr.AbdRegister(2, 2).checker().partitions(2).spawn_bfs().join().unique_state_count() == 544


# ---- the configurations that keep the 8-slot encoding ----

def test_2_2_unchanged():
    from stateright_amd.plugin import model_fingerprint
    m = sr.AbdRegister(2, 2)
    c = m.checker().order("fifo").spawn_bfs().join()
    assert c.unique_state_count() == 544
    c.assert_properties()
    c.assert_discovery("value chosen", ABD_VALUE_CHOSEN_PATH)
    init = c.discovery("value chosen").states[0]
    assert len(init) == 4 * 10 + 4 + 2 + 16  # the 8-slot encoding describes 16 envelopes, as ever
    assert model_fingerprint(m, list(init)) == c.discovery_fingerprints("value chosen")[0]
