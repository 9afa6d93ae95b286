"""expand_fast's action table on the GPU (kernels.hpp ActionTable; models with `action_masks`):
2pc and the Ladder fixture with the table (SR_ACTION_TABLE unset) and with `apply` (=0), in the probe
rounds and in the per-lane probe queues. 2pc's counts, depth and discoveries must equal the CPU
oracle's and its FAST discovery paths must replay on the CPU model; the Ladder's unique count is
(K + 1) * 2^F and everything else must be equal between the two settings. Ladder(58, 4) has 62 slots
(the table), Ladder(58, 8) has 66 (past one slot per lane: `apply`); Ladder(2, 19) at 64 parents per
wave fills more than one window of a wave's successor map."""
import math

import pytest

from stateright_amd import models as sr
from oracle_lib import TWO_PHASE, replay
from test_gpu_parity import gpu, oracle

pytestmark = pytest.mark.gpu

KNOBS = [None, "0"]  # SR_ACTION_TABLE


def set_knob(monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv("SR_ACTION_TABLE", raising=False)
    else:
        monkeypatch.setenv("SR_ACTION_TABLE", knob)


def check_two_phase(n, order):
    o = oracle(TWO_PHASE, [n])
    c, _ = gpu(TWO_PHASE, [n], order)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == \
        (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()
    if order == "fast":
        props = c.properties()
        for name, path in c.discoveries().items():
            assert replay(TWO_PHASE, [n], path.action_ids, n_props=len(props)) is not None, \
                f"{name}: path does not replay on the CPU model"
    return c


@pytest.mark.parametrize("knob", KNOBS, ids=["table", "apply"])
@pytest.mark.parametrize("order", ["fast", "auto"])
@pytest.mark.parametrize("n", [1, 3, 5, 7])
def test_two_phase_matches_oracle(n, order, knob, monkeypatch):
    set_knob(monkeypatch, knob)
    c = check_two_phase(n, order)
    if n == 3:
        assert c.unique_state_count() == 288


@pytest.mark.parametrize("knob", KNOBS, ids=["table", "apply"])
@pytest.mark.parametrize("n", [3, 5])
def test_two_phase_probe_queues(n, knob, monkeypatch):
    # the per-lane probe queues (the form of tables past 2^27 slots) apply the table in their phase A
    # and again when they rebuild the new states
    monkeypatch.setenv("SR_PROBE_BATCH", "-4")
    set_knob(monkeypatch, knob)
    check_two_phase(n, "fast")


def ladder(k, f):
    c = sr.Ladder(k, f).checker().order("fast").spawn_bfs().join()
    c.assert_properties()
    return (c.unique_state_count(), c.state_count(), c.max_depth())


@pytest.mark.parametrize("queues", [False, True], ids=["rounds", "queues"])
@pytest.mark.parametrize("f", [4, 8])
def test_ladder_past_64_slots(f, queues, monkeypatch):
    k = 58
    if queues:
        monkeypatch.setenv("SR_PROBE_BATCH", "-4")
    got = {}
    for knob in KNOBS:
        set_knob(monkeypatch, knob)
        got[knob] = ladder(k, f)
        assert got[knob][0] == (k + 1) * 2 ** f
    assert got[None] == got["0"]
    # every state but the last has successors: rung < K gives one, each clear free bit one
    assert got[None][1] == 1 + sum((r < k) + (f - j) for r in range(k + 1) for j in range(f + 1)
                                   for _ in range(math.comb(f, j)))
    assert got[None][2] == k + f  # (the init state has depth 0)


def test_two_phase_ppw64(monkeypatch):
    # 64 parents per wave, the most a wave's successor map is filled from. (2pc N=7 does not reliably
    # pass the 1 024 entries of one map window: its large levels average 4.5-6.8 moves per parent;
    # test_ladder_window_crossing below does.)
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    got = {}
    for knob in KNOBS:
        set_knob(monkeypatch, knob)
        c = check_two_phase(7, "fast")
        got[knob] = (c.unique_state_count(), c.state_count(), c.max_depth())
    assert got[None] == got["0"]


def ladder_levels(k, f):
    """[(parents, least out-degree)] per BFS level of Ladder(k, f): level L holds the states of rung
    r with j free bits set, r + j = L, comb(f, j) of each, with (r < k) + (f - j) successors."""
    out = []
    for level in range(k + f + 1):
        cls = [(math.comb(f, level - r), (r < k) + f - (level - r)) for r in range(k + 1) if 0 <= level - r <= f]
        out.append((sum(n for n, _ in cls), min(d for _, d in cls)))
    return out


def test_ladder_window_crossing(monkeypatch):
    # A wave's successor map is filled in windows of 1 024 entries. With 64 parents per wave, every
    # full wave of a level whose parents all have more than 16 successors fills a second window
    # (w0 > 0): the tail lanes' slot 0, and the queues' rebuild index s0 + 64 r + lane - w0.
    # Ladder(2, 19), 21 slots (the table): level 2 has 191 parents of at least 18 successors,
    # level 3 has 1 159 of at least 17.
    k, f, window = 2, 19, 1024
    levels = ladder_levels(k, f)
    crossing = [n for n, d in levels if n >= 64 and 64 * d > window]
    assert crossing == [191, 1159]
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    successors = sum(math.comb(f, j) * ((r < k) + (f - j)) for r in range(k + 1) for j in range(f + 1))
    want = ((k + 1) * 2 ** f, 1 + successors, k + f)
    # the levels were launched with those frontiers, whole (one launch per level)
    c = sr.Ladder(k, f).checker().order("fast").profile().spawn_bfs().join()
    fronts = [fr for _, fr in c.launch_profile()]
    assert fronts[:len(levels)] == [n for n, _ in levels][:len(fronts)] and len(fronts) >= 4, fronts[:8]
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == want
    for queues in (False, True):
        if queues:
            monkeypatch.setenv("SR_PROBE_BATCH", "-4")
        for knob in KNOBS:
            set_knob(monkeypatch, knob)
            assert ladder(k, f) == want, (queues, knob)
