"""The distinct-state count of the simulation checker on the GPU (spawn_simulation(count_unique=True),
csrc/kernels_sim.hpp simulate_walks<M, REFILL, LOOPS, true>: an insert per visited state into a
table in HBM) against the host form of the same definition (sr_sim_unique_host, csrc/sim.hpp
"Distinct-state count", run without a device)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sr = pytest.importorskip("stateright_amd")

from stateright_amd import _native as N  # noqa: E402
from stateright_amd.checker import CheckerError  # noqa: E402
from stateright_amd.models import LiveGraph  # noqa: E402
from stateright_amd.plugin import model_fingerprint  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240607
SOMETIMES = N.SR_SOMETIMES
# seven even nodes, one init state: a tail into the cycle 2 4 6, a longer way round it, an exit to 12;
# `sometimes "odd"` is never discovered on it
EVEN = [[0, 2, 4, 6, 2], [0, 2, 4, 8, 10, 2], [0, 2, 4, 6, 12]]

MODELS = {
    "2pc3": lambda: sr.TwoPhaseSys(3),                       # one packed word: the count is exact
    "live4": lambda: LiveGraph(9, 2, 5, 7, 11, 3, words=4),  # 512 nodes with cycles on four words
    "paxos1": lambda: sr.Paxos(1),                           # a wide state: 64-bit hashes
    "even": lambda: sr.DGraph(SOMETIMES, EVEN),
}


@functools.lru_cache(maxsize=None)
def host_set(name, w0, n, depth, loops=False):
    m = MODELS[name]()
    return N.sim_unique_host(m.MODEL_ID, m.params(), SEED, w0, n, depth, loops)


def simulate(name, walks, depth, **kw):
    kw.setdefault("count_unique", True)
    return MODELS[name]().checker().spawn_simulation(SEED, walks=walks, max_depth=depth, **kw).join()


def outcome(c):
    """What the mode must leave alone: records, loop starts, hits, discoveries, counts."""
    return (tuple(a.tolist() for a in c.walk_records_arrays()), c.walk_loop_starts().tolist(),
            [c.hit(name) for name, _ in c.properties()], sorted(c.discoveries()), c.state_count(), c.max_depth(),
            c.stats()["levels"], c.is_done())


# ---- 4. the device's set is the host form's ----------------------------------------------------

@pytest.mark.parametrize("name,walks,depth,loops", [("2pc3", 4096, 64, False), ("2pc3", 4096, 64, True),
                                                     ("live4", 4096, 64, False), ("live4", 4096, 64, True),
                                                     ("paxos1", 4096, 64, False)])
def test_device_set_equals_host_set(name, walks, depth, loops):
    want = host_set(name, 0, walks, depth, loops)
    on = simulate(name, walks, depth, record_walks=True, detect_loops=loops)
    off = simulate(name, walks, depth, record_walks=True, detect_loops=loops, count_unique=False)
    ran = len(on.walk_records_arrays()[0])  # (a check stops after the batch in which every property is discovered)
    assert ran == walks
    got = on.unique_fingerprints()
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    info = on.unique_info()
    assert on.unique_state_count() == len(want) == info["unique"] and (info["on"], info["overflow"], info["stopped_stale"]) == (1, 0, 0)
    assert info["capacity"] == min(walks * (depth + 1), 2**28) and info["slots"] == 2 ** 20  # the least power of two >= 2 C
    assert on.batch_new_states() == [len(want)]
    assert 1 < len(want) < on.state_count()
    if name == "live4":
        assert (on.walk_records_arrays()[1] == N.SIM_LOOP).any() == loops
    # the mode feeds nothing back
    assert outcome(on) == outcome(off)
    assert off.unique_state_count() == off.state_count() == on.state_count()


# ---- 5. the set lies inside the reachable set --------------------------------------------------

def test_2pc3_set_is_inside_what_bfs_visits():
    m = sr.TwoPhaseSys(3)
    rec = sr.StateRecorder()
    b = m.checker().visitor(rec).spawn_bfs().join()
    truth = {model_fingerprint(m, list(s)) for s in rec.states}
    assert len(truth) == b.unique_state_count() == 288
    c = simulate("2pc3", 4096, 64)
    got = set(c.unique_fingerprints().tolist())
    assert got <= truth and len(got) == c.unique_state_count() <= 288


# ---- 6. the launch shape does not matter -------------------------------------------------------

def test_set_and_batch_counts_do_not_depend_on_the_launch_shape(monkeypatch):
    walks, depth = 1000, 48
    want = host_set("2pc3", 0, walks, depth)
    monkeypatch.setenv("SR_SIM_REFILL", "0")
    whole = simulate("2pc3", walks, depth)
    assert np.array_equal(whole.unique_fingerprints(), want) and whole.batch_new_states() == [len(want)]
    # per batch of 64: what the host form's sets grow by
    sizes = [len(host_set("2pc3", 0, min(walks, 64 * (b + 1)), depth)) for b in range(-(-walks // 64))]
    per_batch = [s - p for s, p in zip(sizes, [0] + sizes)]
    assert sum(per_batch) == len(want) and per_batch[0] > 0
    monkeypatch.setenv("SR_SIM_BATCH", "64")
    for refill, grid in (("0", "0"), ("1", "1"), ("1", "0")):  # static; one workgroup refilling; the default grid
        monkeypatch.setenv("SR_SIM_REFILL", refill)
        monkeypatch.setenv("SR_SIM_GRID", grid)
        c = simulate("2pc3", walks, depth)
        assert c.stats()["levels"] == len(per_batch) == 16, (refill, grid)
        assert np.array_equal(c.unique_fingerprints(), want), (refill, grid)
        assert c.batch_new_states() == per_batch and sum(c.batch_new_states()) == c.unique_state_count(), (refill, grid)
    # one workgroup refilling over ONE batch of 1000: its 256 lanes carry four walks each
    monkeypatch.setenv("SR_SIM_BATCH", "1000")
    monkeypatch.setenv("SR_SIM_REFILL", "1")
    monkeypatch.setenv("SR_SIM_GRID", "1")
    for loops in (False, True):
        c = simulate("2pc3", walks, depth, detect_loops=loops)
        assert np.array_equal(c.unique_fingerprints(), host_set("2pc3", 0, walks, depth, loops)), loops
        assert c.batch_new_states() == [c.unique_state_count()], loops


# ---- 7. high load and overflow (tables of at most 1024 slots: a probe covers the whole table) ---

def test_a_capacity_of_exactly_the_set_is_exact():
    want = host_set("2pc3", 0, 4096, 64)
    off = simulate("2pc3", 4096, 64, record_walks=True, count_unique=False)
    for cap in (len(want), (len(want) + 1) // 2):  # load <= 0.5, and a table the set nearly fills
        c = simulate("2pc3", 4096, 64, record_walks=True, unique_capacity=cap)
        info = c.unique_info()
        slots = 2
        while slots < 2 * cap:
            slots *= 2
        assert (info["capacity"], info["slots"], info["overflow"]) == (cap, slots, 0) and len(want) <= slots <= 1024
        assert np.array_equal(c.unique_fingerprints(), want) and c.unique_state_count() == len(want)
        assert outcome(c) == outcome(off)


def test_a_table_too_small_overflows_and_is_full(monkeypatch):
    off = simulate("2pc3", 4096, 64, record_walks=True, count_unique=False)
    for refill in ("0", "1"):
        monkeypatch.setenv("SR_SIM_REFILL", refill)
        c = simulate("2pc3", 4096, 64, record_walks=True, unique_capacity=8)  # join() succeeds
        info = c.unique_info()
        assert (info["overflow"], info["slots"], info["unique"], info["stopped_stale"]) == (1, 16, 16, 0)
        assert c.unique_state_count() == 16 and sum(c.batch_new_states()) == 16
        got = c.unique_fingerprints()
        assert len(got) == 16 and set(got.tolist()) <= set(host_set("2pc3", 0, 4096, 64).tolist())
        assert outcome(c) == outcome(off)
        assert sorted(c.discoveries()) == ["abort agreement", "commit agreement"]


# ---- 8. until_stale ----------------------------------------------------------------------------

def test_until_stale_stops_after_k_batches_without_a_new_state(monkeypatch):
    monkeypatch.setenv("SR_SIM_BATCH", "64")
    depth, k = 40, 2
    # from the host form: the batch at whose end k batches in a row added nothing
    sizes, stale, batches = [0], 0, 0
    while stale < k:
        batches += 1
        sizes.append(len(host_set("even", 0, 64 * batches, depth)))
        stale = stale + 1 if sizes[-1] == sizes[-2] else 0
        assert batches < 100
    c = simulate("even", None, depth, until_stale=k)
    info = c.unique_info()
    assert (info["stopped_stale"], info["batches"], info["overflow"]) == (1, batches, 0)
    assert c.stats()["levels"] == batches and c.state_count() > 64 * batches
    assert c.batch_new_states() == [b - a for a, b in zip(sizes, sizes[1:])] and c.batch_new_states()[-k:] == [0] * k
    assert c.unique_state_count() == sizes[-1] == 7
    assert np.array_equal(c.unique_fingerprints(), host_set("even", 0, 64 * batches, depth))
    # a run stopped this way still proves nothing
    assert not c.is_done() and not c.discoveries()
    with pytest.raises(AssertionError, match="model checking is incomplete"):
        c.assert_no_discovery("odd")
    # walks still bound the check when they run out first
    c = simulate("even", 64, depth, until_stale=k)
    assert (c.unique_info()["stopped_stale"], c.stats()["levels"]) == (0, 1)


def test_until_stale_fails_on_an_overflow(monkeypatch):
    monkeypatch.setenv("SR_SIM_BATCH", "64")
    with pytest.raises(CheckerError, match="overflowed") as e:
        simulate("2pc3", None, 64, until_stale=2, unique_capacity=8)
    assert e.value.code == -3  # SR_ERR_CAPACITY


# ---- 9. mode off -------------------------------------------------------------------------------

def test_mode_off_is_as_before():
    c = simulate("2pc3", 1000, 48, count_unique=False)
    info = c.unique_info()
    assert (info["on"], info["unique"], info["overflow"], info["slots"], info["capacity"], info["stopped_stale"]) == (0,) * 6
    assert info["batches"] == c.stats()["levels"] == 1
    assert c.unique_state_count() == c.state_count() > 1000
    assert c.batch_new_states() == []
    with pytest.raises(CheckerError, match="without sr_sim_opts.unique"):
        c.unique_fingerprints()
