"""Loop detection of the simulation checker on the GPU (spawn_simulation(detect_loops=True),
csrc/kernels_sim.hpp simulate_walks<M, REFILL, true>) against the host walk in the same mode
(sr_sim_walk_loops: the same definition, csrc/sim.hpp, run without a device)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sr = pytest.importorskip("stateright_amd")

from stateright_amd import _native as N  # noqa: E402
from test_gpu_sim import MODELS as PLAIN_MODELS  # noqa: E402
from test_gpu_sim import SEED  # noqa: E402

pytestmark = pytest.mark.gpu

EVENTUALLY, SOMETIMES = N.SR_EVENTUALLY, N.SR_SOMETIMES
FIXME = [[0, 2, 4, 2]]  # src/checker.rs:400-413
RING12 = [[2 * k for k in range(12)] + [0]]
# two cycles through node 0: 0 2 4 (inside the window) and 0 10 12 .. 30 (11 nodes: beyond it)
SHARED = [[0, 2, 4, 0], [0] + list(range(10, 32, 2)) + [0]]

MODELS = dict(PLAIN_MODELS)
MODELS.update({
    "loop_fixme": lambda: sr.DGraph(EVENTUALLY, FIXME),
    "loop_ring12": lambda: sr.DGraph(EVENTUALLY, RING12),
    "loop_held": lambda: sr.DGraph(EVENTUALLY, [[0, 1, 2, 1]]),
    "loop_two_inits": lambda: sr.DGraph(EVENTUALLY, [[0, 2, 4, 2], [2, 6]]),
    "loop_shared": lambda: sr.DGraph(EVENTUALLY, SHARED),
})


def host_walk(model, i, depth, nprops=8):
    return N.sim_walk(model.MODEL_ID, model.params(), SEED, i, depth, nprops, loops=True)


@functools.lru_cache(maxsize=None)
def host_reference(name, walks, depth):
    """(steps, end, fp, loop_start) arrays of the loop-mode walks 0 .. walks-1, computed once."""
    m = MODELS[name]()
    ws = [host_walk(m, i, depth) for i in range(walks)]
    return (np.array([w["steps"] for w in ws], dtype=np.uint32), np.array([w["end"] for w in ws], dtype=np.uint32),
            np.array([w["final_fp"] for w in ws], dtype=np.uint64), np.array([w["loop_start"] for w in ws], dtype=np.int64))


def simulate(model, walks, depth, record=True, loops=True):
    return model.checker().spawn_simulation(SEED, walks=walks, max_depth=depth, record_walks=record, detect_loops=loops).join()


# ---- 6. device equals host ---------------------------------------------------------------------

# SR_SIM_GRID=1: one workgroup, so in the persistent form every walk past index 255 runs on a lane
# (and an LDS window) that carried another walk before.
@pytest.mark.parametrize("refill", ["0", "1"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_loop_walks_equal_host_loop_walks(name, refill, monkeypatch):
    monkeypatch.setenv("SR_SIM_REFILL", refill)
    monkeypatch.setenv("SR_SIM_GRID", "1")
    depth = 48
    steps, end, fp, start = host_reference(name, 1000, depth)
    if name.startswith("loop_") or name in ("2pc3", "2pc5", "binary_clock"):
        assert (end == N.SIM_LOOP).any()  # (the mode is exercised)
    for walks in (1, 63, 64, 65, 1000):
        c = simulate(MODELS[name](), walks, depth)
        ds, de, df = c.walk_records_arrays()
        dl = c.walk_loop_starts()
        assert len(ds) == len(dl) == walks
        assert np.array_equal(ds, steps[:walks]) and np.array_equal(de, end[:walks]) and np.array_equal(df, fp[:walks])
        assert np.array_equal(dl, start[:walks])
        assert c.state_count() == int(steps[:walks].astype(np.int64).sum()) + walks
        assert c.max_depth() == int(steps[:walks].max())
        assert c.unique_state_count() == c.state_count()


# ---- 7. a lane's next walk never sees its predecessor's window ---------------------------------

def test_no_stale_window_in_the_persistent_form(monkeypatch):
    monkeypatch.setenv("SR_SIM_REFILL", "1")
    monkeypatch.setenv("SR_SIM_GRID", "1")
    # no cycle: every walk is 0 2 4 6. A lane's later walks find their predecessor's fingerprints in
    # the LDS ring; a ring trusted beyond the walk's own t would report a loop at t = 1.
    c = simulate(sr.DGraph(SOMETIMES, [[0, 2, 4, 6]]), 1000, 48)
    ds, de, _ = c.walk_records_arrays()
    assert len(ds) == 1000 and (ds == 3).all() and (de == N.SIM_TERMINAL).all()
    assert (c.walk_loop_starts() == -1).all()
    assert c.state_count() == 4000 and not c.discoveries()


# ---- 8. discoveries ----------------------------------------------------------------------------

def test_the_fixme_lasso_is_discovered():
    c = simulate(sr.DGraph(EVENTUALLY, FIXME), 1000, 48, record=False)
    path = c.discovery("odd")
    assert [s[0] for s in path.into_states()] == [0, 2, 4, 2]
    assert path.action_ids == [2, 4, 2]
    assert c.hit("odd") == (3, 0)
    assert c.loop_start("odd") == 1
    assert len(c.discovery_fingerprints("odd")) == 4
    c.assert_discovery("odd", [2, 4, 2])
    c.assert_discovery("odd", path.into_actions())
    with pytest.raises(AssertionError, match="closes no loop"):
        c.assert_discovery("odd", [2, 4])
    assert c.is_done()
    # without the mode the same check finds nothing, as before
    c = simulate(sr.DGraph(EVENTUALLY, FIXME), 1000, 48, record=False, loops=False)
    assert c.discovery("odd") is None and c.hit("odd") is None and c.loop_start("odd") is None
    assert not c.is_done() and not c.discoveries()


def test_a_ring_beyond_the_window_is_discovered_at_a_checkpoint():
    c = simulate(sr.DGraph(EVENTUALLY, RING12), 100, 48, record=False)
    states = [s[0] for s in c.discovery("odd").into_states()]
    assert len(states) == 29 and states[28] == states[16]
    assert states == [2 * (t % 12) for t in range(29)]
    assert c.loop_start("odd") == 16 and c.hit("odd") == (28, 0)
    c.assert_discovery("odd", states[1:])
    assert c.is_done()


def test_a_terminal_trace_is_still_a_discovery_and_has_no_loop_start():
    c = simulate(sr.DGraph(EVENTUALLY, [[0, 2, 4, 2], [2, 6]]), 1000, 48, record=False)
    assert [s[0] for s in c.discovery("odd").into_states()] == [2, 6]  # t = 1, ahead of every lasso
    assert c.loop_start("odd") is None
    c.assert_discovery("odd", [6])


# ---- 9. batches and forms ----------------------------------------------------------------------

def test_loop_records_do_not_depend_on_batch_size_or_form(monkeypatch):
    walks, depth = 20_000, 32
    runs = {}
    for batch in (7_001, 4_096):
        for refill, grid in (("0", "0"), ("1", "7"), ("1", "100"), ("1", "0")):
            monkeypatch.setenv("SR_SIM_BATCH", str(batch))
            monkeypatch.setenv("SR_SIM_REFILL", refill)
            monkeypatch.setenv("SR_SIM_GRID", grid)
            c = simulate(sr.TwoPhaseSys(3), walks, depth)
            assert c.stats()["levels"] == -(-walks // batch)  # never stops early: "consistent" is never hit
            runs[batch, refill, grid] = c.walk_records_arrays() + (c.walk_loop_starts(), c.state_count(), c.max_depth())
    first = runs[7_001, "0", "0"]
    assert len(first[0]) == walks and (first[1] == N.SIM_LOOP).any() and (first[3] >= 0).any()
    for key, r in runs.items():
        for a, b in zip(first[:4], r[:4]):
            assert np.array_equal(a, b), key
        assert r[4:] == first[4:], key
    m = sr.TwoPhaseSys(3)
    for i in list(range(0, walks, 997)) + [7_000, 7_001, 4_095, 4_096, walks - 1]:
        w = host_walk(m, i, depth)
        assert (int(first[0][i]), int(first[1][i]), int(first[2][i]), int(first[3][i])) == \
            (w["steps"], w["end"], w["final_fp"], w["loop_start"]), i
    assert first[4] == int(first[0].astype(np.int64).sum()) + walks
