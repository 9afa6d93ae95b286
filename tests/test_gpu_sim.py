"""The simulation checker on the GPU (CheckerBuilder.spawn_simulation, csrc/kernels_sim.hpp) against
the host walk (sr_sim_walk: the same definition, csrc/sim.hpp, run without a device)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sr = pytest.importorskip("stateright_amd")

from oracle_lib import dgraph_params  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd import build  # noqa: E402
from stateright_amd.models import Ladder  # noqa: E402
from stateright_amd.plugin import Plugin  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240607  # its host walks find every discovery asserted by name below (checked on the CPU)
EVENTUALLY, SOMETIMES = N.SR_EVENTUALLY, N.SR_SOMETIMES
DG_A = [[0, 1, 4, 6], [2, 4, 8]]
DG_B = [[0, 1], [0, 2]]

MODELS = {
    "2pc3": lambda: sr.TwoPhaseSys(3),
    "2pc5": lambda: sr.TwoPhaseSys(5),
    "increment2": lambda: sr.Increment(2),
    "increment_lock3": lambda: sr.IncrementLock(3),
    "linear_equation": lambda: sr.LinearEquation(2, 10, 14),
    "binary_clock": lambda: sr.BinaryClock(),
    "ladder": lambda: Ladder(3, 2),
    "paxos2": lambda: sr.Paxos(2),
    "pingpong1": lambda: sr.PingPong(1),
    "pingpong5": lambda: sr.PingPong(5),
    "dgraph_a": lambda: sr.DGraph(SOMETIMES, DG_A),
    "dgraph_b": lambda: sr.DGraph(EVENTUALLY, DG_B),
}


def host_walk(model, i, depth, nprops=8):
    return N.sim_walk(model.MODEL_ID, model.params(), SEED, i, depth, nprops)


@functools.lru_cache(maxsize=None)
def host_reference(name, walks, depth):
    """(steps, end, fp) arrays and the per-walk first hits of walks 0 .. walks-1, computed once."""
    m = MODELS[name]()
    ws = [host_walk(m, i, depth) for i in range(walks)]
    return (np.array([w["steps"] for w in ws], dtype=np.uint32), np.array([w["end"] for w in ws], dtype=np.uint32),
            np.array([w["final_fp"] for w in ws], dtype=np.uint64), [w["first_hit"] for w in ws])


def simulate(model, walks, depth, record=True, **kw):
    b = model.checker()
    if "target" in kw:
        b = b.target_state_count(kw["target"])
    return b.spawn_simulation(SEED, walks=walks, max_depth=depth, record_walks=record).join()


# ---- device equals host ------------------------------------------------------------------------

# The persistent form hands out, through its cursor, only the indices past its grid's lanes. Its grid
# is capped by the compute units (262 144 lanes on a 256-CU part), far above these batches, so the
# tests cap it themselves (SR_SIM_GRID, in workgroups of 256 lanes): with one workgroup every walk
# past index 255 is one a lane took after its previous walk ended.
@pytest.mark.parametrize("refill", ["0", "1"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_walks_equal_host_walks(name, refill, monkeypatch):
    monkeypatch.setenv("SR_SIM_REFILL", refill)
    monkeypatch.setenv("SR_SIM_GRID", "1")
    depth = 48
    steps, end, fp, _ = host_reference(name, 1000, depth)
    for walks in (1, 63, 64, 65, 1000):
        c = simulate(MODELS[name](), walks, depth)
        if c.is_done():  # every property discovered: the check stopped after its first (only) batch
            assert c.stats()["levels"] == 1
        ds, de, df = c.walk_records_arrays()
        assert len(ds) == walks
        assert np.array_equal(ds, steps[:walks]) and np.array_equal(de, end[:walks]) and np.array_equal(df, fp[:walks])
        assert c.state_count() == int(steps[:walks].astype(np.int64).sum()) + walks
        assert c.max_depth() == int(steps[:walks].max())
        assert c.unique_state_count() == c.state_count()
        st = c.stats()
        assert st["successors"] == c.state_count() - walks and st["levels"] == st["expand_launches"] == 1


# ---- refill and batches ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["2pc3", "ladder"])
def test_records_do_not_depend_on_batch_size_or_form(name, monkeypatch):
    walks, depth = 200_000, 32
    runs = {}
    # 3 batches (none a multiple of 64) and 4; the static form, and the persistent form on grids of
    # 7 workgroups (1 792 lanes: ~39 walks per lane and batch), of 100 (25 600 lanes: the last
    # reservations of a batch straddle its end) and of the compute units' cap (no refill at these sizes)
    for batch in (70_001, 65_536):
        for refill, grid in (("0", "0"), ("1", "7"), ("1", "100"), ("1", "0")):
            monkeypatch.setenv("SR_SIM_BATCH", str(batch))
            monkeypatch.setenv("SR_SIM_REFILL", refill)
            monkeypatch.setenv("SR_SIM_GRID", grid)
            c = simulate(MODELS[name](), walks, depth)
            assert c.stats()["levels"] == -(-walks // batch) >= 3  # never stops early: nothing is discovered
            assert not c.is_done()
            runs[batch, refill, grid] = c.walk_records_arrays() + (c.state_count(), c.max_depth())
    first = runs[70_001, "0", "0"]
    assert len(first[0]) == walks
    for key, r in runs.items():
        for a, b in zip(first[:3], r[:3]):
            assert np.array_equal(a, b), key
        assert r[3:] == first[3:], key
    # a fixed sample of 2 000 indices, the first and last of every batch of either size among them
    edges = {i for batch in (70_001, 65_536) for b0 in range(0, walks, batch) for i in (b0, min(b0 + batch, walks) - 1)}
    rng = np.random.default_rng(7)
    sample = sorted(edges | set(rng.choice(walks, 2000 - len(edges), replace=False).tolist()))
    m = MODELS[name]()
    for i in sample:
        w = host_walk(m, i, depth)
        assert (int(first[0][i]), int(first[1][i]), int(first[2][i])) == (w["steps"], w["end"], w["final_fp"]), i
    assert first[3] == int(first[0].astype(np.int64).sum()) + walks


# ---- discoveries -------------------------------------------------------------------------------

DISCOVERIES = {
    "2pc3": {"abort agreement", "commit agreement"},
    "increment2": {"fin"},
    "dgraph_b": {"odd"},
}


@pytest.mark.parametrize("name", sorted(DISCOVERIES))
def test_discoveries_are_the_host_walks_minimum(name):
    walks, depth = 4096, 64
    c = simulate(MODELS[name](), walks, depth, record=False)
    ran = walks  # one batch: a launch's step budget holds far more than 4 096 walks of depth 64
    assert c.stats()["levels"] == 1
    m = MODELS[name]()
    props = c.properties()
    best = [None] * len(props)
    for i in range(ran):
        for p, t in enumerate(host_walk(m, i, depth, len(props))["first_hit"]):
            if t >= 0 and (best[p] is None or (t, i) < best[p]):
                best[p] = (t, i)
    found = {props[p][0] for p in range(len(props)) if best[p] is not None}
    assert found == DISCOVERIES[name]
    assert set(c.discoveries()) == found
    for p, (pname, exp) in enumerate(props):
        assert c.hit(pname) == best[p]
        path = c.discovery(pname)
        if best[p] is None:
            assert path is None
            continue
        step, walk = best[p]
        assert len(path) == step
        assert path.action_ids == host_walk(m, walk, depth)["actions"][:step]
        assert len(c.discovery_fingerprints(pname)) == step + 1
        states, conds = c.replay(path.into_actions())
        assert [tuple(s) for s in states] == path.into_states()
        if exp == sr.Expectation.Always:
            assert not conds[p]
        elif exp == sr.Expectation.Sometimes:
            assert conds[p]
        else:
            per_state, terminal = c.replay_trace(path.into_actions())
            assert terminal and not any(s[p] for s in per_state)
        c.assert_discovery(pname, path.into_actions())


# ---- no false discovery ------------------------------------------------------------------------

@pytest.mark.parametrize("name,prop", [("paxos2", "linearizable"), ("2pc5", "consistent")])
def test_no_false_discovery(name, prop):
    c = simulate(MODELS[name](), 50_000, 64, record=False)
    assert c.discovery(prop) is None and c.hit(prop) is None
    assert prop not in c.discoveries()
    assert not c.is_done()
    with pytest.raises(AssertionError, match="model checking is incomplete"):
        c.assert_no_discovery(prop)


# ---- stopping ----------------------------------------------------------------------------------

def test_target_state_count_stops_at_the_first_whole_batch_that_reaches_it(monkeypatch):
    monkeypatch.setenv("SR_SIM_BATCH", "1000")
    # every BinaryClock walk of depth 9 visits 10 states: 10 000 per batch
    c = simulate(sr.BinaryClock(), None, 9, record=False, target=25_000)
    assert c.state_count() == 30_000 >= 25_000
    assert c.stats()["levels"] == 3
    assert not c.is_done()
    c = simulate(sr.BinaryClock(), 1500, 9, record=False, target=25_000)  # the walks run out first
    assert (c.state_count(), c.stats()["levels"]) == (15_000, 2)


def test_stops_after_the_first_batch_with_every_property_discovered(monkeypatch):
    monkeypatch.setenv("SR_SIM_BATCH", "64")
    c = simulate(sr.DGraph(SOMETIMES, DG_B), 10_000, 64)
    assert c.is_done() and c.stats()["levels"] == 1
    assert len(c.walk_records()) == 64 and c.state_count() == 128
    assert c.hit("odd")[0] == 1
    c.assert_properties()


# ---- refusals ----------------------------------------------------------------------------------

def test_refusals():
    with pytest.raises(ValueError, match="visitor"):
        sr.TwoPhaseSys(3).checker().visitor(sr.StateRecorder()).spawn_simulation(1, walks=10)
    with pytest.raises(ValueError, match="partition"):
        sr.TwoPhaseSys(3).checker().partitions(2).spawn_simulation(1, walks=10)
    with pytest.raises(ValueError, match="symmetry"):
        sr.TwoPhaseSys(3).checker().symmetry_canonical().spawn_simulation(1, walks=10)
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    with pytest.raises(ValueError, match="plugin"):
        puzzle.model(1, 4, 2, 3, 5, 8, 6, 7, 0).checker().spawn_simulation(1, walks=10)
    with pytest.raises(ValueError, match="walks"):
        sr.TwoPhaseSys(3).checker().spawn_simulation(1)
    for depth in (0, -1, 2**20 + 1):
        with pytest.raises(ValueError, match="max_depth"):
            sr.TwoPhaseSys(3).checker().spawn_simulation(1, walks=10, max_depth=depth)
    # the C ABI refuses the same on its own
    so = N.sr_sim_opts()
    N.load().sr_sim_opts_init_sized(so, 4096)
    assert so.struct_size == ctypes.sizeof(N.sr_sim_opts) and so.max_depth == 4096
    arr = (ctypes.c_int64 * 1)(3)
    assert not N.load().sr_gpu_sim_spawn(N.SR_MODEL_2PC, arr, 1, so)
    assert "walks or target_state_count" in N.last_error()
