"""expand_fast's stage of new states, one region per wave (SR_STAGE_PER_WAVE, kernels.hpp): a wave
appends to its own part of the workgroup's LDS stage, the flush copies the regions out one after the
other, and what does not fit a region goes straight to the next frontier. FAST order must still
find what the CPU oracle finds (counts, depth, discoveries) where the regions are empty, carried
over several chunks, flushed often or overflowing, in every form of the kernel, and the parent
written beside each state at the copy-out must be the state's generator."""
import pytest

from oracle_lib import INCREMENT_LOCK, TWO_PHASE, replay
from test_gpu_parity import gpu, ids, oracle

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")


def check(case, **kw):
    model, params = case
    o = oracle(model, params)
    c, _ = gpu(model, params, "fast", **kw)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == \
        (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()
    return c


def test_levels_smaller_than_a_wave():
    # 2pc N=3 (288 states): every level has fewer parents than a wave, so most regions stay empty
    assert oracle(TWO_PHASE, [3]).unique_state_count == 288
    check((TWO_PHASE, [3]))


@pytest.mark.parametrize("grid", ["1", "2"])
@pytest.mark.parametrize("case", [(TWO_PHASE, [6]), (TWO_PHASE, [8])], ids=ids)
def test_one_workgroup_strides_every_chunk(case, grid, monkeypatch):
    # many flushes, regions carried from chunk to chunk, overflow into direct appends
    monkeypatch.setenv("SR_GRID_MAX", grid)
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    for pipe in ("1", "0"):
        monkeypatch.setenv("SR_PIPELINE", pipe)
        check(case)


@pytest.mark.parametrize("grid", ["1", "2"])
def test_counting_form(grid, monkeypatch):
    monkeypatch.setenv("SR_GRID_MAX", grid)
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    c = check((TWO_PHASE, [6]), counters=True)
    assert c.stats()["probes"] > 0


@pytest.mark.parametrize("grid", ["1", "2"])
def test_queue_form(grid, monkeypatch):
    # the per-lane probe queues append through append_new
    monkeypatch.setenv("SR_GRID_MAX", grid)
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    monkeypatch.setenv("SR_PROBE_BATCH", "-4")
    for pipe in ("1", "0"):
        monkeypatch.setenv("SR_PIPELINE", pipe)
        check((TWO_PHASE, [6]))


@pytest.mark.parametrize("case", [(INCREMENT_LOCK, [8]), (INCREMENT_LOCK, [9])], ids=ids)
def test_every_successor_new(case, monkeypatch):
    # increment_lock: no duplicates, the heaviest load on a region (N=8, one-word states: a chunk
    # makes more states than the regions hold, the rest is appended directly; N=9, two-word states,
    # keeps the stage shared by the waves and overflows it the same way)
    monkeypatch.setenv("SR_GRID_MAX", "1")
    check(case)


def test_default_grid_balanced_levels():
    # 2pc N=7 (296 448 states): levels above 64 K parents run the balanced geometry
    c = check((TWO_PHASE, [7]))
    assert c.stats()["balanced_levels"] > 0


@pytest.mark.parametrize("grid", ["1", None])
def test_every_path_replays(grid, monkeypatch):
    # 2pc N=5 (8 832 states): the path of every state, read from the exported tree of parents,
    # replays on the CPU model and ends in that state at its BFS depth
    n = 5
    if grid:
        monkeypatch.setenv("SR_GRID_MAX", grid)
        monkeypatch.setenv("SR_PPW_LOG2", "6")
    recorder, accessor = sr.PathRecorder.new_with_accessor()
    c = sr.TwoPhaseSys(n).checker().order("fast").visitor(recorder).spawn_bfs().join()
    paths = accessor()
    o = oracle(TWO_PHASE, [n], record_visits=True)
    depth = {s: len(a) for s, a in zip(o.visits(), o.visit_paths())}
    assert len(paths) == c.unique_state_count() == 8_832
    assert {p.last_state() for p in paths} == set(depth)
    for p in paths:
        states, _ = replay(TWO_PHASE, [n], p.action_ids, n_props=3)
        width = len(p.last_state())
        assert tuple(states[-width:]) == p.last_state()
        assert len(p.action_ids) == depth[p.last_state()]
