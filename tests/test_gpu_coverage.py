"""The coverage pass on the MI355X (`CheckerBuilder.coverage()`, csrc/cover.hpp, csrc/kernels_cover.hpp)
against the host form of the same rule (`_native.coverage_host`, itself checked against the reachable
graph in tests/test_coverage_host.py): every figure, field for field.

Sizes: arenas of 1 state, fewer than 64, 65 and 257 (one more than a wave and than a workgroup), a
LiveGraph of about 16 k states with the grid held at 2 workgroups and 3 strides between flushes (several
strides, several flushes), 256 classes (DGraph) and 72 slots on two mask words (wide ping-pong)."""
import ctypes
import functools
import io

import pytest

sr = pytest.importorskip("stateright_amd")

from stateright_amd import _native as N  # noqa: E402
from stateright_amd import build  # noqa: E402
from stateright_amd.models import Ladder, LiveGraph, Spread  # noqa: E402
from stateright_amd.plugin import Plugin  # noqa: E402
from test_coverage_host import MODELS, STOP_EARLY, UNREACHABLE, dgraph  # noqa: E402

pytestmark = pytest.mark.gpu

FIGURES = ("ran", "states", "terminal", "stutter_ends", "max_out_degree", "out_degree", "n_classes", "nprops", "classes")


@functools.lru_cache(maxsize=None)
def host_of(model_id, params):
    return N.coverage_host(model_id, list(params))


def host(model):
    return host_of(model.MODEL_ID, tuple(model.params()))


def spawn(model, order="auto", on=True, hint=None):
    b = model.checker().coverage(on)
    if hint:
        b = b.capacity_hint(hint)
    if order == "dfs":
        return b.spawn_dfs().join()
    return b.order(order).spawn_bfs().join()


def assert_same(c, model, what=""):
    got, want = c.coverage(), host(model)
    for f in FIGURES:
        assert got[f] == want[f], (what, f)
    assert list(got["properties"].values()) == list(want["properties"].values()), what
    assert [n for n, _ in c.properties()] == list(got["properties"]), what
    assert got["states"] == c.unique_state_count(), what
    return got


def assert_properties_agree(c, cov):
    for name, exp in c.properties():
        holds, found = cov["properties"][name], c.discovery(name) is not None
        if exp == sr.Expectation.Sometimes:
            assert (holds > 0) == found, name
        elif exp == sr.Expectation.Always:
            assert (holds < cov["states"]) == found, name


@pytest.mark.parametrize("key", sorted(MODELS))
def test_matches_the_host_form(key):
    model = MODELS[key][0]
    c = spawn(model)
    if key in STOP_EARLY:  # every property discovered: the search did not explore everything
        assert all(c.discovery(n) is not None for n, _ in c.properties())
        with pytest.raises(sr.CheckerError, match="did not explore everything"):
            c.coverage()
        return
    cov = assert_same(c, model, key)
    assert_properties_agree(c, cov)
    if len(set(N.host_graph(model.MODEL_ID, model.params())[1])) == c._lib.sr_gpu_bfs_init_count(c._h):  # distinct init states
        assert sum(k["taken"] for k in cov["classes"]) == c.stats()["successors"], key


@pytest.mark.parametrize("order", ["fifo", "fast", "dfs"])
def test_every_order_gives_the_same_figures(order):
    for key in ("2pc_3", "increment_lock_3", "paxos_1", "ping_pong_2_lossy", "spread_roots_dup", "live_graph_2_words"):
        assert_same(spawn(MODELS[key][0], order), MODELS[key][0], (key, order))


@pytest.mark.parametrize("model", [
    dgraph(N.SR_ALWAYS, [[1]]),                # 1 state
    Ladder(8, 2),                              # 36 states: less than a wave
    Spread(1, 20, 6, roots=1),                 # 64
    Ladder(12, 2), Ladder(4, 4),               # 52, 80
    Ladder(62, 0),                             # 63 states in a chain, 62 classes
    LiveGraph(6, 2, 1, 3, 0, roots=64, dup=1),  # every v < 64 is a root, and one more: 65 arena entries, 64 states
    Ladder(15, 4),                             # 256
    LiveGraph(8, 2, 1, 3, 0, roots=256, dup=1),  # 257 arena entries: one more than a workgroup
    Spread(1, 20, 8, loops=1, roots=1),        # 256 states, self-loops
], ids=lambda m: f"{type(m).__name__}{tuple(m.params())}")
def test_arena_sizes_around_a_wave_and_a_workgroup(model):
    for order in ("fifo", "fast"):
        assert_same(spawn(model, order), model, order)


LIVE_16K = LiveGraph(14, 3, 7, 1, 11, roots=3, dup=2)  # ("marked" holds everywhere: no terminal state refutes it)


def test_several_strides_and_several_flushes(monkeypatch):
    want = host(LIVE_16K)
    assert want["states"] > 12000
    assert_same(spawn(LIVE_16K), LIVE_16K, "default grid")
    # 2 workgroups over ~16 k states: about 30 strides each, a flush every 3
    monkeypatch.setenv("SR_COVER_GRID", "2")
    monkeypatch.setenv("SR_COVER_CHUNK", "3")
    assert_same(spawn(LIVE_16K), LIVE_16K, "2 workgroups")
    monkeypatch.setenv("SR_COVER_GRID", "3")
    monkeypatch.setenv("SR_COVER_CHUNK", "1")
    assert_same(spawn(LIVE_16K, "fifo"), LIVE_16K, "3 workgroups")
    # the hook's peel loop and two mask words under the same squeeze
    for key in ("paxos_2", "ping_pong_wide_8", "increment_lock_3", "dgraph_cycle"):
        assert_same(spawn(MODELS[key][0]), MODELS[key][0], key)


def test_many_classes_and_many_slots():
    # 256 classes: every node of a ring is a class, each taken once (the flush loop runs past a wave's width)
    ring = dgraph(N.SR_EVENTUALLY, [list(range(256)) + [0]])  # (no terminal state: the search finds nothing)
    cov = assert_same(spawn(ring), ring)
    assert cov["n_classes"] == 256 and all(k["enabled"] == k["taken"] == k["moved"] == 1 for k in cov["classes"])
    wide = MODELS["ping_pong_wide_8"][0]  # 72 slots on two mask words
    cov = assert_same(spawn(wide), wide)
    assert sum(k["taken"] for k in cov["classes"]) > 0


def test_an_arena_grown_in_the_middle_of_the_check(monkeypatch):
    # the visited set grows from a first table of 2^10 slots while the check runs
    monkeypatch.setenv("SR_TABLE_LOG2", "10")
    c = spawn(LIVE_16K)
    assert c.stats()["rehashes"] > 0
    assert_same(c, LIVE_16K)
    big = sr.TwoPhaseSys(6)
    c = spawn(big)
    cov = assert_same(c, big)
    assert sum(k["taken"] for k in cov["classes"]) == c.stats()["successors"]
    monkeypatch.delenv("SR_TABLE_LOG2")
    # the arena itself: a hint of 1000 states sizes it for 2^22 words, 2^20 states of 4 words, and the 2^21
    # subsets of 21 bits outgrow that, so the arena is copied into a larger one in the middle of the check and
    # the pass must read that one. The figures in closed form (no host search of 2 M states): every Set(j) is
    # enabled where bit j is clear and moves, the loop is enabled everywhere and never moves, a state with k
    # clear bits has k + 1 successors, and only the full set can do nothing but loop.
    from math import comb
    f = 21
    c = Spread(4, 100, f, loops=1, mark=12345).checker().coverage().capacity_hint(1000).spawn_bfs().join()
    cov = c.coverage()
    assert cov["states"] == c.unique_state_count() == 2 ** f and cov["n_classes"] == f + 1
    half = {"enabled": 2 ** (f - 1), "taken": 2 ** (f - 1), "moved": 2 ** (f - 1)}
    assert cov["classes"] == [dict(half, name=f"Set({j})") for j in range(f)] + [
        {"name": "Loop(0)", "enabled": 2 ** f, "taken": 2 ** f, "moved": 0}]
    assert (cov["terminal"], cov["stutter_ends"], cov["max_out_degree"]) == (0, 1, f + 1)
    assert cov["out_degree"] == [0] + [comb(f, k) for k in range(f + 1)] + [0] * (64 - f - 2)
    assert cov["properties"] == {"in range": 2 ** f, "marked": 1}
    assert sum(k["taken"] for k in cov["classes"]) == c.stats()["successors"]


def test_with_complete_liveness_too():
    for model, name in ((LiveGraph(12, 2, 3, 2, 0, 1), "marked"), (dgraph(N.SR_EVENTUALLY, [[0, 2, 4, 2], [9, 9]]), "odd")):
        both = model.checker().coverage().complete_liveness().spawn_bfs().join()
        live = model.checker().complete_liveness().spawn_bfs().join()
        cover = model.checker().coverage().spawn_bfs().join()
        assert_same(both, model)
        assert {k: v for k, v in both.coverage().items() if k != "pass_ms"} == {
            k: v for k, v in cover.coverage().items() if k != "pass_ms"}
        a, b = both.liveness(name), live.liveness(name)
        varies = ("pass_ms", "rounds", "examined")  # (implementation details of the trim: never compared)
        assert a["ran"] == 1 and {k: v for k, v in a.items() if k not in varies} == {k: v for k, v in b.items() if k not in varies}
        assert (both.discovery(name) is None) == (live.discovery(name) is None)
        if both.discovery(name) is not None:
            assert both.discovery(name) == live.discovery(name)
        with pytest.raises(sr.CheckerError):
            live.coverage()


def test_sliding_puzzle_plugin():
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    c = puzzle.model(1, 2, 3, 4, 5, 6, 8, 7, 0).checker().coverage().spawn_bfs().join()
    cov = c.coverage()
    assert cov["n_classes"] == 4 and cov["states"] == c.unique_state_count() == 181440
    assert sum(k["taken"] for k in cov["classes"]) == c.state_count() - 1
    assert sorted(k["name"] for k in cov["classes"]) == ["Down", "Left", "Right", "Up"]
    assert cov["properties"] == {"solved": 0} and c.discovery("solved") is None
    assert cov["terminal"] == 0 and cov["out_degree"][2] == 4 * 40320 // 2


def test_option_off_changes_nothing():
    for key in ("2pc_3", "paxos_1", "spread_roots_dup", "dgraph_cycle"):
        model = MODELS[key][0]
        off, on = spawn(model, on=False), spawn(model)
        plain = model.checker().spawn_bfs().join()
        with pytest.raises(sr.CheckerError, match="did not run"):
            off.coverage()
        with pytest.raises(sr.CheckerError, match="did not run"):
            plain.coverage()
        counts = (plain.state_count(), plain.unique_state_count(), plain.max_depth(), sorted(plain.discoveries()))
        assert (off.state_count(), off.unique_state_count(), off.max_depth(), sorted(off.discoveries())) == counts
        assert (on.state_count(), on.unique_state_count(), on.max_depth(), sorted(on.discoveries())) == counts
        assert {n: len(p) for n, p in on.discoveries().items()} == {n: len(p) for n, p in off.discoveries().items()}


def test_a_caller_with_the_old_struct_size_has_the_option_off():
    b = sr.TwoPhaseSys(3).checker().coverage()
    assert b._opts.coverage == 1
    b._opts.struct_size = 56
    c = b.spawn_bfs().join()
    with pytest.raises(sr.CheckerError, match="did not run"):
        c.coverage()
    b._opts.struct_size = ctypes.sizeof(N.sr_opts)
    assert b.spawn_bfs().join().coverage()["states"] == 288


def test_a_search_that_stops_early_has_no_figures():
    # sometimes "odd" is discovered at 1: the search stops with every property discovered
    c = spawn(dgraph(N.SR_SOMETIMES, [[0, 1, 2, 4]]), "fifo")
    assert c.discovery("odd") is not None
    with pytest.raises(sr.CheckerError, match="did not explore everything"):
        c.coverage()
    with pytest.raises(sr.CheckerError):
        c.assert_covered()


def test_the_simulation_checker_ignores_the_option():
    c = sr.TwoPhaseSys(3).checker().coverage().spawn_simulation(seed=1, walks=64, max_depth=16).join()
    with pytest.raises(sr.CheckerError):
        c.coverage()


def test_refusals():
    with pytest.raises(sr.CheckerError, match="coverage with a partitioned search"):
        sr.TwoPhaseSys(3).checker().coverage().partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="coverage with symmetry"):
        sr.TwoPhaseSys(3).checker().coverage().symmetry_canonical().spawn_bfs()
    with pytest.raises(sr.CheckerError, match="coverage with target_state_count"):
        sr.TwoPhaseSys(3).checker().coverage().target_state_count(10).spawn_bfs()


def test_assert_covered_and_the_report():
    c = spawn(sr.TwoPhaseSys(3))
    assert c.assert_covered() is c
    out = io.StringIO()
    c.coverage_report(out)
    text = out.getvalue()
    want = host(sr.TwoPhaseSys(3))
    assert text.startswith(f"Coverage. states=288, terminal=0, stutter_ends={want['stutter_ends']}, "
                           f"max_out_degree={want['max_out_degree']}\n") and "TmCommit" in text
    assert "never taken" not in text and text.count("\n") == 2 + 17 + 3
    rep = io.StringIO()
    c.report(rep)
    assert "Coverage" not in rep.getvalue()  # `report` is the reference's, unchanged
    c = spawn(UNREACHABLE)
    with pytest.raises(AssertionError, match=r"never taken: \[.*'7'.*\]"):
        c.assert_covered()
    never = [k["name"] for k in c.coverage()["classes"] if not k["taken"]]
    assert len(never) == 254 and "7" in never
    with pytest.raises(AssertionError, match="'7'"):
        c.assert_covered(allow=[n for n in never if n != "7"])
    c.assert_covered(allow=never)
    out = io.StringIO()
    c.coverage_report(out)
    assert out.getvalue().count("<- never taken") == 254
