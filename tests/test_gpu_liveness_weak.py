"""Weak fairness of the complete `eventually` check on the GPU (`weak_fairness()`, sr_opts.liveness = 3;
csrc/kernels_live.hpp): for the graphs of tests/test_liveness_weak_host.py the device's result equals the
host form (sr_liveness_host_weak, other algorithms: Tarjan, breadth-first ranks) field by field and the
whole witness action by action (every choice in it is canonical), and the restatement
(tests/live_weak_ref.py) where that is cheap. The search's counts and its other discoveries equal those of
the same check with the option off.

Sizes: the DGraph hand cases, LiveGraph of 8 and 12 bits (one to several workgroups with a tail), 16 bits
(62 k states, with and without a capacity hint, so the table has grown) and 20 bits (836 k states: against
the anchors only), 2- and 4-word states, SpinLock(1..4, 10) (SpinLock(10) "every": 6143 small components,
the repeated colouring) and SpinLock(16) (more states than half the word's key space), 2pc-live (no component
at all), 64 init states, 16 of them once more as duplicates, and a terminal state that the search does not flag.

Compared: sr_live_result without `rounds`, `examined` (the sum of the worklist sizes over those rounds:
both depend on the order in which states leave in place) and `pass_ms`; sr_live_weak without its three
round counters and `pass_ms`."""
import functools

import pytest

import live_fair_ref as LF
import live_weak_ref as LW
import stateright_amd as sr
from stateright_amd import _native as N
from stateright_amd.models import LiveGraph, SpinLockSys, TwoPhaseLiveSys
from test_liveness_weak_host import WEAK_KEYS, assert_weak_matches, model_of, params_of, prop_of, reference

pytestmark = pytest.mark.gpu

FIELDS = ("ran", "init_index", "not_p_states", "surviving", "end_kind", "witness_len", "loop_start")
WEAK_FIELDS = ("ran",) + WEAK_KEYS + ("stem_len", "loop_len")


def spawn(model, on=True, hint=None):
    b = model.checker().weak_fairness(on)
    if hint:
        b = b.capacity_hint(hint)
    return b.spawn_bfs().join()


@functools.lru_cache(maxsize=None)
def host_answer(model_id, params, prop):
    return N.liveness_host_weak(model_id, list(params), prop=prop)


def rejected(c, name, actions):
    try:
        c.assert_discovery(name, actions)
    except AssertionError:
        return True
    return False


def assert_device_is_host(c, model, params, prop, what):
    """c: a joined check under weak fairness. Returns (the device's result in the host form's shape, whether
    the pass made the answer: a terminal counterexample may be the search's own discovery)."""
    name = c.properties()[prop][0]
    r = c.liveness(name)
    found = c.discovery(name)
    host = host_answer(model.MODEL_ID, tuple(params), prop)
    assert c.is_done(), what
    if not r["ran"]:  # (the search found a terminal counterexample itself, and may have stopped there)
        assert found is not None and host["init_index"] >= 0 and "weak" not in r, what
        c.assert_discovery(name, found.action_ids)
        return None, False
    assert c.unique_state_count() == host["unique"], what
    assert {k: r[k] for k in FIELDS} == {k: host[k] for k in FIELDS}, what
    assert {k: r["weak"][k] for k in WEAK_FIELDS} == {k: host["weak"][k] for k in WEAK_FIELDS}, what
    got = dict(r, actions=[] if found is None else found.action_ids)
    assert got["actions"] == host["actions"], what
    if host["init_index"] < 0:
        assert found is None, what
    else:
        assert c.loop_start(name) == (host["loop_start"] if host["loop_start"] >= 0 else None), what
        c.assert_discovery(name, found.action_ids)
    return got, True


def assert_search_unchanged(c, off):
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (off.unique_state_count(), off.state_count(), off.max_depth())
    for name, exp in c.properties():
        if exp != sr.Expectation.Eventually:
            assert c.discovery(name) == off.discovery(name), name
        elif off.discovery(name) is not None:
            assert c.discovery(name) == off.discovery(name) and c.liveness(name)["ran"] == 0, name


# ---- the anchors ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(LW.ANCHORS), ids=[repr(c) for c in LW.ANCHORS])
def test_device_on_the_anchors(case):
    model = model_of(case)
    c = spawn(model)
    assert_search_unchanged(c, spawn(model, on=False))
    got, ran = assert_device_is_host(c, model, params_of(case), prop_of(case), case)
    graph, want = reference(case)
    if ran:
        assert_weak_matches(got, graph, want, case)
    else:
        assert want["init_index"] >= 0  # (the search's own terminal discovery: the property is refuted either way)


def test_what_the_hand_cases_show():
    fair = spawn(model_of(("dgraph", ((0, 2, 4, 2),))))
    assert fair.discovery("odd").into_states() == [(0,), (2,), (4,), (2,)] and fair.loop_start("odd") == 1
    unfair = model_of(("dgraph", ((0, 2, 4, 2), (2, 6), (4, 6), (6, 1))))
    held = spawn(unfair)
    assert held.discovery("odd") is None and held.liveness("odd")["weak"]["components"] == 1
    progress = unfair.checker().complete_liveness(fairness="progress").spawn_bfs().join()
    assert progress.discovery("odd").action_ids == [2, 4, 2]  # the lasso the progress mode reports
    progress.assert_discovery("odd", [2, 4, 2])
    # under weak fairness the same lasso is no counterexample: slot 6 is moving-enabled at 2 and at 4, never taken
    other = spawn(model_of(("dgraph", ((0, 2, 4, 2), (2, 6, 8, 6), (4, 6)))))
    assert other.discovery("odd") is not None
    assert rejected(other, "odd", [2, 4, 2])
    other.assert_discovery("odd", other.discovery("odd").action_ids)
    assert other._lib.sr_gpu_bfs_loop_fair(other._h, 0, (N.ctypes.c_int64 * 3)(2, 4, 2), 3, 1) == 0
    assert other._lib.sr_gpu_bfs_loop_fair(other._h, 0, (N.ctypes.c_int64 * 3)(2, 4, 3), 3, 1) == -1
    assert fair._lib.sr_gpu_bfs_loop_fair(fair._h, 0, (N.ctypes.c_int64 * 3)(2, 4, 2), 3, 1) == 1


def test_device_ends_at_a_terminal_state_the_search_does_not_flag():
    """The pass' TERMINAL ending (end_kind 1) on the device: the anchors' terminal counterexamples are the
    search's own discoveries, for which the pass does not run."""
    case = LW.LATE_TERMINAL
    model = model_of(case)
    c = spawn(model)
    off = spawn(model, on=False)
    assert off.discovery("odd") is None  # the search's rule misses it
    got, ran = assert_device_is_host(c, model, params_of(case), 0, case)
    assert ran and (got["end_kind"], got["loop_start"], got["weak"]["loop_len"]) == (1, -1, 0)
    assert c.discovery("odd").into_states() == [(0,), (2,), (4,), (8,), (6,)]
    assert_weak_matches(got, *reference(case), case)


def test_device_with_duplicate_roots():
    """64 roots and the first 16 once more: the arena holds those states twice, live_mark lists one copy of
    each, and the first init state in FairF (root 10) is among them."""
    params, dup = LW.DUP_ROOTS
    model = LiveGraph(*params, dup=dup)
    c = spawn(model)
    once = spawn(LiveGraph(*params))
    assert c.unique_state_count() == once.unique_state_count() and c.state_count() > once.state_count()
    got, ran = assert_device_is_host(c, model, model.params(), 0, LW.DUP_ROOTS)
    assert ran and got["init_index"] == 10
    graph = LW.dup_roots_graph()
    assert_weak_matches(got, graph, LW.check(*graph), LW.DUP_ROOTS)
    assert got["actions"] == once.discovery("marked").action_ids


def test_device_on_spin_lock_16():
    """More states than half of the word's key space has values (17 * 2^17 > 2^21): the declared key must be
    wider than the word, or the visited set's homes run out. Against figures that follow from the model: the
    states where nobody is served are (holder, tick), 2 (n + 1) of them, in n + 1 Tick pairs, none of them
    fair (Acquire or Release stays moving-enabled and is never taken)."""
    n = 16
    c = spawn(SpinLockSys(n), hint=(n + 1) << (n + 1))
    assert c.unique_state_count() == (n + 1) << (n + 1) and c.is_done()
    some, every = c.liveness("some thread served"), c.liveness("every thread served")
    assert (some["not_p_states"], some["surviving"], some["init_index"]) == (2 * (n + 1), 2 * (n + 1), -1)
    assert (some["weak"]["components"], some["weak"]["fair_components"], some["weak"]["fair_states"]) == (n + 1, 0, 0)
    assert c.discovery("some thread served") is None
    total = (n + 1) << (n + 1)
    assert (every["not_p_states"], every["surviving"], every["weak"]["cyclic_states"]) == (total - 2 * (n + 1),) * 3
    assert (every["init_index"], every["end_kind"], every["weak"]["stem_len"]) == (0, 2, 2)
    found = c.discovery("every thread served")
    assert len(found.action_ids) == every["witness_len"] == 2 + every["weak"]["loop_len"]
    c.assert_discovery("every thread served", found.action_ids)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_device_on_spin_lock(n):
    model = SpinLockSys(n)
    c = spawn(model)
    assert_search_unchanged(c, spawn(model, on=False))
    assert c.unique_state_count() == (n + 1) * 2 ** n * 2
    for prop in (0, 1):
        case = ("spin", n, prop)
        got, ran = assert_device_is_host(c, model, [n], prop, case)
        assert ran
        assert_weak_matches(got, *reference(case), case)
    assert c.discovery("some thread served") is None
    for fairness in (None, "progress"):  # the Tick cycle refutes it in the other modes
        other = model.checker().complete_liveness(fairness=fairness).spawn_bfs().join()
        assert other.liveness("some thread served")["end_kind"] == 2


def test_device_on_spin_lock_10():
    model = SpinLockSys(10)
    c = spawn(model)
    for prop in (0, 1):
        case = ("spin", 10, prop)
        got, ran = assert_device_is_host(c, model, [10], prop, case)
        assert ran
        assert_weak_matches(got, *reference(case), case)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_device_on_two_phase_live(n):
    model = TwoPhaseLiveSys(n)
    c = spawn(model)
    assert_search_unchanged(c, spawn(model, on=False))
    for prop in (3, 4):
        case = ("2pc", n, prop)
        got, ran = assert_device_is_host(c, model, [n], prop, case)
        assert ran
        assert_weak_matches(got, *reference(case), case)
    assert c.liveness("every RM commits")["end_kind"] == 3


# ---- shapes: wide states, several launches, a table that has grown -------------------------------------------

@pytest.mark.parametrize("words", [2, 4])
@pytest.mark.parametrize("params", [(12, 2, 26, 2, 0, 1), (12, 2, 1, 2, 0, 64)])
def test_device_on_wide_states(params, words):
    case = ("live", params)
    model = LiveGraph(*params, words=words)
    got, ran = assert_device_is_host(spawn(model), model, model.params(), 0, (case, words))
    assert ran
    assert_weak_matches(got, *reference(case), (case, words))


def test_the_witness_in_several_launches(monkeypatch):
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "3")  # the 9-step stem and the loop's segments take several launches
    case = ("live", (12, 2, 26, 2, 0, 1))
    model = model_of(case)
    got, ran = assert_device_is_host(spawn(model), model, params_of(case), 0, case)
    assert ran and got["weak"]["stem_len"] == 9
    assert_weak_matches(got, *reference(case), case)


@pytest.mark.parametrize("hint", [None, 1 << 17])
def test_device_on_sixteen_bits(hint):
    case = ("live", (16, 3, 26, 2, 0, 1))
    model = model_of(case)
    c = spawn(model, hint=hint)
    got, ran = assert_device_is_host(c, model, params_of(case), 0, (case, hint))
    assert ran
    anchor = LW.GPU_ANCHORS[case]
    flat = dict(got["weak"], unique=c.unique_state_count(), **{k: got[k] for k in ("not_p_states", "surviving", "init_index")})
    assert tuple(flat[k] for k in LW.ANCHOR_KEYS) == anchor[:8] and got["weak"]["stem_len"] == anchor[8]


def test_device_on_twenty_bits():
    case = ("live", (20, 2, 1, 3, 0, 1))
    c = spawn(model_of(case), hint=1 << 20)
    r = c.liveness("marked")
    flat = dict(r["weak"], unique=c.unique_state_count(), **{k: r[k] for k in ("not_p_states", "surviving", "init_index")})
    assert tuple(flat[k] for k in LW.ANCHOR_KEYS) == LW.GPU_ANCHORS[case][:8]
    found = c.discovery("marked")  # (the engine replayed it on the host model and found its loop weakly fair)
    assert r["end_kind"] == 2 and r["loop_start"] == r["weak"]["stem_len"] and len(found.action_ids) == r["witness_len"]
    c.assert_discovery("marked", found.action_ids)


# ---- the option ------------------------------------------------------------------------------------------------

def test_weak_fairness_meets_the_refusals():
    from stateright_amd import build
    from stateright_amd.plugin import Plugin
    with pytest.raises(sr.CheckerError, match="liveness with a partitioned search"):
        TwoPhaseLiveSys(3).checker().weak_fairness().partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        TwoPhaseLiveSys(3).checker().weak_fairness().target_state_count(10).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with symmetry"):
        sr.TwoPhaseSys(3).checker().weak_fairness().symmetry_canonical().spawn_bfs()
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    with pytest.raises(sr.CheckerError, match="liveness with a plugin model"):
        puzzle.model(1, 4, 2, 3, 5, 8, 6, 7, 0).checker().weak_fairness().spawn_bfs()
    with pytest.raises(sr.CheckerError, match=r"more than 2\^32 - 1 unique states"):
        TwoPhaseLiveSys(3).checker().weak_fairness().capacity_hint(2 ** 32).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="slots are not fairness classes"):
        sr.PingPong(2).checker().weak_fairness().spawn_bfs()
    with pytest.raises(sr.CheckerError, match="slots are not fairness classes"):
        sr.Increment(2).checker().weak_fairness().spawn_bfs()


def test_seven_is_still_the_plain_mode():
    b = model_of(("dgraph", ((0, 2, 4, 2), (2, 6), (4, 6), (6, 1)))).checker().complete_liveness()
    b._opts.liveness = 7
    c = b.spawn_bfs().join()
    r = c.liveness("odd")
    assert c.discovery("odd").action_ids == [2, 4, 2] and r["end_kind"] == 2 and "weak" not in r
    w = N.sr_live_weak()
    assert c._lib.sr_gpu_bfs_liveness_weak(c._h, 0, N.ctypes.byref(w)) == 0 and w.ran == 0
