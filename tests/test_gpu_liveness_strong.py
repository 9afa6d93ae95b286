"""Strong fairness of the complete `eventually` check on the GPU (`strong_fairness()`, sr_opts.liveness = 4;
csrc/kernels_live.hpp, Engine::live_strong_pass): the device's level-synchronous decomposition equals the host
form (sr_liveness_host_strong, another algorithm: the tree by recursion, Tarjan, breadth-first ranks) field
by field and the whole witness action by action (every choice in it is canonical), and the restatement
(tests/live_strong_ref.py) where that is cheap. The search's counts and its other discoveries equal those of
the same check with the option off, and `weak_fairness()` still answers as it did.

Sizes: the DGraph hand cases and LiveGraph of 8, 12 and 16 bits (none nests: one level), SpinLock(3), (10)
(two levels, 11253 components, no fair node) and (16) (2.2 M states), FairRings from one lane of two rings to 64
lanes of mixed depths and 13 levels (lanes finish at different levels in the same launches; an arena index is
a component's root at several levels), and 2pc-live (no component at all).

Compared: sr_live_result without `rounds`, `examined` and `pass_ms`; sr_live_strong without its three round
counters and `pass_ms`."""
import functools

import pytest

import live_strong_ref as LS
import live_weak_ref as LW
import stateright_amd as sr
from stateright_amd import _native as N
from stateright_amd.models import FairRings, SpinLockSys, TwoPhaseLiveSys
from test_liveness_strong_host import STRONG_KEYS, assert_strong_matches, model_of, params_of, prop_of, reference

pytestmark = pytest.mark.gpu

FIELDS = ("ran", "init_index", "not_p_states", "surviving", "end_kind", "witness_len", "loop_start")
STRONG_FIELDS = ("ran",) + STRONG_KEYS + ("stem_len", "loop_len")


def spawn(model, on=True, hint=None, mode="strong"):
    b = model.checker()
    b = b.strong_fairness(on) if mode == "strong" else b.weak_fairness(on)
    if hint:
        b = b.capacity_hint(hint)
    return b.spawn_bfs().join()


@functools.lru_cache(maxsize=None)
def host_answer(model_id, params, prop):
    return N.liveness_host_strong(model_id, list(params), prop=prop)


def rejected(c, name, actions):
    try:
        c.assert_discovery(name, actions)
    except AssertionError as e:
        return str(e)
    return None


def assert_device_is_host(c, model, params, prop, what):
    """c: a joined check under strong fairness. Returns (the device's result in the host form's shape, whether
    the pass made the answer: a terminal counterexample may be the search's own discovery)."""
    name = c.properties()[prop][0]
    r = c.liveness(name)
    found = c.discovery(name)
    host = host_answer(model.MODEL_ID, tuple(params), prop)
    assert c.is_done(), what
    if not r["ran"]:  # (the search found a terminal counterexample itself, and may have stopped there)
        assert found is not None and host["init_index"] >= 0 and "strong" not in r, what
        c.assert_discovery(name, found.action_ids)
        return None, False
    assert "weak" not in r, what
    assert c.unique_state_count() == host["unique"], what
    assert {k: r[k] for k in FIELDS} == {k: host[k] for k in FIELDS}, what
    assert {k: r["strong"][k] for k in STRONG_FIELDS} == {k: host["strong"][k] for k in STRONG_FIELDS}, what
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


def check_case(case, hint=None, restated=True):
    model = model_of(case)
    c = spawn(model, hint=hint)
    got, ran = assert_device_is_host(c, model, params_of(case), prop_of(case), (case, hint))
    if restated:
        graph, want = reference(case)
        if ran:
            assert_strong_matches(got, graph, want, case)
        else:
            assert want["init_index"] >= 0  # (the search's own terminal discovery: refuted either way)
    return c, got, ran


# ---- the graphs that do not nest: DGraph, LiveGraph, 2pc-live -------------------------------------------------

DGRAPHS = [c for c in LW.ANCHORS if c[0] == "dgraph"] + [LW.LATE_TERMINAL]


@pytest.mark.parametrize("case", DGRAPHS, ids=[repr(c) for c in DGRAPHS])
def test_device_on_the_dgraph_hand_cases(case):
    c, got, ran = check_case(case)
    assert_search_unchanged(c, spawn(model_of(case), on=False))
    if ran:
        assert got["strong"]["levels"] <= 1


@pytest.mark.parametrize("case", [c for c in LW.ANCHORS if c[0] == "live"], ids=repr)
def test_device_on_live_graphs(case):
    c, got, ran = check_case(case)
    if not ran:  # (a terminal counterexample that the search flags itself: the pass does not run)
        assert case == ("live", (12, 2, 1, 3, 16, 1))
        return
    assert got["strong"]["levels"] <= 1
    weak = spawn(model_of(case), mode="weak").liveness("marked")  # none of these nests: the weak mode's figures
    for key in ("cyclic_states", "components", "fair_components", "goal_states", "fair_states", "stem_len"):
        assert got["strong"][key] == weak["weak"][key], (case, key)
    assert got["init_index"] == weak["init_index"]


@pytest.mark.parametrize("hint", [None, 1 << 17])
def test_device_on_sixteen_bits(hint):
    case = ("live", (16, 3, 26, 2, 0, 1))
    c, got, ran = check_case(case, hint=hint, restated=False)
    assert ran
    anchor = LW.GPU_ANCHORS[case]  # (one level: the weak mode's figures)
    flat = dict(got["strong"], unique=c.unique_state_count(), **{k: got[k] for k in ("not_p_states", "surviving", "init_index")})
    assert tuple(flat[k] for k in LW.ANCHOR_KEYS) == anchor[:8] and got["strong"]["stem_len"] == anchor[8]
    assert got["strong"]["levels"] == 1


def test_device_on_two_phase_live():
    model = TwoPhaseLiveSys(3)
    c = spawn(model)
    assert_search_unchanged(c, spawn(model, on=False))
    for prop in (3, 4):
        case = ("2pc", 3, prop)
        got, ran = assert_device_is_host(c, model, [3], prop, case)
        assert ran and (got["strong"]["components"], got["strong"]["levels"]) == (0, 0)
        assert_strong_matches(got, *reference(case), case)
    assert c.liveness("every RM commits")["end_kind"] == 3


# ---- SpinLock: two levels, no fair node ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 10])
def test_device_on_spin_lock(n):
    model = SpinLockSys(n)
    c = spawn(model)
    assert_search_unchanged(c, spawn(model, on=False))
    for prop in (0, 1):
        case = ("spin", n, prop)
        got, ran = assert_device_is_host(c, model, [n], prop, case)
        assert ran
        assert_strong_matches(got, *reference(case), case)
        if case in LS.ANCHORS:
            flat = dict(got["strong"], unique=c.unique_state_count(), surviving=got["surviving"], init_index=got["init_index"])
            assert tuple(flat[k] for k in LS.ANCHOR_KEYS) == LS.ANCHORS[case][:8]
    assert c.discovery("some thread served") is None and c.discovery("every thread served") is None
    weak = spawn(model, mode="weak")  # the contrast: weak fairness refutes "every thread served" from init 0
    assert weak.liveness("every thread served")["init_index"] == 0


def test_assert_discovery_rejects_a_loop_that_is_only_weakly_fair():
    """The weak mode's own witness of SpinLock(3) "every thread served": its loop starves a thread whose Acquire
    is enabled again and again, so a check under strong fairness does not take it for a counterexample."""
    name = "every thread served"
    weak = spawn(SpinLockSys(3), mode="weak")
    lasso = weak.discovery(name).action_ids
    weak.assert_discovery(name, lasso)
    # a check under strong fairness that has a discovery of its own to compare with: FairRings has none for this
    # model, so ask the loop predicate, and assert_discovery on a model with a discovery below
    strong = spawn(SpinLockSys(3))
    arr = (N.ctypes.c_int64 * len(lasso))(*lasso)
    start = weak.loop_start(name)
    assert weak._lib.sr_gpu_bfs_loop_fair(weak._h, 0, arr, len(lasso), start) == 1
    assert strong._lib.sr_gpu_bfs_loop_strongly_fair(strong._h, 0, arr, len(lasso), start) == 0
    assert strong.discovery(name) is None
    with pytest.raises(AssertionError, match="not found"):
        strong.assert_discovery(name, lasso)
    # FairRings(1, 4, 1, 1): Step round ring 0 is weakly fair to nothing it must take but is a closed loop in
    # N_p; Out(0) is moving-enabled on it and never taken, so it is not strongly fair
    rings = spawn(FairRings(1, 4, 1, 1))
    why = rejected(rings, "done", [0, 0, 0, 0])
    assert why is not None and "closes a loop that is not strongly fair" in why
    rings.assert_discovery("done", rings.discovery("done").action_ids)


def test_device_on_spin_lock_16():
    """A decomposition over 2.2 M states in two levels; its figures come from the host form."""
    n = 16
    model = SpinLockSys(n)
    c = spawn(model, hint=(n + 1) << (n + 1))
    assert c.unique_state_count() == (n + 1) << (n + 1) and c.is_done()
    host = host_answer(model.MODEL_ID, (n,), 1)
    every = c.liveness("every thread served")
    assert {k: every[k] for k in FIELDS} == {k: host[k] for k in FIELDS}
    assert {k: every["strong"][k] for k in STRONG_FIELDS} == {k: host["strong"][k] for k in STRONG_FIELDS}
    assert (every["strong"]["levels"], every["strong"]["fair_components"], every["init_index"]) == (2, 0, -1)
    assert c.discovery("every thread served") is None


# ---- FairRings: nesting by construction ---------------------------------------------------------------------

RINGS = [(1, 4, 0, 1), (1, 4, 1, 1), (1, 4, 2, 1), (2, 4, 2, 2), (4, 6, 2, 8), (12, 16, 2, 64), (12, 16, 0, 64)]


@pytest.mark.parametrize("params", RINGS, ids=repr)
def test_device_on_fair_rings(params):
    case = ("rings", params)
    c, got, ran = check_case(case)
    assert ran
    assert_search_unchanged(c, spawn(model_of(case), on=False))
    forms = LS.fair_rings_closed_forms(*params)
    flat = dict(got["strong"], unique=c.unique_state_count(), **{k: got[k] for k in ("not_p_states", "surviving", "init_index")})
    assert {k: flat[k] for k in forms} == forms
    if case in LS.ANCHORS:
        assert tuple(flat[k] for k in LS.ANCHOR_KEYS) == LS.ANCHORS[case][:8]
    if case in LS.WITNESSES:
        stem, loop = LS.WITNESSES[case]
        assert got["actions"] == stem + loop and c.loop_start("done") == len(stem)
    # under weak fairness the same model is refuted from init 0: every lane is one weakly fair component
    weak = spawn(model_of(case), mode="weak")
    r = weak.liveness("done")
    assert (r["init_index"], r["end_kind"]) == (0, 2)
    assert (r["weak"]["components"], r["weak"]["fair_components"]) == (params[3], params[3])
    weak.assert_discovery("done", weak.discovery("done").action_ids)


def test_the_witness_in_several_launches(monkeypatch):
    monkeypatch.setenv("SR_LIVE_WALK_STEPS", "2")  # the 3-step stem and the loop's segments take several launches
    check_case(("rings", (4, 6, 2, 8)))


# ---- the option ------------------------------------------------------------------------------------------------

def test_strong_fairness_false_is_off():
    model = FairRings(2, 4, 2, 2)
    c = spawn(model, on=False)
    r = c.liveness("done")
    assert r["ran"] == 0 and "strong" not in r and c.discovery("done") is None
    g = N.sr_live_strong()
    assert c._lib.sr_gpu_bfs_liveness_strong(c._h, 0, N.ctypes.byref(g)) == 0 and g.ran == 0


def test_strong_fairness_meets_the_refusals():
    with pytest.raises(sr.CheckerError, match="liveness with a partitioned search"):
        TwoPhaseLiveSys(3).checker().strong_fairness().partitions(2).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with target_state_count"):
        TwoPhaseLiveSys(3).checker().strong_fairness().target_state_count(10).spawn_bfs()
    with pytest.raises(sr.CheckerError, match="liveness with symmetry"):
        sr.TwoPhaseSys(3).checker().strong_fairness().symmetry_canonical().spawn_bfs()
    with pytest.raises(sr.CheckerError, match="slots are not fairness classes"):
        sr.PingPong(2).checker().strong_fairness().spawn_bfs()
    with pytest.raises(sr.CheckerError, match="slots are not fairness classes"):
        sr.Paxos(1).checker().strong_fairness().spawn_bfs()


def test_seven_is_still_the_plain_mode():
    b = model_of(("dgraph", ((0, 2, 4, 2), (2, 6), (4, 6), (6, 1)))).checker().complete_liveness()
    b._opts.liveness = 7
    c = b.spawn_bfs().join()
    r = c.liveness("odd")
    assert c.discovery("odd").action_ids == [2, 4, 2] and r["end_kind"] == 2 and "weak" not in r and "strong" not in r
    g = N.sr_live_strong()
    assert c._lib.sr_gpu_bfs_liveness_strong(c._h, 0, N.ctypes.byref(g)) == 0 and g.ran == 0
