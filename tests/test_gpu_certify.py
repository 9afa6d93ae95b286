"""The production forms of the search under the certificate pass (csrc/certify.hpp; tests/certify_lib.py).

The table audit of a counting run never sees the kernels a plain check launches (`counters()` selects the
counting instantiations and switches forms off), and counts cannot see a wrong parent, a state listed a level
late or a wrong FIFO order. Here no test uses `counters()`: every check runs what a user's check runs, with
`certify()` on, and asserts a clean certificate (assert_certified: every error counter 0, the count identities
exact, every discovery at the first discovering level, in FIFO order at the first discovering state) beside the
oracle's or the closed-form counts. The certificate's kernels are themselves compared with a plain host
evaluation in test_gpu_certify_selftest.py; for the small models here its figures are also compared with a
Python search over the host graph (certify_lib.reference).

Sizes are the smallest that reach a form; a check takes a fraction of a second up to a few seconds."""
import functools
import json
import math
import os

import pytest

from certify_lib import assert_certified, assert_matches_reference, reference
from oracle_lib import INCREMENT, INCREMENT_LOCK, PAXOS, TWO_PHASE, OracleRun

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")
from stateright_amd import build  # noqa: E402
from stateright_amd.models import Ladder, LiveGraph, Spread  # noqa: E402
from stateright_amd.plugin import Plugin  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = ["fifo", "fast"]


def counts(c):
    return c.unique_state_count(), c.state_count(), c.max_depth()


def two_phase_counts(n):
    return 6 ** n + 4 ** n + 2 ** n, (4 * n * 6 ** n + 3 * (n + 1) * 4 ** n + 3 * n * 2 ** n + 6) // 3, 3 * n + 1


def increment_lock_counts(n):
    u = 1 + 4 * sum(math.factorial(n) // math.factorial(n - k) for k in range(1, n + 1))
    return u, u, 4 * n


def paxos_counts(clients):
    with open(os.path.join(HERE, "golden", "paxos_counts.json")) as f:
        r = next(r for r in json.load(f)["cases"] if r["client_count"] == clients)
    return r["unique_state_count"], r["state_count"], r["max_depth"]


@functools.lru_cache(maxsize=None)
def oracle_counts(model, *params):
    o = OracleRun(model, list(params))
    return o.unique_state_count, o.state_count, o.max_depth


def certified(model, order, hint=0):
    b = model.checker().order(order).certify()
    if hint:
        b = b.capacity_hint(hint)
    return b.spawn_bfs().join()


_refs = {}


def check_against_reference(c, key, model):
    """The certificate's figures against the Python search over the host graph, computed once per model."""
    if key not in _refs:
        _refs[key] = reference(model, c.properties())
    ref = _refs[key]
    assert counts(c) == (ref["unique"], ref["state_count"], ref["max_depth"])
    assert_matches_reference(c.certificate(), ref)


# ---- families, default forms ----------------------------------------------------------------------------------

@pytest.mark.parametrize("order", BOTH)
def test_two_phase_7(order):
    c = certified(sr.TwoPhaseSys(7), order)
    assert counts(c) == two_phase_counts(7) == oracle_counts(TWO_PHASE, 7)
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_two_phase_5_against_the_reference(order):
    c = certified(sr.TwoPhaseSys(5), order)
    assert counts(c) == two_phase_counts(5)
    assert_certified(c)
    check_against_reference(c, "2pc5", sr.TwoPhaseSys(5))


def test_two_phase_9_compiled_in():
    # the compiled-in TwoPhaseT<9>: 10 M states, the bench's own form
    n = 9
    c = certified(sr.TwoPhaseSys(n), "fast", hint=two_phase_counts(n)[0])
    assert counts(c) == two_phase_counts(n)
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_increment_10_two_words(order):
    # Its one property ("fin") is violated at depth 4, so the check ends inside level 4 as the reference's does: an
    # early exit, certified as one. In FAST order the counts of an early exit depend on the visit order by design
    # (test_counts_match_oracle), so only FIFO order is compared with the oracle's.
    c = certified(sr.Increment(10), order)
    assert sorted(c.discoveries()) == ["fin"] and len(c.discovery("fin")) == 4
    if order == "fifo":
        assert counts(c) == oracle_counts(INCREMENT, 10)
    else:
        assert c.unique_state_count() <= c.state_count()
    cert = assert_certified(c, complete=False)
    assert cert["explored_all"] == 0 and cert["levels"] == 5 and cert["first_level"] == [4]


@pytest.mark.parametrize("order", BOTH)
@pytest.mark.parametrize("n", [8, 9])
def test_increment_lock(n, order):
    # N=8: one word; N=9: a two-word quotient key, no duplicate filter
    c = certified(sr.IncrementLock(n), order, hint=increment_lock_counts(n)[0])
    assert counts(c) == increment_lock_counts(n) == oracle_counts(INCREMENT_LOCK, n)
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_paxos_2(order):
    c = certified(sr.Paxos(2, 3), order)
    assert counts(c) == paxos_counts(2) == oracle_counts(PAXOS, 2)
    assert_certified(c)
    check_against_reference(c, "paxos2", sr.Paxos(2, 3))


@pytest.mark.parametrize("clients", [3, 5])
def test_paxos_fast(clients):
    # C=3 runs the compiled-in PaxosT<11, 3>; C=5 has 12-word states
    c = certified(sr.Paxos(clients, 3), "fast")
    assert counts(c) == paxos_counts(clients)
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_ping_pong_17_words(order):
    model = sr.PingPong(8, lossy=True)
    c = certified(model, order)
    assert_certified(c)
    check_against_reference(c, "pingpong8", model)


@pytest.mark.parametrize("order", BOTH)
@pytest.mark.parametrize("clients,servers", [(2, 2), (3, 2)])
def test_abd(clients, servers, order):
    c = certified(sr.AbdRegister(clients, servers), order)
    assert_certified(c)
    check_against_reference(c, f"abd{clients}{servers}", sr.AbdRegister(clients, servers))


@pytest.mark.parametrize("order", BOTH)
def test_single_copy_3_1(order):
    c = certified(sr.SingleCopyRegister(3, 1), order)
    assert_certified(c)
    check_against_reference(c, "single31", sr.SingleCopyRegister(3, 1))


@pytest.mark.parametrize("order", BOTH)
def test_linear_equation_510_tiny_levels(order):
    # 510 levels of at most 256 states: chained launches
    c = certified(sr.LinearEquation(2, 4, 7), order)
    assert counts(c) == (65536, 131073, 510)
    assert c.discoveries() == {}
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
@pytest.mark.parametrize("rungs,free_bits", [(58, 8), (2, 19)])
def test_ladder_with_64_parents_per_wave(rungs, free_bits, order, monkeypatch):
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    c = certified(Ladder(rungs, free_bits), order)
    assert counts(c)[0] == (rungs + 1) * 2 ** free_bits and c.max_depth() == rungs + free_bits
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_spread_one_bit_remainder(order):
    # a 13-bit key in the default 2^22 slots: the table is larger than the key space
    f = 12
    c = certified(Spread(1, 13, f, 1, 0b010110011011), order)
    assert counts(c) == (2 ** f, 1 + f * 2 ** (f - 1) + 2 ** f, f)
    assert c.stats()["table_encoding"] & 0xff == 1
    assert_certified(c)
    check_against_reference(c, "spread13", Spread(1, 13, f, 1, 0b010110011011))


@pytest.mark.parametrize("order", BOTH)
def test_live_graph_four_words(order):
    # "marked" holds everywhere (p_mod = 1), so the `eventually` property is never discovered and the search explores
    # everything; it is not of the certified kinds
    c = certified(LiveGraph(12, 3, 7, 1, 9, 3, words=4), order)
    assert c.discoveries() == {}
    cert = assert_certified(c)
    assert cert["pmask"] == 0 and cert["fifo"] == (order == "fifo")


@pytest.mark.parametrize("order", BOTH)
def test_repeated_init_states(order):
    # roots 0 .. 39 and 0 .. 8 again: the repeats are popped and expanded a second time, and counted apart
    f, roots, dup = 12, 40, 9
    model = Spread(2, 50, f, 1, 0b010110011011, roots, dup)
    c = certified(model, order)
    cert = assert_certified(c)
    assert (cert["inits"], cert["repeated_inits"], cert["states"]) == (roots + dup, dup, 2 ** f + dup)
    assert cert["repeated_edges"] == sum(f - bin(i).count("1") + 1 for i in range(dup))
    check_against_reference(c, "spread-dup", model)


@pytest.mark.parametrize("order", BOTH)
def test_symmetry_canonical(order):
    c = sr.TwoPhaseSys(6).checker().order(order).symmetry_canonical().certify().spawn_bfs().join()
    plain = sr.TwoPhaseSys(6).checker().order(order).symmetry_canonical().spawn_bfs().join()
    assert counts(c) == counts(plain) and c.unique_state_count() < two_phase_counts(6)[0]
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_sliding_puzzle_plugin(order):
    puzzle = Plugin(build.plugin_path("sliding_puzzle"), "sliding_puzzle")
    c = puzzle.model(1, 2, 3, 4, 5, 6, 8, 7, 0).checker().order(order).certify().spawn_bfs().join()
    assert c.unique_state_count() == 181440 and c.discoveries() == {}
    assert_certified(c)


def test_a_partitioned_spawn_leaves_the_certificate_empty():
    c = sr.TwoPhaseSys(5).checker().partitions(2).certify().spawn_bfs().join()
    assert counts(c) == two_phase_counts(5)
    assert c.certificate()["ran"] == 0


def test_a_check_without_the_option_has_no_certificate():
    assert sr.TwoPhaseSys(4).checker().spawn_bfs().join().certificate()["ran"] == 0


# ---- forms forced by knobs, FAST order ------------------------------------------------------------------------

KNOBS = [
    {"SR_PROBE_BATCH": "-4"}, {"SR_ACTION_TABLE": "0"}, {"SR_PIPELINE": "0"}, {"SR_PIPELINE": "1"},
    {"SR_GRID_MAX": "1"}, {"SR_GRID_MAX": "2"}, {"SR_BALANCE": "0", "SR_BALANCE_MIN": "0"}, {"SR_BALANCE": "1", "SR_BALANCE_MIN": "0"},
    {"SR_CHAIN_MAX": "0"}, {"SR_CHAIN_MAX": "100000000"}, {"SR_FILTER_LOG2": "0"}, {"SR_FILTER_COMPACT": "0"},
    {"SR_PPW_LOG2": "0"}, {"SR_PPW_LOG2": "6"},
]
PAXOS_KNOBS = KNOBS + [{"SR_WIDE_NOPF": "0"}, {"SR_WIDE_NOPF": "1"}]


def knob_id(k):
    return ",".join(f"{a[3:].lower()}={b}" for a, b in k.items())


@pytest.mark.parametrize("knobs", KNOBS, ids=knob_id)
def test_two_phase_forms(knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    n = 8 if "SR_GRID_MAX" not in knobs else 7  # (one workgroup strides over N=7's levels in a fraction of N=8's time)
    c = certified(sr.TwoPhaseSys(n), "fast")
    assert counts(c) == two_phase_counts(n)
    assert_certified(c)


@pytest.mark.parametrize("knobs", PAXOS_KNOBS, ids=knob_id)
def test_paxos_forms(knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    c = certified(sr.Paxos(2, 3), "fast")
    assert counts(c) == paxos_counts(2)
    assert_certified(c)


# ---- growth, without counters() -------------------------------------------------------------------------------

@pytest.mark.parametrize("order", BOTH)
def test_growth_from_a_tiny_table_by_doubling(order, monkeypatch):
    monkeypatch.setenv("SR_TABLE_LOG2", "10")
    monkeypatch.setenv("SR_GROW_STEP", "2")
    c = certified(sr.TwoPhaseSys(7), order)
    assert counts(c) == two_phase_counts(7)
    # (2^10 slots cannot hold 296 448 states: at least one growth; FAST order's enqueued early growth sizes the
    # table for three projected levels at once, so it may need no second one)
    assert c.stats()["rehashes"] >= 1, c.stats()
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
@pytest.mark.parametrize("ranges", ["0", "1"])
def test_rehash_by_cas_and_by_ranges(ranges, order, monkeypatch):
    monkeypatch.setenv("SR_TABLE_LOG2", "12")
    monkeypatch.setenv("SR_REHASH_RANGES", ranges)
    c = certified(sr.TwoPhaseSys(7), order)
    assert counts(c) == two_phase_counts(7)
    assert c.stats()["rehashes"] >= 1, c.stats()
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
@pytest.mark.parametrize("model", ["2pc7", "inclock9"])
def test_mid_level_doubling_and_repair(model, order, monkeypatch):
    # the probe limit lowered as in test_probe_limit_overflow_doubles_the_table: a level overflows it, the table
    # doubles in the middle of the level and the repair pass finishes the level on the new table
    monkeypatch.setenv("SR_DISP_LIMIT", "3" if model == "2pc7" else "6")
    if model == "2pc7":
        c = certified(sr.TwoPhaseSys(7), order)
        assert counts(c) == two_phase_counts(7)
    else:
        c = certified(sr.IncrementLock(9), order)
        assert counts(c) == increment_lock_counts(9)
    assert c.stats()["table_doublings"] > 0 and c.stats()["restarts"] == 0, c.stats()
    assert_certified(c)


@pytest.mark.parametrize("order", BOTH)
def test_arena_growth(order, monkeypatch):
    monkeypatch.setenv("SR_ARENA_STEP", "2")
    c = certified(sr.TwoPhaseSys(8), order)
    assert counts(c) == two_phase_counts(8)
    assert_certified(c)


def test_increment_lock_9_unhinted_defers_a_speculative_level():
    c = certified(sr.IncrementLock(9), "fast")
    assert counts(c) == increment_lock_counts(9)
    assert c.stats()["rehashes"] > 0, c.stats()
    assert_certified(c)


# ---- stops ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", [1500, 5000])
def test_target_state_count_stop(target):
    o = OracleRun(TWO_PHASE, [4], target=target)
    c = sr.TwoPhaseSys(4).checker().target_state_count(target).certify().spawn_bfs().join()
    assert (c.unique_state_count(), c.state_count()) == (o.unique_state_count, o.state_count)
    cert = assert_certified(c, complete=False)
    assert cert["fifo"] == 1 and cert["states"] <= c.unique_state_count()


@pytest.mark.parametrize("order", BOTH)
def test_every_property_discovered_inside_a_level(order):
    c = certified(sr.SingleCopyRegister(2, 2), order)
    assert len(c.discoveries()) == len(c.properties()) > 0
    cert = assert_certified(c, complete=False)
    assert cert["explored_all"] == 0 and cert["states"] <= c.unique_state_count()


# ---- FIFO order past the oracle's reach -----------------------------------------------------------------------

def test_two_phase_8_fifo_order_with_several_scan_chunks():
    # levels past 524 288 parents take the multi-chunk path of the FIFO scan
    c = certified(sr.TwoPhaseSys(8), "fifo")
    assert counts(c) == two_phase_counts(8)
    cert = assert_certified(c)
    assert cert["fifo"] == 1 and cert["fifo_order"] == cert["fifo_not_first"] == cert["tree_slot"] == 0


# ---- the option is inert --------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["2pc7", "paxos2"])
def test_the_option_changes_nothing_of_the_search(model):
    make = (lambda: sr.TwoPhaseSys(7)) if model == "2pc7" else (lambda: sr.Paxos(2, 3))
    for order in BOTH:
        runs = [make().checker().order(order).profile().certify(on).spawn_bfs().join() for on in (False, True)]
        off, on = runs
        assert counts(off) == counts(on) and sorted(off.discoveries()) == sorted(on.discoveries())
        a, b = off.stats(), on.stats()
        assert (a["table_encoding"], a["levels"], a["rehashes"], a["expand_launches"]) == \
            (b["table_encoding"], b["levels"], b["rehashes"], b["expand_launches"])
        assert [f for _, f in off.launch_profile()] == [f for _, f in on.launch_profile()]
        if order == "fifo":
            for name, path in off.discoveries().items():
                assert on.discovery(name).action_ids == path.action_ids and on.discovery(name).states == path.states
        assert off.certificate()["ran"] == 0 and on.certificate()["ran"] == 1
