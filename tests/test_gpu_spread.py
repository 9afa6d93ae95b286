"""The visited set driven through every slot encoding with the Spread fixture (csrc/models.hpp Spread):
its key width is a parameter and its state space (the 2^F subsets of F bits) is known in closed form,
so "which encoding" (csrc/kernels.hpp make_table_view: fingerprint, 8-byte and 4-byte quotient slots,
the 1-bit remainder past the key space; the duplicate filter off, 8-byte or compact) is chosen apart
from "how big a run". Everything is compared exactly: small runs (F = 12) with the Python restatement
oracle/pybfs.py spread_bfs (FIFO: visit order and path; FAST: the visited set and a replayed shortest
path), the growth runs (F = 22, the smallest hypercube past the default 2^22 table) and the
partitioned runs (F = 14; F = 17 and 23 where the part tables grow) with the closed forms. Each case
asserts the encoding it is meant to hit from what the run reports (sr_stats: table_capacity,
displacement_limit, table_encoding), and that the engine's rule (sr_table_encoding) says the same."""
import functools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pybfs  # noqa: E402
from audit_lib import assert_clean_audit  # noqa: E402
from stateright_amd import StateRecorder  # noqa: E402
from stateright_amd import _native as N  # noqa: E402
from stateright_amd.models import Spread  # noqa: E402

pytestmark = pytest.mark.gpu

F = 12
MARK = 0b010110011010  # 6 of 12 bits
FP = 65536             # probe limit of fingerprint mode and of >= 17 displacement bits
DEFAULT_LOG2 = 22      # the single-GPU engine's first table


def closed_form(free_bits, loops):
    return 2 ** free_bits, 1 + free_bits * 2 ** (free_bits - 1) + loops * 2 ** free_bits, free_bits


@functools.lru_cache(maxsize=None)
def reference(words, bits, loops):
    r = pybfs.spread_bfs(words, bits, F, loops, MARK)
    assert (r["unique"], r["state_count"], r["max_depth"]) == closed_form(F, loops)
    r["set"] = frozenset(r["visits"])
    return r


def compact_filter_bound():
    """The widest one-word key whose duplicate filter is compact, from the engine's own rule and
    entry count (not a constant of this file)."""
    on = [b for b in range(F + 1, 63) if N.table_encoding(1, b, 1 << DEFAULT_LOG2)["filter"] == 2]
    return on[-1]


# (words, key_bits) -> (log2 slots, remainder bits, 4-byte slots, probe limit, filter) the case is meant to hit
def sweep_cases():
    cb = compact_filter_bound()

    def narrow_limit(b):  # 4-byte slots at 2^22: 32 - (b - 22) displacement bits, limit 2^dbits - 2 below 17 bits
        return (1 << (54 - b)) - 2 if 54 - b < 17 else FP

    one = {13: (22, 1, 1, FP, 2), 22: (22, 1, 1, FP, 2), 23: (22, 1, 1, FP, 2), 32: (22, 10, 1, FP, 2),
           cb: (22, cb - 22, 1, narrow_limit(cb), 2), cb + 1: (22, cb + 1 - 22, 1, narrow_limit(cb + 1), 1),
           44: (22, 22, 1, 1022, 1), 45: (22, 23, 0, FP, 1), 62: (22, 40, 0, FP, 1), 63: (22, 0, 0, FP, 1),
           64: (22, 0, 0, FP, 1)}
    two = {18: (22, 1, 0, FP, 0), 50: (22, 28, 0, FP, 0), 64: (22, 42, 0, FP, 0), 65: (22, 43, 0, FP, 0),
           78: (22, 56, 0, 254, 0), 79: (23, 56, 0, 254, 0), 97: (22, 0, 0, FP, 1), 120: (22, 0, 0, FP, 1),
           121: (22, 0, 0, FP, 1), 128: (22, 0, 0, FP, 1)}
    four = {50: (22, 28, 0, FP, 0), 78: (22, 56, 0, 254, 0), 120: (22, 0, 0, FP, 1), 128: (22, 0, 0, FP, 1)}
    return [(w, b, want) for w, d in ((1, one), (2, two), (4, four)) for b, want in sorted(d.items())]


def ran_with(st):
    """(remainder bits, 4-byte slots, filter: 0 none / 1 8-byte / 2 compact entries, log2 of its entries)
    of the check's final table and its duplicate filter, as the engine reports them (sr_stats.table_encoding)."""
    w = st["table_encoding"]
    flog = w >> 16 & 0xff
    return w & 0xff, w >> 8 & 1, (2 if w >> 24 & 1 else 1) if flog else 0, flog


def check_encoding(c, words, bits, want):
    """The run's table is the one the case is meant to hit: its size, probe limit, slot encoding and
    filter as the run reports them; and the engine's rule (sr_table_encoding) says the same."""
    log2, qbits, s32, plimit, filt = want
    st = c.stats()
    assert st["table_capacity"] == 1 << log2, st
    assert st["displacement_limit"] == plimit, st
    assert st["rehashes"] == 0 and st["restarts"] == 0 and st["table_doublings"] == 0, st
    assert ran_with(st)[:3] == (qbits, s32, filt), (ran_with(st), st)
    e = N.table_encoding(words, bits, st["table_capacity"])
    assert (e["qbits"], e["s32"], e["plimit"], e["filter"], e["filter_log2"]) == (qbits, s32, plimit, filt, ran_with(st)[3]), e
    assert e["dbits"] == ((32 if s32 else 64) - qbits if qbits else 0)


def run(words, bits, loops, order, free_bits=F, mark=MARK, record=True, partitions=1, counters=False):
    b = Spread(words, bits, free_bits, loops, mark).checker().order(order).counters(counters)
    rec = None
    if record:
        rec = StateRecorder()
        b = b.visitor(rec)
    if partitions > 1:
        b = b.partitions(partitions)
    c = b.spawn_bfs().join()
    c.assert_properties()  # "in range" never discovered (every state is the packing of its x), "marked" found
    return c, rec


def check_small(words, bits, loops, order, want=None):
    ref = reference(words, bits, loops)
    c, rec = run(words, bits, loops, order)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == (ref["unique"], ref["state_count"], ref["max_depth"])
    assert sorted(c.discoveries()) == sorted(ref["discoveries"]) == ["marked"]
    path = c.discovery("marked")
    if order == "fifo":
        assert rec.states == ref["visits"]
        assert path.states == ref["discoveries"]["marked"] and path.action_ids == ref["actions"]["marked"]
    else:
        assert len(rec.states) == len(ref["visits"]) and frozenset(rec.states) == ref["set"]
        assert len(path) == bin(MARK).count("1") and path.last_state() == pybfs.spread_describe(words, bits, F, MARK)
        replayed = c.replay(path.action_ids)
        assert replayed is not None and replayed[0] == path.states and replayed[1] == [1, 1]
        assert all(s in ref["set"] for s in path.states)
    if want is not None:
        check_encoding(c, words, bits, want)
    return c


@pytest.mark.parametrize("loops", [0, 2])
@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("words,bits,want", sweep_cases(), ids=lambda v: str(v) if isinstance(v, int) else "enc")
def test_encoding_sweep(words, bits, want, order, loops):
    check_small(words, bits, loops, order, want)


FEW = [(1, 44), (2, 78), (4, 50)]  # one case per state width: 4-byte slots, the shortest probe limit, the wide kernel


@pytest.mark.parametrize("words,bits", FEW)
def test_few_workgroups(words, bits, monkeypatch):
    # two workgroups stride over every chunk of every level, with and without level pipelining
    monkeypatch.setenv("SR_GRID_MAX", "2")
    for pipe in ("1", "0"):
        monkeypatch.setenv("SR_PIPELINE", pipe)
        check_small(words, bits, 2, "fast")


@pytest.mark.parametrize("words,bits", FEW)
def test_probe_queues(words, bits, monkeypatch):
    # the per-lane probe queues (the form of tables past 2^27 slots)
    monkeypatch.setenv("SR_PROBE_BATCH", "-4")
    check_small(words, bits, 2, "fast")


# ---- growth: F = 22, 2^22 states outgrow the default 2^22-slot table ----
GF = 22
GMARK = 0b0101100110100101100110  # 11 of 22 bits
# (words, key_bits, SR_GROW_STEP or None, what the growth is meant to cross)
GROWTH = [
    (1, 45, "2", "8to4"),     # 8-byte slots at 2^22, 4-byte slots from 2^23
    (1, 46, "8", "8to4"),     # the same at 2^25
    (1, 44, None, "4to4"),
    (1, 62, None, "8to8"),
    (1, 24, "8", "past"),     # the table passes the key space: remainder 2 -> 1, the CAS rehash
    (1, 64, None, "fp"),
    (2, 24, None, "past"),    # a two-word key whose table passes its key space
    (2, 60, None, "8to8"),
    (2, 78, "2", "8to8"),
    (2, 78, "8", "8to8"),
    (4, 60, None, "8to8"),
]


def check_growth(words, bits, step, kind, order, monkeypatch, counters=False):
    if step is None:
        monkeypatch.delenv("SR_GROW_STEP", raising=False)
    else:
        monkeypatch.setenv("SR_GROW_STEP", step)
    c, _ = run(words, bits, 0, order, free_bits=GF, mark=GMARK, record=False, counters=counters)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == closed_form(GF, 0)
    path = c.discovery("marked")
    assert len(path) == bin(GMARK).count("1") and path.last_state() == pybfs.spread_describe(words, bits, GF, GMARK)
    assert c.replay(path.action_ids)[0] == path.states
    st = c.stats()
    assert st["rehashes"] >= 1 and st["restarts"] == 0, st
    cap = st["table_capacity"]
    assert cap > 1 << DEFAULT_LOG2 and cap & (cap - 1) == 0, st
    first, last = N.table_encoding(words, bits, 1 << DEFAULT_LOG2), N.table_encoding(words, bits, cap)
    assert st["displacement_limit"] == last["plimit"], (st, last)
    assert ran_with(st) == (last["qbits"], last["s32"], last["filter"], last["filter_log2"]), (ran_with(st), last)
    assert (first["qbits"] != 0) == (last["qbits"] != 0)
    if kind == "8to4":
        assert (first["qbits"] != 0, first["s32"], last["s32"]) == (True, 0, 1), (first, last)
    elif kind == "4to4":
        assert (first["s32"], last["s32"]) == (1, 1), (first, last)
    elif kind == "8to8":
        assert first["qbits"] and last["qbits"] and not first["s32"] and not last["s32"], (first, last)
    elif kind == "past":
        assert first["qbits"] == bits - DEFAULT_LOG2 and last["qbits"] == 1 and cap >= 1 << bits, (first, last)
    elif kind == "quotient":
        assert first["qbits"] == bits - DEFAULT_LOG2 and last["qbits"] == max(1, bits - cap.bit_length() + 1), (first, last)
    else:
        assert first["qbits"] == 0 and last["qbits"] == 0
    if counters:  # the grown table holds exactly the arena's states
        assert_clean_audit(c, fifo=order == "fifo")
    return c


@pytest.mark.parametrize("ranges", ["1", "0"], ids=["ranges", "cas"])
@pytest.mark.parametrize("words,bits,step,kind", GROWTH)
def test_growth(words, bits, step, kind, ranges, monkeypatch):
    monkeypatch.setenv("SR_REHASH_RANGES", ranges)
    check_growth(words, bits, step, kind, "fast", monkeypatch)
    check_growth(words, bits, step, kind, "fast", monkeypatch, counters=True)


def test_growth_fifo_two_word_key_below_its_key_space(monkeypatch):
    # FIFO order: the rehash moves `meta` along and the level's candidate slots are remapped. FIFO
    # grows by doubling, so the 24-bit key ends in 2^23 slots, on its last real remainder bit: the
    # table stays BELOW the key space (k < B), and the FIFO rehash across k = B runs on no GPU; the
    # host self-test covers its arithmetic (reprobe is the same function in both orders).
    # (A 23-bit key would pass its key space here, but 2^22 states fill every home of a 23-bit key
    # space: a table past the key space homes its keys in its first 2^(B-1) slots, so it cannot hold
    # more than about that many states at any size, and such a check ends with SR_ERR_CAPACITY. See
    # DESIGN.md "Which encoding, as tested".)
    check_growth(2, 24, None, "quotient", "fifo", monkeypatch)
    check_growth(2, 24, None, "quotient", "fifo", monkeypatch, counters=True)


# ---- partitioned engine ----
# The partitioned engine explores levels of up to 65 536 states in a replicated head table before the
# partitions take over, so a check this small can end in the head alone unless SR_HEAD_MAX=0 turns it off:
# both are run. Without a hint the part tables are planned for 2^22 states (2^23 slots each), which an
# 18-bit key has passed from the start.
@pytest.mark.parametrize("head", [None, "0"], ids=["head", "parts"])
@pytest.mark.parametrize("words,bits", [(1, 45), (2, 60), (2, 18), (4, 50)])
def test_partitioned(words, bits, head, monkeypatch):
    if head is not None:
        monkeypatch.setenv("SR_HEAD_MAX", head)
    c, rec = run(words, bits, 2, "fast", free_bits=14, mark=0b01011001101001, record=True, partitions=3)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == closed_form(14, 2)
    assert len(rec.states) == 2 ** 14 and sorted(s[0] for s in rec.states) == list(range(2 ** 14))
    assert all(s == pybfs.spread_describe(words, bits, 14, s[0]) for s in rec.states[::97])
    path = c.discovery("marked")
    assert len(path) == 7 and c.replay(path.action_ids)[0] == path.states
    st = c.stats()
    assert st["table_capacity"] == 3 << 23 and st["rehashes"] == 0, st
    e = N.table_encoding(words, bits, 1 << 23)
    assert ran_with(st)[:2] == (e["qbits"], e["s32"]) and st["displacement_limit"] == e["plimit"], (st, e)
    if bits == 18:
        assert ran_with(st)[0] == 1  # quotient mode past the key space (a fingerprint table before)


def part_tables(st, parts):
    """log2 of the slots of one part table (sr_stats.table_capacity is that of all of them)."""
    cap = st["table_capacity"] // parts
    assert cap * parts == st["table_capacity"] and cap & (cap - 1) == 0, st
    return cap.bit_length() - 1


# Part tables that GROW (DistEngine::grow_table), the head off. A capacity hint below the real count
# starts them at 2^16 slots, and 2^17 states in 2 partitions (about 65 536 each, past the 0.75 load of
# 2^16 slots) make each of them grow, to 2^17 slots at the least (the engine grows for the states a
# level may add, so it goes further: 2^19 when this was written, which takes the 18-bit key across
# k = B as well). 39 bits on one word go from 8-byte to 4-byte slots at 2^17.
@pytest.mark.parametrize("words,bits", [(1, 39), (1, 45), (2, 60), (2, 18), (4, 50)])
def test_partitioned_growth(words, bits, monkeypatch):
    monkeypatch.setenv("SR_HEAD_MAX", "0")
    check_partitioned_growth(words, bits, False)
    assert_clean_audit(check_partitioned_growth(words, bits, True), fifo=False)


def check_partitioned_growth(words, bits, counters):
    b = Spread(words, bits, 17, 0, 0b01011001101001011).checker().order("fast").partitions(2).capacity_hint(30000)
    c = b.counters(counters).spawn_bfs().join()
    c.assert_properties()
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == closed_form(17, 0)
    path = c.discovery("marked")
    assert len(path) == 9 and c.replay(path.action_ids)[0] == path.states
    st = c.stats()
    k = part_tables(st, 2)
    assert st["rehashes"] >= 1 and k >= 17, st
    first, last = N.table_encoding(words, bits, 1 << 16), N.table_encoding(words, bits, 1 << k)
    assert first["qbits"] == bits - 16 and last["qbits"] == max(1, bits - k)
    assert ran_with(st)[:2] == (last["qbits"], last["s32"]) and st["displacement_limit"] == last["plimit"], (st, last)
    if (words, bits) == (1, 39):
        assert (first["s32"], last["s32"]) == (0, 1)
    return c


# Part tables that MUST grow across their key space, by load alone: two partitions of an unhinted
# check (part tables of 2^23 slots, grown once a level would load them past 0.45) with F = 23 under a
# 24-bit key hold 4 194 304 states each, more than 0.45 * 2^23, so each ends at 2^24 slots or more
# (k >= B). On two words this is the rehash that collapsed every entry while a multi-word table fell
# back to fingerprints at k >= B.
@pytest.mark.parametrize("words", [1, 2])
def test_partitioned_growth_across_the_key_space(words):
    bits, free_bits, mark = 24, 23, 0b01011001101001011001101
    for counters in (False, True):
        c, _ = run(words, bits, 0, "fast", free_bits=free_bits, mark=mark, record=False, partitions=2, counters=counters)
        assert (c.unique_state_count(), c.state_count(), c.max_depth()) == closed_form(free_bits, 0)
        path = c.discovery("marked")
        assert len(path) == bin(mark).count("1") and c.replay(path.action_ids)[0] == path.states
        st = c.stats()
        k = part_tables(st, 2)
        assert st["rehashes"] >= 1 and k >= bits, st
        assert N.table_encoding(words, bits, 1 << 23)["qbits"] == 1 and ran_with(st)[:2] == (1, 1 if words == 1 else 0), st
    assert_clean_audit(c, fifo=False)
