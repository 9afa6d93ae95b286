"""The visited set audited against the arena after every kind of growth (csrc/kernels_audit.hpp,
checker.table_audit()): a check run with counters() compares its final table with its arena, which
lists every visited state. The growth tests elsewhere compare counts, and counts come from the
claims counter: in a graded model (Spread: level = popcount; increment_lock: level = the sum of the
program counters) a state is generated from the level before it and never again, so a rehash that
dropped, duplicated or misfiled an older entry would pass them. Here every run asserts a clean
audit: no misplaced or duplicate slot, every arena state found in a slot of its own, in FIFO order
the slot's meta naming the state's level and parent, and occupied == arena states == unique states
(exact; no tolerance anywhere).

The growth reached: synchronous growth from a tiny first table (SR_TABLE_LOG2) by every step, by
ranges and by CAS, in both orders; the enqueued early growth of unhinted checks; the doubling in
the middle of a level (SR_DISP_LIMIT); tables recycled without a clear; part tables; and an
enqueued or a synchronous rehash that reports a full table (SR_REHASH_FAIL)."""
import pytest

from audit_lib import assert_clean_audit

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")
from stateright_amd.distributed import Communicator  # noqa: E402
from stateright_amd.models import Spread  # noqa: E402


def spread_counts(free_bits, loops):
    return 2 ** free_bits, 1 + free_bits * 2 ** (free_bits - 1) + loops * 2 ** free_bits, free_bits


def two_phase_counts(n):
    return 6 ** n + 4 ** n + 2 ** n, (4 * n * 6 ** n + 3 * (n + 1) * 4 ** n + 3 * n * 2 ** n + 6) // 3, 3 * n + 1


def counts(c):
    return c.unique_state_count(), c.state_count(), c.max_depth()


MARK16 = 0b0101100110100101
MARK22 = 0b0101100110100101100110

# (words, key bits, free bits). F = 16 wherever 2^16 states outgrow the model's smallest table (2^12
# slots here, SR_TABLE_LOG2). A 78-bit key cannot: its remainder fills a slot's 56 bits only from
# 2^22 slots up (min_table_cap), which 2^16 states load to 1.6%; it takes the smallest hypercube
# that outgrows 2^22 slots, F = 22, with the same assertions.
TINY = [(1, 24, 16), (1, 44, 16), (2, 50, 16), (2, 78, 22), (4, 50, 16)]


@pytest.mark.parametrize("order", ["fast", "fifo"])
@pytest.mark.parametrize("ranges", ["1", "0"], ids=["ranges", "cas"])
@pytest.mark.parametrize("step", ["2", "8", "64"])
@pytest.mark.parametrize("words,bits,free_bits", TINY)
def test_synchronous_growth_from_a_tiny_table(words, bits, free_bits, step, ranges, order, monkeypatch):
    # A hinted check does not grow early (enqueued): every growth here waits for its rehash. The
    # hint is far below the state count, so the first table is the smallest and grows repeatedly.
    monkeypatch.setenv("SR_TABLE_LOG2", "12")
    monkeypatch.setenv("SR_GROW_STEP", step)
    monkeypatch.setenv("SR_REHASH_RANGES", ranges)
    loops = 1 if free_bits == 16 else 0
    mark = MARK16 if free_bits == 16 else MARK22
    c = Spread(words, bits, free_bits, loops, mark).checker().order(order).capacity_hint(1000).counters().spawn_bfs().join()
    c.assert_properties()
    assert counts(c) == spread_counts(free_bits, loops)
    st = c.stats()
    assert st["rehashes"] >= 1, st
    assert_clean_audit(c, fifo=order == "fifo")


@pytest.mark.parametrize("model", ["spread1", "spread2", "2pc8", "2pc8-small", "2pc9"])
def test_unhinted_growth(model, monkeypatch):
    # Without a hint the first growth is enqueued behind the level in flight (grow_table_async) and
    # its outcome read later; a restart would hide a failed one. 2pc N=8 (1 745 408 states) stays
    # within the default 2^22 slots and grows nothing; it does from a first table of 2^20, and N=9
    # does from the default one.
    if model.startswith("2pc"):
        n = int(model[3])
        if model == "2pc8-small":
            monkeypatch.setenv("SR_TABLE_LOG2", "20")
        c = sr.TwoPhaseSys(n).checker().order("fast").counters().spawn_bfs().join()
        assert counts(c) == two_phase_counts(n)
        assert (c.stats()["rehashes"] >= 1) == (model != "2pc8"), c.stats()
    else:
        words, bits = (1, 44) if model == "spread1" else (2, 50)
        c = Spread(words, bits, 22, 0, MARK22).checker().order("fast").counters().spawn_bfs().join()
        assert counts(c) == spread_counts(22, 0)
        assert c.stats()["rehashes"] >= 1, c.stats()
    assert c.stats()["restarts"] == 0, c.stats()
    assert_clean_audit(c, fifo=False)


@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("order", ["fifo", "fast"])
@pytest.mark.parametrize("model", ["2pc7", "inclock9"])
def test_mid_level_doubling(model, order, pipe, monkeypatch):
    # A level overflows the lowered probe limit: the table doubles in the middle of it and the level
    # is finished on the new one. FIFO: the level's candidate slots are remapped, meta moves along.
    monkeypatch.setenv("SR_DISP_LIMIT", "3" if model == "2pc7" else "6")
    monkeypatch.setenv("SR_PIPELINE", pipe)
    if model == "2pc7":
        c = sr.TwoPhaseSys(7).checker().order(order).counters().spawn_bfs().join()
        assert counts(c) == two_phase_counts(7)
    else:
        import math
        n = 9
        expect = 1 + 4 * sum(math.factorial(n) // math.factorial(n - k) for k in range(1, n + 1))
        c = sr.IncrementLock(n).checker().order(order).counters().spawn_bfs().join()
        assert counts(c) == (expect, expect, 4 * n)
    assert c.stats()["table_doublings"] > 0, c.stats()
    assert_clean_audit(c, fifo=order == "fifo")


def test_recycled_and_unzeroed_tables():
    # An unhinted check that grew by ranges hands its table back without a clear; the checks after
    # it in this process take pooled blocks: a hinted one clears what it takes, an unhinted one
    # grows into a dirty block that rehash_ranges has to overwrite whole. A stale entry that
    # happens not to collide shows in occupied == unique alone.
    n = 9
    first = sr.TwoPhaseSys(n).checker().order("fast").spawn_bfs().join()  # no counters(): the table is released
    assert counts(first) == two_phase_counts(n) and first.stats()["rehashes"] >= 1
    hinted = Spread(1, 44, 20, 0, MARK16).checker().order("fast").capacity_hint(2 ** 20).counters().spawn_bfs().join()
    assert counts(hinted) == spread_counts(20, 0)
    assert_clean_audit(hinted, fifo=False)
    unhinted = Spread(1, 44, 22, 0, MARK22).checker().order("fast").counters().spawn_bfs().join()
    assert counts(unhinted) == spread_counts(22, 0) and unhinted.stats()["rehashes"] >= 1
    assert_clean_audit(unhinted, fifo=False)
    again = sr.TwoPhaseSys(n).checker().order("fast").counters().spawn_bfs().join()
    assert counts(again) == two_phase_counts(n) and again.stats()["rehashes"] >= 1
    assert_clean_audit(again, fifo=False)


PMARK = 0b01011001101001011


@pytest.mark.parametrize("head", ["0", "4096", None], ids=["parts", "handover", "head"])
@pytest.mark.parametrize("words,bits", [(1, 39), (2, 60)])
def test_partitioned_growth(words, bits, head, monkeypatch):
    # Part tables that grow (a hint below the real count starts them at 2^16 slots), audited per part
    # against the part's arena. With a replicated head of up to 4096 states per level the parts take
    # over in the middle of the check: each part's table also holds its share of the head's levels,
    # which only the head arena lists. With the default head (65 536) the whole check ends inside it,
    # nothing grows, and the head's own table is audited.
    if head is None:
        monkeypatch.delenv("SR_HEAD_MAX", raising=False)
    else:
        monkeypatch.setenv("SR_HEAD_MAX", head)
    c = Spread(words, bits, 17, 0, PMARK).checker().order("fast").partitions(2).capacity_hint(30000).counters().spawn_bfs().join()
    c.assert_properties()
    assert counts(c) == spread_counts(17, 0)
    assert (c.stats()["rehashes"] >= 1) == (head is not None), c.stats()
    assert (c.stats()["head_levels"] > 0) == (head == "4096"), c.stats()
    assert_clean_audit(c, fifo=False)


def test_two_ranks_growth(monkeypatch):
    # The same shape on two ranks in this process: each rank audits its own part, the figures are
    # summed over the ranks, and every rank reports the sum.
    monkeypatch.setenv("SR_HEAD_MAX", "0")
    comms = Communicator.local_group(2)
    cs = []
    try:
        for comm in comms:
            cs.append(Spread(1, 39, 17, 0, PMARK).checker().comm(comm).capacity_hint(30000).counters().spawn_bfs())
        for c in cs:
            c.join()
        for c in cs:
            assert counts(c) == spread_counts(17, 0)
            assert c.stats()["rehashes"] >= 1, c.stats()
            assert_clean_audit(c, fifo=False)
        assert cs[0].table_audit() == cs[1].table_audit()
    finally:
        cs.clear()
        for comm in comms:
            comm.close()


@pytest.mark.parametrize("n,table_log2", [(8, "20"), (9, None)])
def test_failed_enqueued_rehash_restarts_and_stays_exact(n, table_log2, monkeypatch):
    # SR_REHASH_FAIL=1: the first growth of the check, the early growth enqueued behind a level, has
    # ERR_TABLE_FULL stored into its error word behind the rehash (nothing on the device is
    # corrupted). The outcome is read at the next synchronous point and the check restarts with
    # larger buffers; counts stay exact and the final table is clean. Unhinted 2pc N=9 grows early
    # from the default table; N=8 fits the default table (test_unhinted_growth), so it starts at 2^20 slots.
    if table_log2:
        monkeypatch.setenv("SR_TABLE_LOG2", table_log2)
    monkeypatch.setenv("SR_REHASH_FAIL", "1")
    c = sr.TwoPhaseSys(n).checker().order("fast").counters().spawn_bfs().join()
    assert counts(c) == two_phase_counts(n)
    assert c.stats()["restarts"] >= 1, c.stats()
    assert_clean_audit(c, fifo=False)


def test_failed_synchronous_rehash_grows_further(monkeypatch):
    # A synchronous growth that reports a full table is redone into a table twice as large, with no
    # restart: aimed at the last growth of the check, the table ends larger than without the knob.
    monkeypatch.setenv("SR_TABLE_LOG2", "12")
    monkeypatch.setenv("SR_GROW_STEP", "2")

    def check():
        c = Spread(1, 44, 16, 0, MARK16).checker().order("fast").capacity_hint(1000).counters().spawn_bfs().join()
        assert counts(c) == spread_counts(16, 0)
        assert c.stats()["restarts"] == 0, c.stats()
        assert_clean_audit(c, fifo=False)
        return c.stats()

    base = check()
    assert base["rehashes"] >= 1, base
    monkeypatch.setenv("SR_REHASH_FAIL", str(base["rehashes"]))
    failed = check()
    assert failed["table_capacity"] > base["table_capacity"], (base, failed)
