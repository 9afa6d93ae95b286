"""The visited set's encodings as the engine itself chooses them (csrc/kernels.hpp make_table_view),
walked through growth on the host: sr_selftest_table_growth (csrc/table_selftest.hpp), and the
encoding rules read back through sr_table_encoding at the points the GPU suite runs
(tests/test_gpu_spread.py). CPU only, nothing is allocated."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stateright_amd import _native as N  # noqa: E402

enc = N.table_encoding


def test_table_growth_selftest():
    assert N.load().sr_selftest_table_growth() == 0, N.last_error()


def test_rehash_selftest_cases_on_the_host():
    # The GPU self-test of the rehash kernels (csrc/rehash_selftest.hpp) with device < 0: every case
    # is built and its expectations come from the host model alone, nothing is launched. The random
    # fills must be predicted to spill, the long run to extend its window at least twice, the
    # constructed spills to have their exact counts, and B = 35 at 2^12 slots to be a pair of slot widths.
    assert N.load().sr_selftest_rehash_gpu(-1) == 0, N.last_error()


def test_78_bit_key_cannot_grow_from_a_small_table():
    # why tests/test_gpu_table_audit.py grows the 78-bit key at F = 22: its smallest table is 2^22 slots
    assert enc(2, 78, 1 << 22)["min_cap_log2"] == 22 and all(enc(w, b, 1 << 12)["min_cap_log2"] <= 12
                                                             for w, b in ((1, 24), (1, 44), (2, 50), (4, 50)))


@pytest.mark.parametrize("words,bits", [(2, 18), (2, 24), (4, 18), (2, 2), (2, 50), (2, 90)])
def test_multi_word_mode_is_fixed_across_the_key_space(words, bits):
    # a multi-word key stays in quotient mode when the table passes its key space (1-bit remainder,
    # as one-word keys), from the partitioned engine's 2^12 head table to past the default table
    for k in range(max(10, enc(words, bits, 1 << 40)["min_cap_log2"]), 35):
        e = enc(words, bits, 1 << k)
        assert e["qbits"] == max(1, bits - k) and e["dbits"] == 64 - e["qbits"] and not e["s32"], (k, e)
        assert e["filter"] == 0  # multi-word quotient tables run without the duplicate filter


@pytest.mark.parametrize("words,bits", [(1, 63), (1, 64), (2, 97), (2, 120), (2, 121), (2, 128), (4, 120), (4, 128)])
def test_wide_keys_are_fingerprinted_at_every_size(words, bits):
    for k in range(10, 35):
        e = enc(words, bits, 1 << k)
        assert (e["qbits"], e["s32"], e["plimit"], e["filter"]) == (0, 0, 65536, 1), (k, e)


def test_one_word_slot_width_rule():
    # 4-byte slots iff the remainder leaves 10 displacement bits in 32; 2^22 slots: B = 44 / 45
    assert enc(1, 44, 1 << 22) == dict(qbits=22, dbits=10, bbits=44, plimit=1022, s32=1, filter=1, filter_log2=9,
                                       min_cap_log2=0)
    e = enc(1, 45, 1 << 22)
    assert (e["qbits"], e["dbits"], e["s32"], e["plimit"]) == (23, 41, 0, 65536)
    assert enc(1, 45, 1 << 23)["s32"] == 1 and enc(1, 46, 1 << 25)["s32"] == 1 and enc(1, 46, 1 << 22)["s32"] == 0
    # past the key space: a 1-bit remainder
    e = enc(1, 13, 1 << 22)
    assert (e["qbits"], e["dbits"], e["s32"]) == (1, 31, 1)
    # the last quotient width, and its smallest table
    e = enc(1, 62, 1 << 22)
    assert (e["qbits"], e["dbits"], e["s32"], e["min_cap_log2"]) == (40, 24, 0, 6)


def test_compact_filter_bound():
    # compact entries for one-word quotient keys of at most 30 + log2(entries) bits
    on = [b for b in range(14, 63) if enc(1, b, 1 << 22)["filter"] == 2]
    assert on == list(range(14, on[-1] + 1))
    log2 = enc(1, on[-1], 1 << 22)["filter_log2"]
    assert on[-1] == 30 + log2
    e = enc(1, on[-1] + 1, 1 << 22)
    assert (e["filter"], e["filter_log2"]) == (1, log2 - 1)


def test_two_word_minimum_table():
    # 8 displacement bits at the least: B = 78 fits the default 2^22 table, 79 needs 2^23
    assert (enc(2, 78, 1 << 22)["dbits"], enc(2, 78, 1 << 22)["plimit"], enc(2, 78, 1 << 22)["min_cap_log2"]) == (8, 254, 22)
    assert enc(2, 79, 1 << 23)["min_cap_log2"] == 23 and enc(2, 79, 1 << 23)["plimit"] == 254
    with pytest.raises(ValueError):
        enc(2, 79, 1 << 22)
    # 85..96 bits: tables past one card (2^29 .. 2^40 slots of 8 bytes at the least)
    assert [enc(2, b, 1 << 40)["min_cap_log2"] for b in (84, 85, 94, 96)] == [28, 29, 38, 40]
