"""The visited set's growth kernels on synthetic tables (csrc/rehash_selftest.hpp,
sr_selftest_rehash_gpu): rehash_ranges<u32|u64> + rehash_spill, the CAS rehash with meta and
remap_slots, launched through the engines' own growth routine and compared slot by slot with a
sequential host rebuild. The cases (an empty table, the table's two ends, a cluster wrapped round
the old table's end, spills into the next range and round the new table's end, a run longer than the
first window, one-range tables and the window's clamp, random fills that must spill, 8-byte slots
growing into 4-byte ones, the error word on a lowered probe limit and on a spill list of one entry
with its guard word) are listed there; the first failing one is named in the error."""
import pytest

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")
from stateright_amd import _native as N  # noqa: E402


def test_rehash_kernels_match_the_host_rebuild():
    assert N.load().sr_selftest_rehash_gpu(0) == 0, N.last_error()
