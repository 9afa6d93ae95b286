"""Host-side check of the FAST expansion's level geometry (no GPU): the function the kernel cuts a
level into workgroup, chunk, wave and lane shares with is walked on the CPU."""


def test_level_geometry_selftest():
    # sr_selftest_level_geometry walks the shares level_geometry (kernels.hpp) yields, the way
    # expand_fast does, for every n in 0..2048 and 2^k - 1, 2^k, 2^k + 1 up to 2^21, 1..48 and
    # 1535..1537 expanding workgroups, caps of 4..64 parents per wave and 4 or 8 waves per workgroup,
    # fixed and balanced: every parent rank of [lo, hi) exactly once and none outside, pw <= cap,
    # cw <= WPB cap, workgroup shares within one chunk width of each other, and the fixed geometry
    # equal to the shift formula (chunk = WPB << ppw_log2) it replaces.
    from stateright_amd import _native
    lib = _native.load()
    assert lib.sr_selftest_level_geometry() == 0, _native.last_error()


def test_stats_mirror_has_balanced_levels():
    from stateright_amd import _native
    assert "balanced_levels" in _native.sr_stats().as_dict()
