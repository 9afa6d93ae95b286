"""The Spread fixture (csrc/models.hpp Spread, SR_MODEL_SPREAD) without a GPU: its independent Python
restatement (oracle/pybfs.py spread_bfs) against the closed forms, the host walk of the compiled
model (describe -> undescribe -> fingerprint over every reachable state), and its parameter checks."""
import ctypes
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pybfs  # noqa: E402
from stateright_amd import _native as N  # noqa: E402

SR_ERR_ARG, SR_ERR_UNSUPPORTED = -1, -4


def closed_form(free_bits, loops):
    """(unique, state_count, depth) of Spread(.., free_bits, loops, ..)."""
    return 2 ** free_bits, 1 + free_bits * 2 ** (free_bits - 1) + loops * 2 ** free_bits, free_bits


@pytest.mark.parametrize("words,bits,free_bits,loops", [
    (1, 13, 12, 0), (1, 45, 12, 2), (1, 64, 9, 4), (2, 18, 12, 2), (2, 128, 11, 0), (4, 50, 7, 1), (4, 128, 12, 2),
    (1, 2, 1, 0)])
def test_spread_bfs_matches_closed_forms(words, bits, free_bits, loops):
    mark = int("0101" * 6, 2) & (2 ** free_bits - 1)
    r = pybfs.spread_bfs(words, bits, free_bits, loops, mark)
    assert (r["unique"], r["state_count"], r["max_depth"]) == closed_form(free_bits, loops)
    # FIFO visits level by level: C(F, L) states of L bits
    levels = [bin(s[0]).count("1") for s in r["visits"]]
    assert levels == sorted(levels) and [levels.count(k) for k in range(free_bits + 1)] == \
        [math.comb(free_bits, k) for k in range(free_bits + 1)]
    # described states: x, then the halves of `words` words that hold a key below 2^bits, x in its low bits
    for s in r["visits"][:64] + r["visits"][-64:]:
        assert len(s) == 1 + 2 * words and all(0 <= h < 2 ** 32 for h in s[1:])
        key = sum(h << (32 * i) for i, h in enumerate(s[1:5]))
        assert key < 2 ** bits and key % 2 ** free_bits == s[0]
    assert len(set(r["visits"])) == 2 ** free_bits
    assert sorted(r["discoveries"]) == ["marked"]
    path = r["discoveries"]["marked"]
    assert path[-1][0] == mark and len(path) - 1 == bin(mark).count("1") == len(r["actions"]["marked"])


def closed_form_roots(free_bits, loops, roots, dup):
    """(unique, state_count, depth) with the init states 0 .. roots-1, then 0 .. dup-1 again: x = 0 is a
    root, so every subset is reachable; every duplicate root is popped and expanded a second time; a
    state's depth is the fewest bits it adds to a root inside it."""
    count = (roots + dup) + free_bits * 2 ** (free_bits - 1) + loops * 2 ** free_bits + \
        sum(free_bits - bin(i).count("1") + loops for i in range(dup))
    depth = max(min(bin(x ^ r).count("1") for r in range(roots) if r & ~x == 0) for x in range(2 ** free_bits))
    return 2 ** free_bits, count, depth


@pytest.mark.parametrize("words,bits,free_bits,loops,roots,dup", [
    (1, 13, 4, 0, 16, 16), (1, 45, 5, 2, 3, 1), (1, 64, 6, 4, 33, 0), (2, 18, 7, 2, 128, 5), (2, 128, 8, 0, 40, 3),
    (4, 50, 9, 1, 256, 256), (4, 128, 10, 2, 300, 100), (1, 32, 11, 1, 257, 64), (1, 45, 12, 2, 65, 7), (4, 78, 12, 0, 8, 0)])
def test_spread_bfs_with_roots_matches_closed_forms(words, bits, free_bits, loops, roots, dup):
    mark = int("0111" * 3, 2) & (2 ** free_bits - 1)
    r = pybfs.spread_bfs(words, bits, free_bits, loops, mark, roots, dup)
    assert (r["unique"], r["state_count"], r["max_depth"]) == closed_form_roots(free_bits, loops, roots, dup)
    if roots & (roots - 1) == 0:  # roots = 2^j: the low j bits are free from the start
        assert r["max_depth"] == free_bits - (roots.bit_length() - 1)
    xs = [s[0] for s in r["visits"]]
    inits = pybfs.spread_inits(roots, dup)
    assert inits == list(range(roots)) + list(range(dup))
    assert xs[:roots + dup] == inits[::-1]  # popped from the back: level 0 in reverse init order
    seen = {}
    for x in xs:
        seen[x] = seen.get(x, 0) + 1
    assert sorted(seen) == list(range(2 ** free_bits))
    assert all(n == (2 if x < dup else 1) for x, n in seen.items())  # a duplicate root is visited twice
    # the discovery: a shortest path, from the root inside the mark that is nearest to it
    path, acts = r["discoveries"]["marked"], r["actions"]["marked"]
    assert path[0][0] in inits and path[-1][0] == mark
    assert len(acts) == len(path) - 1 == min(bin(mark ^ x).count("1") for x in range(roots) if x & ~mark == 0)
    x = path[0][0]
    for a, s in zip(acts, path[1:]):  # each action sets one clear bit, whichever root the path starts at
        assert not x >> a & 1
        x |= 1 << a
        assert s == pybfs.spread_describe(words, bits, free_bits, x)


def test_spread_filler_reaches_every_key_bit():
    # every key bit up to B - 1 takes both values over the states (so every slot field is exercised)
    for words, bits in ((1, 64), (2, 128), (2, 79)):
        seen_or, seen_and = 0, (1 << bits) - 1
        for x in range(256):
            w = pybfs.spread_words(words, bits, 8, x)
            key = w[0] | (w[1] << 64 if words > 1 else 0)
            seen_or |= key
            seen_and &= key
        assert seen_or == (1 << bits) - 1 and seen_and == 0


@pytest.mark.parametrize("params,want", [
    ([1, 13, 12, 0, 0], 4096), ([1, 64, 10, 2, 5], 1024), ([2, 18, 12, 2, 0], 4096), ([2, 128, 10, 0, 0], 1024),
    ([4, 50, 10, 1, 0], 1024), ([4, 128, 12, 4, 0], 4096),
    # 40 init states and 3 duplicates of them: the same 2^12 states
    ([1, 45, 12, 0, 0, 40, 3], 4096), ([2, 79, 12, 0, 0, 40, 3], 4096), ([4, 128, 12, 0, 0, 40, 3], 4096)])
def test_compiled_model_describe_roundtrip(params, want):
    p = (ctypes.c_int64 * len(params))(*params)
    n = N.load().sr_selftest_describe(N.SR_MODEL_SPREAD, p, len(params), want + 1)
    assert n == want, N.last_error()


def test_compiled_model_packs_like_the_restatement():
    # the engine's fingerprint of a described state exists only if undescribe -> describe gives the
    # description back, i.e. if the compiled model derives the same x from the restatement's words
    from stateright_amd.models import Spread
    from stateright_amd.plugin import model_fingerprint
    for words, bits in ((1, 45), (2, 79), (4, 128)):
        m = Spread(words, bits, 12, 0, 0)
        fps = {model_fingerprint(m, list(pybfs.spread_describe(words, bits, 12, x))) for x in (0, 1, 77, 4095)}
        assert len(fps) == 4 and 0 not in fps
        bad = list(pybfs.spread_describe(words, bits, 12, 77))
        bad[0] = 78  # x that is not the words' low bits
        with pytest.raises(ValueError):
            model_fingerprint(m, bad)


@pytest.mark.parametrize("params,code", [
    ([1, 12, 12, 0, 0], SR_ERR_UNSUPPORTED),   # B <= F
    ([1, 5, 12, 0, 0], SR_ERR_UNSUPPORTED),
    ([1, 65, 12, 0, 0], SR_ERR_UNSUPPORTED),   # B > 64 W
    ([2, 129, 12, 0, 0], SR_ERR_UNSUPPORTED),
    ([4, 129, 12, 0, 0], SR_ERR_UNSUPPORTED),  # B > 128
    ([3, 40, 12, 0, 0], SR_ERR_UNSUPPORTED),   # W = 3
    ([1, 40, 12, 5, 0], SR_ERR_UNSUPPORTED),   # loops > 4
    ([1, 40, 25, 0, 0], SR_ERR_UNSUPPORTED),   # F > 24
    ([1, 40, 12, 0, 4096], SR_ERR_ARG),        # mark past 2^F
    ([1, 40, 12, 0], SR_ERR_ARG),              # a parameter short
    ([1, 40, 12, 0, 0, 0, 0], SR_ERR_ARG),     # roots = 0
    ([1, 40, 4, 0, 0, 17, 0], SR_ERR_ARG),     # roots > 2^F
    ([1, 40, 12, 0, 0, 4, 5], SR_ERR_ARG),     # dup > roots
    ([1, 40, 12, 0, 0, 4, -1], SR_ERR_ARG),    # dup < 0
    ([1, 40, 12, 0, 0, 257, 256], SR_ERR_UNSUPPORTED),  # roots + dup > 512
    ([1, 40, 12, 0, 0, 4, 1, 0], SR_ERR_ARG),  # a parameter too many
])
def test_bad_parameters_are_refused(params, code):
    p = (ctypes.c_int64 * len(params))(*params)
    assert N.load().sr_selftest_describe(N.SR_MODEL_SPREAD, p, len(params), 10) == code
    assert "spread" in N.last_error()


def test_roots_and_dup_are_appended_only_when_given():
    from stateright_amd.models import Spread
    assert Spread(1, 45, 12, 2, 5).params() == [1, 45, 12, 2, 5]
    assert Spread(1, 45, 12, 2, 5, 1, 0).params() == [1, 45, 12, 2, 5]
    assert Spread(1, 45, 12, 2, 5, roots=40).params() == [1, 45, 12, 2, 5, 40, 0]
    assert Spread(1, 45, 12, 2, 5, 40, 3).params() == [1, 45, 12, 2, 5, 40, 3]
    p = (ctypes.c_int64 * 7)(4, 128, 12, 0, 0, 256, 256)  # the bounds themselves are accepted
    assert N.load().sr_selftest_describe(N.SR_MODEL_SPREAD, p, 7, 5000) == 4096, N.last_error()
