"""ORACLE — TEST INFRASTRUCTURE ONLY. A pure-Python restatement of the reference's single-threaded
breadth-first checker (src/checker/bfs.rs) for small models given as Python functions, and the
sliding puzzle of the reference crate's documentation (src/lib.rs:40-116), the model of the
example GpuModel plugin (examples/plugins/sliding_puzzle.hip). Pinned by that doc test: the puzzle
[1,4,2,3,5,8,6,7,0] discovers "solved" and [Down, Right, Down, Right] is a valid discovery
(src/lib.rs:89-115). No product path imports this file.
"""
from collections import deque

ALWAYS, EVENTUALLY, SOMETIMES = 0, 1, 2


def bfs(init_states, actions, next_state, properties, within_boundary=lambda s: True):
    """bfs.rs:36-342 with thread_count = 1: init states filtered by the boundary and queued in init
    order, popped from the back with successors pushed to the front (FIFO); properties evaluated
    at pop (always: discovery when the condition fails; sometimes: when it holds); a pop finding
    every property discovered stops; `generated` keeps the first generator (parent) of every state.
    Returns dict(unique, state_count, discoveries={name: [states...]}, visits=[states])."""
    inits = [s for s in init_states if within_boundary(s)]
    generated = {}
    depth = {}
    for s in inits:
        generated.setdefault(s, None)
        depth.setdefault(s, 0)
    state_count = len(inits)
    pending = deque(inits)  # pop from the back, push to the front (bfs.rs:61-66,183,263)
    discoveries = {}
    visits = []
    while pending:
        s = pending.pop()
        visits.append(s)
        awaiting = False
        for name, exp, cond in properties:
            if name in discoveries:
                continue
            if exp == ALWAYS and not cond(s):
                discoveries[name] = s
            elif exp == SOMETIMES and cond(s):
                discoveries[name] = s
            else:
                awaiting = True
        if not awaiting:  # bfs.rs:226 (nothing left to discover: the worker stops)
            break
        for a in actions(s):
            ns = next_state(s, a)
            if ns is None or not within_boundary(ns):
                continue
            state_count += 1
            if ns not in generated:
                generated[ns] = s
                depth[ns] = depth[s] + 1
                pending.appendleft(ns)

    def path(t):
        out = []
        while t is not None:
            out.append(t)
            t = generated[t]
        return out[::-1]

    return {"unique": len(generated), "state_count": state_count, "visits": visits,
            "max_depth": max(depth.values(), default=0),
            "discoveries": {n: path(s) for n, s in discoveries.items()}}


# ---- the Spread fixture (stateright_amd/csrc/models.hpp Spread), restated independently ----
M64 = (1 << 64) - 1


def fmix64(k):
    """murmur3's 64-bit finalizer."""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def spread_chunk(x, c):
    return fmix64((x + 0x9E3779B97F4A7C15 * (2 * c + 1)) & M64)


def spread_words(words, key_bits, free_bits, x):
    """The packed state of the subset x: key = (x | filler << free_bits) mod 2^key_bits in words 0
    and 1 (little-endian), filler chunks 2 and 3 in words 2 and 3 of a four-word state."""
    fill = spread_chunk(x, 0) | spread_chunk(x, 1) << 64
    key = (x | fill << free_bits) & ((1 << key_bits) - 1)
    out = [key & M64, key >> 64, spread_chunk(x, 2), spread_chunk(x, 3)]
    return tuple(out[:words])


def spread_describe(words, key_bits, free_bits, x):
    """x, then the low and the high 32 bits of every word."""
    d = [x]
    for w in spread_words(words, key_bits, free_bits, x):
        d += [w & 0xffffffff, w >> 32]
    return tuple(d)


def spread_inits(roots=1, dup=0):
    """The subsets that are Spread's init states, in init order: 0 .. roots-1, then 0 .. dup-1 again."""
    return list(range(roots)) + list(range(dup))


def spread_bfs(words, key_bits, free_bits, loops=0, mark=0, roots=1, dup=0):
    """Spread(words, key_bits, free_bits, loops, mark, roots, dup) on bfs(): states are described
    states (spread_describe); action j < free_bits sets bit j of x where it is clear, actions
    free_bits .. free_bits + loops - 1 return the state itself. always "in range" (x < 2^free_bits),
    sometimes "marked" (x == mark). The init states are spread_inits(roots, dup). Adds `actions`: per
    discovery, the action ids along its path (each step sets one bit, whichever root the path starts at)."""
    assert words in (1, 2, 4) and free_bits < key_bits <= min(64 * words, 128) and 0 <= loops <= 4
    assert 1 <= roots <= 1 << free_bits and 0 <= dup <= roots and roots + dup <= 512
    packed = {}

    def d(x):  # (two subsets never pack alike: x is the key's low bits)
        if x not in packed:
            packed[x] = spread_describe(words, key_bits, free_bits, x)
        return packed[x]

    def actions(s):
        return [j for j in range(free_bits) if not s[0] >> j & 1] + [free_bits + j for j in range(loops)]

    def next_state(s, a):
        return d(s[0] | 1 << a) if a < free_bits else s

    r = bfs([d(x) for x in spread_inits(roots, dup)], actions, next_state,
            [("in range", ALWAYS, lambda s: s[0] < 1 << free_bits), ("marked", SOMETIMES, lambda s: s[0] == mark)])
    r["actions"] = {name: [(b[0] ^ a[0]).bit_length() - 1 for a, b in zip(path, path[1:])]
                    for name, path in r["discoveries"].items()}
    return r


# ---- the sliding puzzle (src/lib.rs:43-88) ----
SLIDES = ("Down", "Up", "Right", "Left")
SOLVED = (0, 1, 2, 3, 4, 5, 6, 7, 8)


def puzzle_next(state, action):
    empty = state.index(0)
    y, x = divmod(empty, 3)
    frm = {"Down": empty - 3 if y > 0 else None, "Up": empty + 3 if y < 2 else None,
           "Right": empty - 1 if x > 0 else None, "Left": empty + 1 if x < 2 else None}[action]
    if frm is None:
        return None
    ns = list(state)
    ns[empty] = state[frm]
    ns[frm] = 0
    return tuple(ns)


def puzzle_bfs(cells):
    return bfs([tuple(cells)], lambda s: SLIDES, puzzle_next, [("solved", SOMETIMES, lambda s: s == SOLVED)])


def puzzle_replay(cells, actions):
    s = tuple(cells)
    states = [s]
    for a in actions:
        s = puzzle_next(s, a)
        if s is None:
            return None
        states.append(s)
    return states
