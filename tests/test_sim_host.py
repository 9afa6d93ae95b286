"""The simulation checker's walk on the host (sr_sim_walk, csrc/sim.hpp): the same code the kernel
runs, checked here without a device against the independent CPU oracle."""
import math

import pytest

import oracle_lib
from oracle_lib import dgraph_params
from stateright_amd import _native as N

SEED = 20240607
TERMINAL, DEPTH = N.SIM_TERMINAL, N.SIM_DEPTH
ALWAYS, EVENTUALLY, SOMETIMES = N.SR_ALWAYS, N.SR_EVENTUALLY, N.SR_SOMETIMES


def walk(model, params, i, max_depth=64, seed=SEED, nprops=8):
    return N.sim_walk(model, params, seed, i, max_depth, nprops)


# ---- determinism -------------------------------------------------------------------------------

def test_same_seed_and_walk_twice():
    for i in (0, 1, 77, 2**39):
        assert walk(N.SR_MODEL_2PC, [3], i) == walk(N.SR_MODEL_2PC, [3], i)


def test_consecutive_walks_differ_and_seeds_differ():
    a = [walk(N.SR_MODEL_2PC, [3], i)["actions"] for i in range(256)]
    assert len({tuple(x) for x in a}) > 1
    b = [walk(N.SR_MODEL_2PC, [3], i, seed=SEED + 1)["actions"] for i in range(256)]
    assert any(x != y for x, y in zip(a, b))


# ---- validity against the CPU oracle -----------------------------------------------------------

DG_PATHS = [[0, 1, 4, 6], [2, 4, 8]]
# (model id, params, expectations per property, oracle params per first action or None)
VALIDITY = {
    "2pc3": (N.SR_MODEL_2PC, [3], [SOMETIMES, SOMETIMES, ALWAYS]),
    "increment_lock3": (N.SR_MODEL_INCREMENT_LOCK, [3], [ALWAYS, ALWAYS]),
    "linear_equation": (N.SR_MODEL_LINEAR_EQUATION, [2, 10, 14], [SOMETIMES]),
    "dgraph": (N.SR_MODEL_DGRAPH, dgraph_params(SOMETIMES, DG_PATHS), [SOMETIMES]),
}


def oracle_params(name, params, actions):
    """The oracle replays from its FIRST init state only. The DGraph has two (0 and 2): a walk from 2
    (its first action is 4; from 0 it is 1) is replayed on the sub-graph reachable from 2, written
    with 2 as its lowest init state (2 -> 4 -> {6, 8}), which has the same edges there."""
    if name == "dgraph" and actions and actions[0] == 4:
        return dgraph_params(SOMETIMES, [[2, 4, 8], [4, 6]])
    return params


@pytest.mark.parametrize("name", sorted(VALIDITY))
def test_walks_replay_on_the_oracle(name):
    model, params, expect = VALIDITY[name]
    seen_hit = False
    for i in range(200):
        w = walk(model, params, i)
        assert w["steps"] == len(w["actions"]) <= 64
        assert w["end"] in (TERMINAL, DEPTH)
        if name == "dgraph":  # (the walk against the model's own edges: a DGraph action is its destination)
            edges = {(p[k], p[k + 1]) for p in DG_PATHS for k in range(len(p) - 1)}
            nodes = [0 if w["actions"][0] == 1 else 2] + w["actions"]
            assert all(e in edges for e in zip(nodes, nodes[1:])), f"walk {i}: {nodes}"
            assert w["end"] == TERMINAL and nodes[-1] in (6, 8)
        op = oracle_params(name, params, w["actions"])
        first = [-1] * len(expect)
        for t in range(w["steps"] + 1):  # every prefix: the oracle gives the last state's conditions
            r = oracle_lib.replay(model, op, w["actions"][:t], len(expect))
            assert r is not None, f"walk {i}: the oracle refuses step {t} of {w['actions']}"
            _, holds = r
            for p, e in enumerate(expect):
                discovered = (not holds[p]) if e == ALWAYS else bool(holds[p])
                if discovered and first[p] < 0:
                    first[p] = t
        assert w["first_hit"][:len(expect)] == first, f"walk {i}"
        seen_hit = seen_hit or any(f >= 0 for f in first)
    if name != "increment_lock3":  # (its properties hold everywhere)
        assert seen_hit


# ---- end reasons -------------------------------------------------------------------------------

def test_ladder_ends_terminal_after_five_steps():
    for i in range(50):
        w = walk(N.SR_MODEL_LADDER, [3, 2], i)
        assert (w["steps"], w["end"]) == (5, TERMINAL)


@pytest.mark.parametrize("max_depth", [1, 7, 64])
def test_binary_clock_ends_at_depth(max_depth):
    for i in range(20):
        w = walk(N.SR_MODEL_BINARY_CLOCK, [], i, max_depth)
        assert (w["steps"], w["end"]) == (max_depth, DEPTH)


def test_pingpong_redraws_refused_slots():
    # max_nat = 1: Deliver slots stay listed whose next state is outside the boundary
    ws = [walk(N.SR_MODEL_PINGPONG, [1, 0, 1, 0], i) for i in range(200)]
    assert any(w["attempts"] > 0 for w in ws)
    assert all(w["end"] == TERMINAL for w in ws if w["steps"] < 64)


# ---- eventually --------------------------------------------------------------------------------

def test_eventually_hit_only_at_a_terminal_state_that_never_satisfied_it():
    params = dgraph_params(EVENTUALLY, [[0, 1], [0, 2]])
    ends = set()
    for i in range(200):
        w = walk(N.SR_MODEL_DGRAPH, params, i, nprops=1)
        assert (w["steps"], w["end"]) == (1, TERMINAL)
        ends.add(w["actions"][0])
        assert w["first_hit"] == ([1] if w["actions"][0] == 2 else [-1])
    assert ends == {1, 2}


def test_eventually_on_a_cycle_has_no_hit():
    params = dgraph_params(EVENTUALLY, [[0, 2, 4, 2]])
    for i in range(50):
        w = walk(N.SR_MODEL_DGRAPH, params, i, nprops=1)
        assert (w["steps"], w["end"], w["first_hit"]) == (64, DEPTH, [-1])


# ---- the chooser -------------------------------------------------------------------------------

def test_chooser_is_uniform_over_the_enabled_slots():
    # 2pc N = 3 at its init state lists TmAbort and, per rm, RmPrepare and RmChooseToAbort
    # (examples/2pc.rs:56-81): slots 1 and 2 + 5 rm + {1, 2}
    slots = [1] + [2 + 5 * rm + k for rm in range(3) for k in (1, 2)]
    n = 65536
    counts = dict.fromkeys(slots, 0)
    for i in range(n):
        w = walk(N.SR_MODEL_2PC, [3], i, 1, nprops=3)
        assert w["steps"] == 1
        counts[w["actions"][0]] += 1  # (a slot enabled() does not list is a KeyError)
    p = 1 / len(slots)
    sd = math.sqrt(n * p * (1 - p))
    for s, c in counts.items():
        assert c > 0 and abs(c - n * p) <= 6 * sd, (s, c, n * p, sd)


def test_init_draw_is_uniform_over_forty_init_states():
    # 40 init nodes, each with a successor of its own: the first action names the init state drawn
    roots = list(range(100, 140))
    params = dgraph_params(SOMETIMES, [[r, r + 100] for r in roots])
    n = 65536
    counts = dict.fromkeys(roots, 0)
    for i in range(n):
        w = walk(N.SR_MODEL_DGRAPH, params, i, 1, nprops=1)
        assert w["steps"] == 1
        counts[w["actions"][0] - 100] += 1  # (a node that is no init state's successor is a KeyError)
    p = 1 / len(roots)
    sd = math.sqrt(n * p * (1 - p))
    for r, c in counts.items():
        assert c > 0 and abs(c - n * p) <= 6 * sd, (r, c, n * p, sd)


def test_spread_walks_start_at_every_init_state_and_its_duplicates():
    # W = 4, 10 init states and 2 duplicates (48 words of init states): a walk of depth 1 ends at its
    # root plus one bit, and the duplicated roots 0 and 1 are drawn twice as often
    params = [4, 78, 12, 0, 0, 10, 2]
    n = 12000
    started = dict.fromkeys(range(10), 0)
    for i in range(n):
        w = walk(N.SR_MODEL_SPREAD, params, i, 12, nprops=2)
        bits = sum(1 << a for a in w["actions"])
        assert bin(bits).count("1") == w["steps"] and w["end"] in (TERMINAL, DEPTH)
        root = (2 ** 12 - 1) & ~bits if w["end"] == TERMINAL else None
        if root is not None:
            started[root] += 1
    # depth 12 reaches the full set from every root but 0 (12 steps from 0 end at the depth limit)
    assert started[0] == 0 and all(started[r] > 0 for r in range(1, 10))
    sd = math.sqrt(n * (1 / 12) * (11 / 12))
    assert abs(started[1] - n / 6) <= 6 * math.sqrt(n * (1 / 6) * (5 / 6))
    assert all(abs(started[r] - n / 12) <= 6 * sd for r in range(2, 10))


# ---- arguments ---------------------------------------------------------------------------------

def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        walk(N.SR_MODEL_2PC, [3], 0, max_depth=2**20 + 1)
    with pytest.raises(ValueError):
        walk(N.SR_MODEL_2PC, [99], 0)
    with pytest.raises(ValueError):
        walk(N.SR_MODEL_2PC, [3], 2**40)
