"""Loop detection of the simulation checker on the host (sr_sim_walk_loops, csrc/sim.hpp "Loop
detection"): the same code the kernel runs, checked here without a device against the rule's closed
forms on deterministic lassos and against an independent restatement over state equality."""
import pytest

import oracle_lib
from oracle_lib import dgraph_params
from stateright_amd import _native as N

SEED = 20240607
TERMINAL, DEPTH, LOOP = N.SIM_TERMINAL, N.SIM_DEPTH, N.SIM_LOOP
EVENTUALLY, SOMETIMES = N.SR_EVENTUALLY, N.SR_SOMETIMES
FIXME = [[0, 2, 4, 2]]  # src/checker.rs:400-413


def walk(model, params, i, max_depth=64, loops=True, nprops=1):
    return N.sim_walk(model, params, SEED, i, max_depth, nprops, loops=loops)


def lasso(mu, cycle):
    """One path: a prefix of mu even nodes (200, 202, ...), then the ring 0, 2, .., 2 (cycle - 1), 0."""
    return [[200 + 2 * k for k in range(mu)] + [2 * k for k in range(cycle)] + [0]]


# ---- 1. the reference's FIXME ------------------------------------------------------------------

def test_fixme_lasso_is_a_hit_with_loops_on():
    params = dgraph_params(EVENTUALLY, FIXME)
    for i in range(50):
        w = walk(N.SR_MODEL_DGRAPH, params, i)
        assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (3, LOOP, 1, [3])
        assert w["actions"] == [2, 4, 2]
        off = walk(N.SR_MODEL_DGRAPH, params, i, loops=False)
        assert (off["steps"], off["end"], off["first_hit"]) == (64, DEPTH, [-1])
        assert "loop_start" not in off
        assert off == N.sim_walk(N.SR_MODEL_DGRAPH, params, SEED, i, 64, 1)  # the default is off


# ---- 2. deterministic lassos: the rule's closed forms -------------------------------------------

# cycle length -> (t, j) for a prefix of 0 states; beyond the window j is the checkpoint's power of two
BEYOND = {9: (25, 16), 12: (28, 16), 13: (29, 16), 20: (52, 32), 33: (97, 64)}


@pytest.mark.parametrize("cycle", sorted(BEYOND))
def test_rings_beyond_the_window_end_at_a_checkpoint(cycle):
    t, j = BEYOND[cycle]
    for mu in (0, 1, 3, 5):  # (the powers of two involved are all >= 16 > mu)
        params = dgraph_params(EVENTUALLY, lasso(mu, cycle))
        w = walk(N.SR_MODEL_DGRAPH, params, 0, max_depth=128)
        assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (t, LOOP, j, [t]), (cycle, mu)


@pytest.mark.parametrize("cycle", [1, 2, 3, 7, 8])
def test_rings_within_the_window_end_at_their_first_closure(cycle):
    for mu in (0, 1, 3, 5):
        params = dgraph_params(EVENTUALLY, lasso(mu, cycle))
        w = walk(N.SR_MODEL_DGRAPH, params, 0, max_depth=128)
        assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (mu + cycle, LOOP, mu, [mu + cycle]), (cycle, mu)


def test_the_loop_test_precedes_the_depth_test():
    params = dgraph_params(EVENTUALLY, lasso(0, 12))
    w = walk(N.SR_MODEL_DGRAPH, params, 0, max_depth=27)
    assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (27, DEPTH, -1, [-1])
    w = walk(N.SR_MODEL_DGRAPH, params, 0, max_depth=28)
    assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (28, LOOP, 16, [28])


# ---- 3. a cycle on which the property held ------------------------------------------------------

def test_a_cycle_on_which_the_property_held_is_no_hit():
    params = dgraph_params(EVENTUALLY, [[0, 1, 2, 1]])
    for i in range(20):
        w = walk(N.SR_MODEL_DGRAPH, params, i)
        assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (3, LOOP, 1, [-1])


def test_other_expectations_end_at_the_loop_without_a_hit_of_it():
    params = dgraph_params(SOMETIMES, [[0, 2, 4, 2]])
    w = walk(N.SR_MODEL_DGRAPH, params, 0)
    assert (w["steps"], w["end"], w["loop_start"], w["first_hit"]) == (3, LOOP, 1, [-1])


# ---- 4. hit order -------------------------------------------------------------------------------

def test_a_shorter_terminal_trace_is_ahead_of_the_lasso():
    params = dgraph_params(EVENTUALLY, [[0, 2, 4, 2], [2, 6]])
    best, kinds = None, set()
    for i in range(200):
        w = walk(N.SR_MODEL_DGRAPH, params, i)
        t = w["first_hit"][0]
        assert t == w["steps"] and w["end"] in (TERMINAL, LOOP)  # every node is even: each walk ends in a hit
        nodes = [0 if w["actions"][0] == 2 else 2] + w["actions"]
        kinds.add((tuple(nodes), w["end"], w["loop_start"]))
        if best is None or (t, i) < best[:2]:
            best = (t, i, nodes, w["end"])
    # init states 0 and 2; from 2: 4 or 6; from 4: 2
    assert kinds == {((0, 2, 6), TERMINAL, -1), ((0, 2, 4, 2), LOOP, 1), ((2, 6), TERMINAL, -1), ((2, 4, 2), LOOP, 0)}
    assert best[0] == 1 and best[2] == [2, 6]
    # among the walks from init state 0 the terminal [0, 2, 6] (t = 2) is ahead of the lasso (t = 3)
    from0 = sorted((len(k[0]) - 1, k[0]) for k in kinds if k[0][0] == 0)
    assert from0[0] == (2, (0, 2, 6))


# ---- 5. an independent restatement over state equality -----------------------------------------

def first_detection(states, window=8):
    """The window and checkpoint rule over the states themselves: (t, j) of the first detection on
    the path `states`, or None."""
    checkpoint = (states[0], 0)
    for t in range(1, len(states)):
        recent = [i for i in range(max(0, t - window), t) if states[i] == states[t]]
        if recent:
            return t, max(recent)
        if checkpoint[0] == states[t]:
            return t, checkpoint[1]
        if t & (t - 1) == 0:
            checkpoint = (states[t], t)
    return None


def dgraph_states(init_of_first_action):
    return lambda model, params, w: [init_of_first_action(w["actions"])] + w["actions"]


def clock_states(model, params, w):  # GoHigh = 1 leads to 1, GoLow = 0 to 0
    return [1 - w["actions"][0]] + w["actions"]


def oracle_states(model, params, w):
    flat, _ = oracle_lib.replay(model, params, w["actions"])
    width = len(flat) // (w["steps"] + 1)
    return [tuple(flat[k:k + width]) for k in range(0, len(flat), width)]


# two cycles through node 0: 0 2 4 (inside the window) and 0 10 12 .. 30 (11 nodes: beyond it)
SHARED = [[0, 2, 4, 0], [0] + list(range(10, 32, 2)) + [0]]
RESTATED = {
    "fixme": (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, FIXME), 48, dgraph_states(lambda a: 0)),
    "ring12": (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, lasso(3, 12)), 48, dgraph_states(lambda a: 200)),
    "two_inits": (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, [[0, 2, 4, 2], [2, 6]]), 48,
                  dgraph_states(lambda a: 0 if a[0] == 2 else 2)),
    "shared": (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, SHARED), 48, dgraph_states(lambda a: 0)),
    "binary_clock": (N.SR_MODEL_BINARY_CLOCK, [], 48, clock_states),
    "2pc3": (N.SR_MODEL_2PC, [3], 48, oracle_states),
}


@pytest.mark.parametrize("name", sorted(RESTATED))
def test_loop_walk_is_the_plain_walk_cut_at_the_restatements_first_detection(name):
    model, params, depth, states_of = RESTATED[name]
    gaps = []
    for i in range(200):
        plain = walk(model, params, i, depth, loops=False, nprops=8)
        got = walk(model, params, i, depth, loops=True, nprops=8)
        states = states_of(model, params, plain)
        assert len(states) == plain["steps"] + 1
        d = first_detection(states)
        if d is None:
            want = (plain["steps"], plain["end"], -1)
            t = plain["steps"]
        else:
            t, j = d
            want = (t, LOOP, j)
            gaps.append(t - j)
        assert (got["steps"], got["end"], got["loop_start"]) == want, i
        assert got["actions"] == plain["actions"][:t]
        if model == N.SR_MODEL_DGRAPH:  # eventually "odd": a hit where the walk ends, unless it ends at the depth
            ended = d is not None or plain["end"] == TERMINAL
            assert got["first_hit"][0] == (t if ended and not any(s % 2 for s in states[:t + 1]) else -1), i
        else:  # always / sometimes: the plain walk's hits up to the cut
            assert got["first_hit"] == [h if h <= t else -1 for h in plain["first_hit"]], i
    if name == "shared":  # the sample holds both kinds of detection
        assert any(g <= 8 for g in gaps) and any(g > 8 for g in gaps)
        assert len(gaps) == 200  # every walk of depth 48 closes a loop here
    if name in ("binary_clock", "fixme", "ring12"):
        assert len(gaps) == 200
    if name == "2pc3":
        assert gaps and set(gaps) <= set(range(1, 9))


# ---- arguments ---------------------------------------------------------------------------------

def test_bad_arguments_are_refused_in_loop_mode_too():
    with pytest.raises(ValueError):
        walk(N.SR_MODEL_2PC, [3], 0, max_depth=2**20 + 1)
    with pytest.raises(ValueError):
        walk(N.SR_MODEL_2PC, [3], 2**40)
