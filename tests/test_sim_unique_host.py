"""The distinct-state count of the simulation checker on the host (sr_sim_unique_host, csrc/sim.hpp
"Distinct-state count"): the set the device collects in its table, checked here without a device
against an independent restatement (the walks' action ids replayed on the CPU oracle, the path
states' fingerprints through sr_model_fingerprint), and the C ABI's growth for the mode."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from oracle_lib import dgraph_params
from stateright_amd import TwoPhaseSys
from stateright_amd import _native as N
from stateright_amd.plugin import model_fingerprint

SEED = 7
WALKS, DEPTH = 200, 40
EVENTUALLY = N.SR_EVENTUALLY
# seven nodes, one init state (every path starts at 0): a tail 0 -> 2 into the cycle 2 4 6, a longer
# way round it through 8 10, and an exit 6 -> 12
CYCLE = [[0, 2, 4, 6, 2], [0, 2, 4, 8, 10, 2], [0, 2, 4, 6, 12]]
MASK64 = (1 << 64) - 1


def fmix64(k):
    """murmur3's finalizer (csrc/models.hpp fmix64)."""
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & MASK64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & MASK64
    return k ^ k >> 33


def dgraph_fp(node):
    """A DGraph state is its node in one word, and fingerprint<1>(s) = fmix64(s ^ 2^63) (csrc/models.hpp)."""
    return fmix64(node ^ 1 << 63)


def unique_host(model, params, w0, n, loops=False, depth=DEPTH):
    return N.sim_unique_host(model, params, SEED, w0, n, depth, loops)


def walks_of(model, params, loops, depth=DEPTH, walks=WALKS):
    return [N.sim_walk(model, params, SEED, i, depth, 8, loops=loops) for i in range(walks)]


# ---- 1. the host form against an independent restatement ---------------------------------------

@pytest.mark.parametrize("loops", [False, True])
def test_2pc3_set_is_the_fingerprints_of_the_replayed_paths(loops):
    m = TwoPhaseSys(3)
    want, visited = set(), 0
    for w in walks_of(N.SR_MODEL_2PC, [3], loops):
        flat, _ = oracle_lib.replay(N.SR_MODEL_2PC, [3], w["actions"])
        width = len(flat) // (w["steps"] + 1)
        states = [flat[k:k + width] for k in range(0, len(flat), width)]
        assert len(states) == w["steps"] + 1
        fps = [model_fingerprint(m, s) for s in states]
        assert fps[-1] == w["final_fp"]  # (the restatement meets the engine at the walk's own record)
        want.update(fps)
        visited += len(states)
    got = unique_host(N.SR_MODEL_2PC, [3], 0, WALKS, loops)
    assert got.dtype == np.uint64 and got.tolist() == sorted(want)
    assert 1 < len(want) <= 288 and len(want) < visited  # 2pc N=3 has 288 states; the walks repeat many


@pytest.mark.parametrize("loops", [False, True])
def test_dgraph_with_a_cycle_set_is_the_nodes_on_the_walks(loops):
    params = dgraph_params(EVENTUALLY, CYCLE)
    nodes, ends = set(), set()
    for w in walks_of(N.SR_MODEL_DGRAPH, params, loops):
        path = [0] + w["actions"]  # one init state, and a DGraph action is its destination
        assert dgraph_fp(path[-1]) == w["final_fp"]
        nodes.update(path)
        ends.add(w["end"])
    got = unique_host(N.SR_MODEL_DGRAPH, params, 0, WALKS, loops)
    assert got.tolist() == sorted(dgraph_fp(v) for v in nodes)
    assert nodes == {0, 2, 4, 6, 8, 10, 12}
    assert (N.SIM_LOOP in ends) == loops and N.SIM_TERMINAL in ends


# ---- 2. the set is a union over the walks -------------------------------------------------------

@pytest.mark.parametrize("model,params", [(N.SR_MODEL_2PC, [3]), (N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, CYCLE)),
                                          (N.SR_MODEL_PAXOS, [1])], ids=["2pc3", "dgraph", "paxos1"])
def test_halves_unite_to_the_whole_and_loops_give_a_subset(model, params):
    sets = {}
    for loops in (False, True):
        whole = unique_host(model, params, 0, 200, loops)
        a, b = unique_host(model, params, 0, 100, loops), unique_host(model, params, 100, 100, loops)
        assert np.array_equal(whole, np.union1d(a, b))
        assert np.array_equal(whole, np.unique(whole))  # sorted, distinct
        assert len(unique_host(model, params, 0, 0, loops)) == 0
        sets[loops] = set(whole.tolist())
    assert sets[True] <= sets[False]  # the loop-mode walk is the plain walk cut short


def test_depth_one_holds_the_init_state_and_one_successor_each():
    got = unique_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, CYCLE), 0, 50, depth=1)
    assert got.tolist() == sorted([dgraph_fp(0), dgraph_fp(2)])


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="max_depth"):
        unique_host(N.SR_MODEL_2PC, [3], 0, 1, depth=2**20 + 1)
    with pytest.raises(ValueError, match="2\\^40"):
        unique_host(N.SR_MODEL_2PC, [3], 2**40 - 1, 2)
    with pytest.raises(ValueError):
        unique_host(N.SR_MODEL_2PC, [99], 0, 1)


# ---- 3. the C ABI -------------------------------------------------------------------------------

def spawn_error(so):
    arr = (ctypes.c_int64 * 1)(3)
    assert not N.load().sr_gpu_sim_spawn(N.SR_MODEL_2PC, arr, 1, ctypes.byref(so))
    return N.last_error()


def test_opts_grew_behind_the_old_tail_padding():
    assert ctypes.sizeof(N.sr_sim_opts) == 72
    assert (N.sr_sim_opts.loops.offset, N.sr_sim_opts.reserved0.offset, N.sr_sim_opts.unique.offset,
            N.sr_sim_opts.stale_batches.offset, N.sr_sim_opts.unique_capacity.offset) == (48, 52, 56, 60, 64)
    so = N.sr_sim_opts()
    N.load().sr_sim_opts_init_sized(ctypes.byref(so), 4096)
    assert (so.struct_size, so.max_depth, so.unique, so.stale_batches, so.unique_capacity) == (72, 4096, 0, 0, 0)
    ctypes.memset(ctypes.byref(so), 0xAB, ctypes.sizeof(so))
    N.load().sr_sim_opts_init_sized(ctypes.byref(so), 56)  # an older caller: only its own bytes are written
    assert (so.struct_size, so.max_depth, so.loops) == (56, 4096, 0)
    assert (so.unique & 0xFF, so.stale_batches & 0xFF) == (0xAB, 0xAB)
    assert ctypes.sizeof(N.sr_sim_unique_result) == 48


def test_a_56_byte_caller_is_read_as_mode_off_whatever_its_padding_holds():
    so = N.sr_sim_opts()
    N.load().sr_sim_opts_init_sized(ctypes.byref(so), 56)
    so.reserved0 = -0x21524111  # garbage where the old struct had tail padding
    # beyond its 56 bytes: were these read, the check would have a bound (stale_batches with unique)
    so.unique, so.stale_batches, so.unique_capacity = 1, 3, 2**40
    assert so.struct_size == 56
    assert "walks or target_state_count must be set" in spawn_error(so)
    so.struct_size = 72  # the same bytes from a caller of today are read: the capacity is refused
    assert "unique_capacity" in spawn_error(so)


def test_stale_batches_needs_the_mode():
    so = N.sr_sim_opts()
    N.load().sr_sim_opts_init_sized(ctypes.byref(so), ctypes.sizeof(so))
    so.walks, so.stale_batches = 100, 2
    assert "stale_batches needs unique" in spawn_error(so)
    so.walks = 0
    assert "stale_batches needs unique" in spawn_error(so)


def test_no_bound_is_refused_with_the_message_of_before():
    so = N.sr_sim_opts()
    N.load().sr_sim_opts_init_sized(ctypes.byref(so), ctypes.sizeof(so))
    assert spawn_error(so) == "simulation: walks or target_state_count must be set (a property may never be discovered)"
    so.unique = 1  # the mode alone is no bound
    assert spawn_error(so) == "simulation: walks or target_state_count must be set (a property may never be discovered)"


def test_python_refusals():
    b = TwoPhaseSys(3).checker()
    with pytest.raises(ValueError, match="until_stale needs count_unique"):
        b.spawn_simulation(1, walks=10, until_stale=2)
    with pytest.raises(ValueError, match="until_stale must be positive"):
        b.spawn_simulation(1, walks=10, count_unique=True, until_stale=0)
    with pytest.raises(ValueError, match="unique_capacity"):
        b.spawn_simulation(1, walks=10, count_unique=True, unique_capacity=0)
    with pytest.raises(ValueError, match="walks or a target_state_count"):
        b.spawn_simulation(1, count_unique=True)
