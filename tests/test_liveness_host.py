"""The complete `eventually` check on the host (sr_liveness_host, csrc/live.hpp): the rule the kernels
run, checked here without a device against an independent Python restatement (tests/live_ref.py) of
the fixture, the fixpoint and the deterministic witness."""
import random

import pytest

import live_ref
from oracle_lib import dgraph_params
from stateright_amd import _native as N
from stateright_amd.models import LiveGraph, PingPong

EVENTUALLY = N.SR_EVENTUALLY
FIXME_CYCLE = [[0, 2, 4, 2]]          # src/checker.rs:400-413: should give [0, 2, 4, 2]
FIXME_JOIN = [[0, 2, 4], [1, 4, 6]]   # ... and [0, 2, 4, 6]
CAN_VALIDATE = [[1], [2, 3], [2, 6, 7], [4, 9, 10]]  # src/checker.rs:358-376


def random_graph(rng):
    """The generator of tests/test_gpu_eventually.py (`_random_graph`)."""
    paths = []
    for _ in range(rng.randint(1, 6)):
        n = rng.randint(1, 7)
        paths.append([rng.randrange(0, 24) for _ in range(n)])
    return paths


def random_live_graphs(count=40, seed=20250101):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n_bits = rng.randint(1, 10)
        out.append((n_bits, rng.randint(1, 4), rng.getrandbits(40), rng.choice([0, 1, 2, 2, 3, 3, 5]),
                    rng.choice([0, 0, 0, 3, 8, 16]), rng.randint(1, min(512, 2 ** n_bits))))
    return out


def assert_matches(got, want, what):
    """got: a dict of sr_live_result (+ actions); want: live_ref.check() of the same graph."""
    assert got["ran"] == 1, what
    assert (got["not_p_states"], got["surviving"]) == (want["not_p_states"], want["surviving"]), what
    w = want["witness"]
    if w is None:
        assert (got["init_index"], got["witness_len"], got["loop_start"], got["actions"]) == (-1, -1, -1, []), what
    else:
        assert (got["init_index"], got["witness_len"], got["loop_start"]) == (w["init_index"], len(w["actions"]), w["loop_start"]), what
        assert got["actions"] == w["actions"], what
    assert got["rounds"] >= 1 and got["examined"] >= got["not_p_states"], what


def dgraph_states(paths, got):
    """The witness' states: a DGraph action id is the node it leads to."""
    return [sorted({p[0] for p in paths})[got["init_index"]]] + got["actions"]


@pytest.mark.parametrize("params", sorted(live_ref.ANCHORS))
def test_anchors(params):
    want = live_ref.check(*live_ref.live_graph(*params))
    unique, n, f, init, steps, loop = live_ref.ANCHORS[params]
    w = want["witness"]
    assert (want["unique"], want["not_p_states"], want["surviving"]) == (unique, n, f)
    assert (w and w["init_index"], w and len(w["actions"]), w and w["loop_start"]) == (init, steps, loop)
    got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, LiveGraph(*params).params())
    assert got["unique"] == unique
    assert_matches(got, want, params)


def test_random_live_graphs():
    kinds = set()
    for params in random_live_graphs():
        want = live_ref.check(*live_ref.live_graph(*params))
        got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, list(params))
        assert got["unique"] == want["unique"], params
        assert_matches(got, want, params)
        w = want["witness"]
        kinds.add("none" if w is None else "terminal" if w["loop_start"] < 0 else "lasso")
    assert kinds == {"none", "terminal", "lasso"}  # the draw covers every outcome


def test_fixme_graphs_give_the_paths_the_reference_asks_for():
    got = N.liveness_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, FIXME_CYCLE))
    assert dgraph_states(FIXME_CYCLE, got) == [0, 2, 4, 2] and got["loop_start"] == 1
    assert_matches(got, live_ref.check(*live_ref.dgraph(FIXME_CYCLE)), FIXME_CYCLE)
    got = N.liveness_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, FIXME_JOIN))
    assert dgraph_states(FIXME_JOIN, got) == [0, 2, 4, 6] and got["loop_start"] == -1
    assert_matches(got, live_ref.check(*live_ref.dgraph(FIXME_JOIN)), FIXME_JOIN)


def test_can_validate_graphs_have_no_discovery():
    for paths in [CAN_VALIDATE] + [[p] for p in CAN_VALIDATE]:
        got = N.liveness_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, paths))
        assert (got["ran"], got["init_index"], got["witness_len"]) == (1, -1, -1), paths
        assert_matches(got, live_ref.check(*live_ref.dgraph(paths)), paths)


def test_random_dgraphs():
    rng = random.Random(1234 + EVENTUALLY)
    found = 0
    for _ in range(60):
        paths = random_graph(rng)
        want = live_ref.check(*live_ref.dgraph(paths))
        got = N.liveness_host(N.SR_MODEL_DGRAPH, dgraph_params(EVENTUALLY, paths))
        assert got["unique"] == want["unique"], paths
        assert_matches(got, want, paths)
        if want["witness"] is not None:
            found += 1
            assert dgraph_states(paths, got) == want["witness"]["states"], paths
    assert 0 < found < 60


PINGPONG_EVENTUALLY = (2, 3, 5)  # csrc/actor.hpp PingPongSysT::expectation


@pytest.mark.parametrize("duplicating", [False, True])
@pytest.mark.parametrize("lossy", [False, True])
@pytest.mark.parametrize("max_nat", [1, 3, 5])
def test_ping_pong_matches_the_fixpoint_over_its_host_graph(max_nat, lossy, duplicating):
    params = PingPong(max_nat, lossy=lossy, duplicating=duplicating).params()
    succ_l, inits, conds = N.host_graph(N.SR_MODEL_PINGPONG, params)
    succ = dict(enumerate(succ_l))
    for p in range(6):
        if p not in PINGPONG_EVENTUALLY:
            with pytest.raises(ValueError, match="not an `eventually` property"):
                N.liveness_host(N.SR_MODEL_PINGPONG, params, prop=p)
            continue
        want = live_ref.check(succ, inits, lambda s: conds[s] >> p & 1)
        got = N.liveness_host(N.SR_MODEL_PINGPONG, params, prop=p)
        assert got["unique"] == len(succ)
        assert_matches(got, want, (params, p))


def test_a_model_past_max_states_is_refused():
    with pytest.raises(ValueError, match="max_states"):
        N.liveness_host(N.SR_MODEL_LIVE_GRAPH, [12, 2, 1, 2, 0, 1], max_states=100)
    with pytest.raises(ValueError, match="no `eventually` property"):
        N.liveness_host(N.SR_MODEL_2PC, [3])


def test_live_graph_describes_and_fingerprints():
    p = [10, 3, 7, 4, 5, 9]
    arr = (N.ctypes.c_int64 * len(p))(*p)
    want = live_ref.check(*live_ref.live_graph(*p))["unique"]
    assert N.load().sr_selftest_describe(N.SR_MODEL_LIVE_GRAPH, arr, len(p), 1 << 20) == want, N.last_error()
    for bad in ([0, 2, 1, 2, 0, 1], [25, 2, 1, 2, 0, 1], [8, 0, 1, 2, 0, 1], [8, 5, 1, 2, 0, 1], [8, 2, 1, 2, 0, 0],
                [8, 2, 1, 2, 0, 513], [2, 2, 1, 2, 0, 5], [8, 2, 1, 2, 0]):
        with pytest.raises(ValueError):
            N.liveness_host(N.SR_MODEL_LIVE_GRAPH, bad)


def test_opts_grew_for_the_option():
    # the old 56-byte struct ended in 4 bytes of padding: `liveness` lies beyond them, so that a caller's
    # struct_size of 56 says that it has none (tests/test_gpu_liveness.py spawns with such a struct)
    assert N.ctypes.sizeof(N.sr_opts) == 72 and N.sr_opts.reserved0.offset == 52 and N.sr_opts.liveness.offset == 56
    o = N.sr_opts()
    o.liveness = 7
    N.load().sr_opts_init_sized(N.ctypes.byref(o), 56)
    assert (o.struct_size, o.reserved0, o.liveness) == (56, 0, 7)  # only the caller's 56 bytes are written


@pytest.mark.parametrize("words", [2, 4])
def test_wide_live_graph_is_the_same_graph(words):
    for params in [(8, 2, 1, 3, 0, 1), (12, 2, 3, 2, 0, 1), (12, 2, 1, 3, 16, 1), (10, 3, 7, 4, 5, 9)]:
        want = live_ref.check(*live_ref.live_graph(*params))
        got = N.liveness_host(N.SR_MODEL_LIVE_GRAPH, LiveGraph(*params, words=words).params())
        assert got["unique"] == want["unique"]
        assert_matches(got, want, (params, words))
    p = [10, 3, 7, 4, 5, 9, words]
    arr = (N.ctypes.c_int64 * len(p))(*p)
    assert N.load().sr_selftest_describe(N.SR_MODEL_LIVE_GRAPH, arr, len(p), 1 << 20) == want["unique"], N.last_error()
    with pytest.raises(ValueError, match="words"):
        N.liveness_host(N.SR_MODEL_LIVE_GRAPH, [8, 2, 1, 3, 0, 1, 3])
