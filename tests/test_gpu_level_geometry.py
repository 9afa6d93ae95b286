"""expand_fast's balanced level geometry on the GPU: every level cut into equal workgroup shares from
the real frontier size (SR_BALANCE_MIN=1: small frontiers too), on grids of 3, 5 and 7 workgroups, so
that the chunk counts do not divide and every workgroup strides. Counts, depth and discoveries must
equal the CPU oracle's, with and without level pipelining, in the counting instantiation and with
the geometry switched off; stats.balanced_levels shows which geometry ran."""
import pytest

from oracle_lib import INCREMENT_LOCK, PAXOS, TWO_PHASE, replay
from test_gpu_parity import gpu, ids, oracle

pytestmark = pytest.mark.gpu

# one-word states (2pc N=5: the reference's golden 8 832 states; N=7: 296 448), two-word states
# (increment_lock, no duplicate filter), wide states (paxos, W = 11: 16 668)
CASES = [(TWO_PHASE, [5]), (TWO_PHASE, [7]), (INCREMENT_LOCK, [9]), (PAXOS, [2])]


def check(case, balanced, **kw):
    model, params = case
    o = oracle(model, params)
    c, _ = gpu(model, params, "fast", **kw)
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == \
        (o.unique_state_count, o.state_count, o.max_depth)
    assert sorted(c.discoveries()) == o.discovery_names()
    st = c.stats()
    assert st["balanced_levels"] > 0 if balanced else st["balanced_levels"] == 0
    if case == (TWO_PHASE, [5]):
        props = c.properties()
        for name, path in c.discoveries().items():
            r = replay(model, params, path.action_ids, n_props=len(props))
            assert r is not None, f"{name}: path does not replay on the CPU model"
            assert len(path) == len(o.discovery_actions(name))
    return c


@pytest.mark.parametrize("grid", ["3", "5", "7"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_balanced_shares_on_small_grids(case, grid, monkeypatch):
    monkeypatch.setenv("SR_GRID_MAX", grid)
    monkeypatch.setenv("SR_BALANCE_MIN", "1")
    for pipe in ("1", "0"):
        monkeypatch.setenv("SR_PIPELINE", pipe)
        check(case, True)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_balanced_shares_counting_form(case, monkeypatch):
    # counters=True: the STATS instantiation follows the static form
    monkeypatch.setenv("SR_GRID_MAX", "5")
    monkeypatch.setenv("SR_BALANCE_MIN", "1")
    c = check(case, True, counters=True)
    assert c.stats()["probes"] > 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_switch_off_keeps_the_fixed_geometry(case, monkeypatch):
    monkeypatch.setenv("SR_GRID_MAX", "5")
    monkeypatch.setenv("SR_BALANCE_MIN", "1")
    monkeypatch.setenv("SR_BALANCE", "0")
    for pipe in ("1", "0"):
        monkeypatch.setenv("SR_PIPELINE", pipe)
        check(case, False)


def test_default_threshold_balances_only_large_levels():
    # defaults: 2pc N=7's levels reach 64 K parents (balanced), 2pc N=5's never do on the pipelined path
    big = check((TWO_PHASE, [7]), True)
    assert big.stats()["balanced_levels"] < big.stats()["expand_launches"]
