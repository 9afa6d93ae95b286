"""The ABD register past 3 clients / 3 servers, on the host (stateright_amd/csrc/abd_wide.hpp):
the choice of encoding (8, 16 or 32 network slots), the limits, the SR_ABD_SLOTS override, the
network bound the choice rests on, and the oracle's counts fixture. CPU only: the self-test walks
the reachable states on the host (describe -> undescribe -> fingerprint), and a network past its
slots makes `describe` fail, so a positive count also says that no state overflowed."""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stateright_amd import _native as N  # noqa: E402
from oracle_lib import OracleRun  # noqa: E402

ABD = N.SR_MODEL_ABD
SR_ERR_UNSUPPORTED = -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abd_counts.json")


def selftest(params, cap=200000):
    lib = N.load()
    p = (ctypes.c_int64 * len(params))(*params)
    return lib.sr_selftest_describe(ABD, p, len(params), cap)


def net_bound(c, s):
    """abd_wide.hpp abd_net_bound: the largest network of ABD (c clients, s servers)."""
    d = s - (s // 2 + 1)
    return c * max(1, 3 * d + s - 1, 4 * d)


@pytest.fixture(autouse=True)
def no_override(monkeypatch):
    monkeypatch.delenv("SR_ABD_SLOTS", raising=False)


def test_roundtrip_1_4_every_state():
    # the oracle: 12 915 unique states, 40 298 generated, depth 24
    assert selftest([1, 4]) == 12915, N.last_error()


@pytest.mark.parametrize("params", [[4, 2], [6, 2], [2, 3], [3, 3], [2, 4],  # 16 slots
                                    [4, 3], [4, 4]],                          # 32 slots
                         ids=lambda p: "-".join(map(str, p)))
def test_roundtrip_first_states(params):
    assert selftest(params) > 0, N.last_error()


@pytest.mark.parametrize("params,want", [([1, 3], 1449), ([1, 2], 13)], ids=["1-3", "1-2"])
def test_roundtrip_one_client_eight_slots(params, want):
    # A lone client's history describes as its Get's returned value only, -1 both while its Put is
    # in flight and while its Get is: undescribe tells the two apart by the client's op_count
    # (paxos.hpp Tables::hist_index). The counts are the oracle's.
    o = OracleRun(ABD, params)
    assert o.unique_state_count == want
    assert selftest(params) == want, N.last_error()


@pytest.mark.parametrize("params", [[7, 1], [1, 5], [5, 4], [0, 2]], ids=lambda p: "-".join(map(str, p)))
def test_refused_outside_the_limits(params):
    assert selftest(params) == SR_ERR_UNSUPPORTED
    msg = N.last_error()
    for limit in ("client_count in 1..=6", "server_count in 1..=4", "client_count + server_count <= 8"):
        assert limit in msg, msg


def test_eight_slots_overflow_on_2_3(monkeypatch):
    # the finding: B(2, 3) = 10 envelopes do not fit the 8-slot encoding that used to check (2, 3)
    assert net_bound(2, 3) == 10 and net_bound(3, 3) == 15
    monkeypatch.setenv("SR_ABD_SLOTS", "8")
    assert selftest([2, 3]) == SR_ERR_UNSUPPORTED
    assert "a network exceeded its capacity" in N.last_error()


def test_eight_slots_refuse_four_servers(monkeypatch):
    monkeypatch.setenv("SR_ABD_SLOTS", "8")
    assert selftest([1, 4]) == SR_ERR_UNSUPPORTED
    assert "1..=3" in N.last_error()


def test_32_slots_forced_on_1_4(monkeypatch):
    monkeypatch.setenv("SR_ABD_SLOTS", "32")
    assert selftest([1, 4]) == 12915, N.last_error()


@pytest.mark.parametrize("c,s", [(1, 4), (3, 2), (1, 3)])
def test_bound_is_the_oracles_largest_network(c, s):
    o = OracleRun(ABD, [c, s], record_visits=True)
    net = o.visits_array()[:, -16:]  # the description's last 16 columns: envelope codes, -1 padded
    assert int((net >= 0).sum(axis=1).max()) == net_bound(c, s)


def test_counts_fixture():
    with open(GOLDEN) as f:
        rows = {(r["client_count"], r["server_count"]): r for r in json.load(f)["cases"]}
    assert {(1, 4), (3, 2), (4, 2)} <= set(rows)
    for r in rows.values():
        assert r["unique_state_count"] > 0 and r["state_count"] >= r["unique_state_count"] and r["max_depth"] > 0
        assert r["discoveries"] == ["value chosen"]
    o = OracleRun(ABD, [1, 4])
    r = rows[(1, 4)]
    assert (r["unique_state_count"], r["state_count"], r["max_depth"]) == (o.unique_state_count, o.state_count, o.max_depth)
    assert (o.unique_state_count, o.state_count, o.max_depth) == (12915, 40298, 24)
    assert r["discoveries"] == o.discovery_names()
