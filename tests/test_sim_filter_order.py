"""scripts/sim_filter_order.py, the CPU simulation of expand_fast's duplicate filter under the two
append orders of the new states: its BFS must be the oracle's (unique and generated states), and
the order grouped per wave must send fewer successors past the filter than the interleaved one."""
import os
import sys

import pytest

from oracle_lib import TWO_PHASE, OracleRun

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import sim_filter_order as sim  # noqa: E402


@pytest.mark.parametrize("order", sim.ORDERS)
@pytest.mark.parametrize("n", [3, 5])
def test_counts_equal_the_oracle(n, order):
    o = OracleRun(TWO_PHASE, [n])
    r = sim.simulate(n, order)
    assert (r["unique"], r["generated"]) == (o.unique_state_count, o.state_count)
    if n == 3:
        assert r["unique"] == 288
    assert sum(lv["new"] for lv in r["levels"]) + 1 == r["unique"]
    assert r["unique"] - 1 <= r["first_probes"] <= r["entering"] < r["generated"]


def test_grouped_order_probes_less():
    a, b = sim.simulate(6, "interleaved"), sim.simulate(6, "grouped")
    assert (a["unique"], a["generated"], a["entering"]) == (b["unique"], b["generated"], b["entering"])
    assert [lv["parents"] for lv in a["levels"]] == [lv["parents"] for lv in b["levels"]]
    assert b["first_probes"] < a["first_probes"]
