#!/usr/bin/env python3
"""Regenerates tests/golden/abd_counts.json: the CPU oracle's `spawn_bfs` counts of the ABD
linearizable register (examples/linearizable-register.rs:192-279) for (client_count, server_count)
pairs past the reference's own golden (2, 2), from the multi-threaded restatement in
oracle/liboracle.so (counts are order-independent: "linearizable" holds, so ABD explores its whole
state space). Fixture only: data, no reference source.

    python tests/golden/make_abd_counts.py     # rewrites the JSON next to this script (~1 minute)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle_lib import OracleRun  # noqa: E402

ABD = 11  # SR_MODEL_ABD
CASES = [(1, 4), (3, 2), (4, 2)]


def run(c, s):
    o = OracleRun(ABD, [c, s], threads=min(16, os.cpu_count() or 1))
    assert o.is_done
    return {"client_count": c, "server_count": s, "unique_state_count": o.unique_state_count,
            "state_count": o.state_count, "max_depth": o.max_depth, "discoveries": o.discovery_names(),
            "pinning": "oracle-derived (CPU restatement only; the reference's golden is (2, 2): 544 states)"}


def main():
    rows = [run(c, s) for c, s in CASES]
    with open(os.path.join(HERE, "abd_counts.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_abd_counts.py (oracle/liboracle.so, CPU restatement)", "cases": rows},
                  f, indent=1)
        f.write("\n")
    print(rows)


if __name__ == "__main__":
    main()
