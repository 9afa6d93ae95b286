"""The forms of the partitioned kernels (and one path of expand_fast) that no default run selects,
each forced by the host's switches and compared with the CPU oracle like tests/test_gpu_partitioned.py:

  queue     expand_route<M, -4>: the per-lane probe queues (SR_ROUTE_QUEUE=1; only without a sent cache)
  ordered   expand_route's owner-ordered record flush (SR_ORDERED_FLUSH=1)
  tiny      stages too small for a chunk: the per-wave overflow reservations of the local append and
            of the record staging, in the round form and in the queue form
  big       insert_recv_lag<M, -4> and <M, 4>: four records per thread on the large insert grid

Every case sets SR_HEAD_MAX=0, so that each level is partitioned (the replicated head would explore
these small models alone). Which kernels the module runs was read once from a kernel trace of it
(rocprofv3 --kernel-trace --stats): expand_route<TwoPhaseT<0>, -4, false> and
expand_route<IncrementLock<1>, -4, false> beside the <.., 1, false> forms, and
insert_recv_lag<TwoPhaseT<0>, -4> and <TwoPhaseT<0>, 4> beside <.., 1>.

increment_lock N=5 packs its state into one word (IncrementLock<1>, as every N <= 8), so the
two-word case of the ordered flush and of the tiny stages is increment_lock N=9 (IncrementLock<2>:
expand_route<IncrementLock<2>, 1, false>, whose two-word stage holds one state or one record).
Two forms have no two-word case: the host gives two-word quotient tables no queue form, and no
two-word model small enough for a test plans an insert of more than 512 Ki records
(increment_lock N=9 was traced: insert_recv_lag<IncrementLock<2>, 1> only)."""
import pytest

from oracle_lib import INCREMENT_LOCK, TWO_PHASE
from stateright_amd.models import Spread
from test_gpu_partitioned import MODELS, ids, oracle
from test_gpu_spread import closed_form

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")

SMALL = [(TWO_PHASE, [3]), (TWO_PHASE, [5]), (INCREMENT_LOCK, [5])]
TWO_WORDS = (INCREMENT_LOCK, [9])

# Stages of two words: two one-word states or records (one of two words). A chunk of 4 waves x 64
# parents (SR_ROUTE_PPW_LOG2=6) stages hundreds of each, so all but the first two of every flush
# interval take the per-wave overflow reservations. The host takes any size but 0 ("the default");
# two words is the least that still stages a record of either width.
TINY = {"SR_RSTAGE_WORDS": "2", "SR_LSTAGE_WORDS": "2", "SR_ROUTE_PPW_LOG2": "6"}
QUEUE = {"SR_ROUTE_QUEUE": "1", "SR_SEND_CACHE": "0"}
SETTINGS = {
    "queue": QUEUE,
    "ordered": {"SR_ORDERED_FLUSH": "1"},
    "ordered-queue": {"SR_ORDERED_FLUSH": "1", **QUEUE},
    "tiny": TINY,
    "tiny-queue": {**TINY, **QUEUE},
}


def check(case, parts, env, monkeypatch):
    monkeypatch.setenv("SR_HEAD_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, params = case
    o = oracle(model, params)
    c = MODELS[model](params).checker().partitions(parts).spawn_bfs().join()
    assert c.unique_state_count() == o.unique_state_count
    assert c.state_count() == o.state_count
    assert c.max_depth() == o.max_depth
    assert sorted(c.discoveries()) == o.discovery_names()
    return c


# every setting on the one-word models; the two that have a two-word form on the two-word model too
FORCED = [(s, c) for s in sorted(SETTINGS) for c in SMALL + ([TWO_WORDS] if s in ("ordered", "tiny") else [])]


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("setting,case", FORCED, ids=[f"{s}-{ids(c)}" for s, c in FORCED])
def test_forced_forms_match_oracle(setting, case, parts, monkeypatch):
    c = check(case, parts, SETTINGS[setting], monkeypatch)
    st = c.stats()
    assert st["records_routed"] > 0, st
    # The one-word models run every level on the pipelined plan. increment_lock N=9 outgrows that
    # plan's buckets under any setting, the default ones included, and the search restarts with one
    # host synchronisation per level: both level loops launch the same route kernel with the same
    # stages and flags, so the forced form runs in either.
    if case is not TWO_WORDS:
        assert st["pipelined"] == 2 and st["restarts"] == 0, st


# The four-records insert needs an insert grid above 512 workgroups: more than 512 Ki planned
# records over the partitions' buckets (T x the bucket capacity, which the plan derives from the
# frontier, not from a capacity hint), with SR_INSERT_BATCH_MIN=0. 2pc N=8 (1.7 M states) plans so
# many at its widest levels; the N=3 and N=5 runs above cannot. The first case takes 2.6 s on an
# MI355X (the oracle's run of N=8 included, which the other three share), each further one 10 ms.
@pytest.mark.parametrize("machines", ["1", "0"])
@pytest.mark.parametrize("case,parts", [((TWO_PHASE, [8]), 2), ((TWO_PHASE, [8]), 3)], ids=["2pc-8-T2", "2pc-8-T3"])
def test_four_record_inserts_match_oracle(case, parts, machines, monkeypatch):
    check(case, parts, {"SR_INSERT_BATCH_MIN": "0", "SR_INSERT_MACHINES": machines}, monkeypatch)


@pytest.mark.parametrize("batch", ["1", "-4"])
def test_expand_fast_stage_overflow(batch, monkeypatch):
    # expand_fast's direct append: a workgroup that stages more than STAGE = 1024 one-word states
    # between two flushes. The fixed geometry with 64 parents per wave makes a chunk 256 parents
    # (a narrow state's chunk is 256 parents whatever the waves per workgroup, expand_ppw_log2_max),
    # and the stage is flushed only between chunks, so a level of at most 256 parents with more
    # than 1024 new states overflows whatever the grid. Spread's level k is the C(F, k) subsets of
    # k bits, all new: F = 20 is the smallest F with such a level (190 parents, 1140 new states,
    # so at least 116 direct appends; F = 19 has 171 and 969). The counts are Spread's closed form,
    # which tests/test_gpu_spread.py holds against the Python oracle at F = 12.
    F, mark = 20, 0b01011001101001011001
    monkeypatch.setenv("SR_PPW_LOG2", "6")
    monkeypatch.setenv("SR_BALANCE", "0")
    monkeypatch.setenv("SR_PROBE_BATCH", batch)  # the probe rounds, the per-lane probe queues
    c = Spread(1, 45, F, 0, mark).checker().order("fast").capacity_hint(2 ** F).spawn_bfs().join()
    assert (c.unique_state_count(), c.state_count(), c.max_depth()) == closed_form(F, 0)
    assert sorted(c.discoveries()) == ["marked"]
    assert len(c.discovery("marked")) == bin(mark).count("1")
    c.assert_properties()
