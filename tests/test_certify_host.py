"""The certificate pass without a device (csrc/certify.hpp, csrc/certify_selftest.hpp, tests/certify_lib.py).

`sr_selftest_certify_gpu(-1)` builds every case of the GPU self-test (arenas by a sequential search, tables by
sequential probing, nine planted errors on three models in both orders), evaluates the definitions on the
host and cross-checks the cases: a clean arena gives zeros and the count identities, every planted error
moves the counter it was planted for. The Python reference of tests/certify_lib.py, which the GPU tests
compare certificates with, is checked here against the CPU oracle's counts and discoveries."""
import ctypes

import pytest

import certify_lib
from oracle_lib import INCREMENT, INCREMENT_LOCK, LINEAR_EQUATION, PAXOS, TWO_PHASE, OracleRun
from stateright_amd import Expectation, Increment, IncrementLock, LinearEquation, Paxos, TwoPhaseSys
from stateright_amd import _native as N
from stateright_amd.models import Spread

ALWAYS, SOMETIMES = Expectation.Always, Expectation.Sometimes


def test_selftest_host_halves():
    assert N.load().sr_selftest_certify_gpu(-1) == 0, N.last_error()


def test_the_structs():
    assert ctypes.sizeof(N.sr_opts) == 72 and N.sr_opts.certify.offset == 64 and N.sr_opts.coverage.offset == 60
    # 16 + 16 counters of 8 bytes, 8, four arrays of 32 x 8, two of 32 x 4, pass_ms
    assert ctypes.sizeof(N.sr_certificate) == 16 + 16 * 8 + 8 + 4 * 256 + 2 * 128 + 8
    assert N.sr_certificate.holds.offset == 152 and N.sr_certificate.first_level.offset == 152 + 1024
    # a caller built against the 64-byte struct: only its bytes are written, and `certify` reads as 0
    o = N.sr_opts()
    o.certify = 7
    N.load().sr_opts_init_sized(ctypes.byref(o), 64)
    assert (o.struct_size, o.coverage, o.certify) == (64, 0, 7)
    N.load().sr_opts_init(ctypes.byref(o))
    assert (o.struct_size, o.certify) == (72, 0)


def test_the_builder_sets_and_clears_the_option():
    b = TwoPhaseSys(3).checker()
    assert b._opts.certify == 0 and b.certify()._opts.certify == 1 and b.certify(False)._opts.certify == 0
    assert b._opts.counters == 0  # the option implies no counting run


# (model, oracle id, params, its properties as the checker lists them)
TWO_PHASE_PROPS = [("abort agreement", SOMETIMES), ("commit agreement", SOMETIMES), ("consistent", ALWAYS)]
CASES = [
    (lambda: TwoPhaseSys(3), TWO_PHASE, [3], TWO_PHASE_PROPS),
    (lambda: TwoPhaseSys(5), TWO_PHASE, [5], TWO_PHASE_PROPS),
    (lambda: IncrementLock(4), INCREMENT_LOCK, [4], [("fin", ALWAYS), ("mutex", ALWAYS)]),
    (lambda: Increment(3), INCREMENT, [3], [("fin", ALWAYS)]),
    (lambda: LinearEquation(2, 4, 7), LINEAR_EQUATION, [2, 4, 7], [("solvable", SOMETIMES)]),
    (lambda: Paxos(1, 3), PAXOS, [1], [("linearizable", ALWAYS), ("value chosen", SOMETIMES)]),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}-{c[2]}")
def test_reference_matches_the_oracle(case):
    make, oracle_id, params, props = case
    ref = certify_lib.reference(make(), props)
    o = OracleRun(oracle_id, params)
    names = o.discovery_names()
    if len(names) < len(props):  # the oracle explored everything: its three integers are the reference's
        assert (ref["unique"], ref["state_count"], ref["max_depth"]) == (o.unique_state_count, o.state_count, o.max_depth)
        assert ref["states"] == ref["unique"] and sum(ref["levels"]) == ref["states"] and ref["repeated_edges"] == 0
    for p, (name, _) in enumerate(props):
        if len(names) < len(props):
            assert (ref["holds"][p] > 0) == (name in names), name
        if name in names:  # a discovery is a shortest path: its length is the first discovering level
            assert ref["holds"][p] > 0 and ref["first_level"][p] == len(o.discovery_actions(name)), name


def test_reference_counts_repeated_init_states_apart():
    # Spread with roots 0 .. 2 and root 0, 1 again: the search pops and expands the repeats a second time
    f, loops = 8, 1
    props = [("in range", ALWAYS), ("marked", SOMETIMES)]
    plain = certify_lib.reference(Spread(1, 24, f, loops, 0b1011, 3, 0), props)
    ref = certify_lib.reference(Spread(1, 24, f, loops, 0b1011, 3, 2), props)
    assert (ref["inits"], ref["repeated_inits"], ref["states"], ref["unique"]) == (5, 2, 2 ** f + 2, 2 ** f)
    assert ref["edges"] == plain["edges"] and ref["repeated_edges"] == 2 * (f + loops) - 1
    assert ref["state_count"] == plain["state_count"] + 2 + ref["repeated_edges"]
    assert ref["holds"] == plain["holds"] == {0: 0, 1: 1} and ref["first_level"][1] == 2  # 0b1011 from root 1 or 2


class _Fake:
    """What assert_certified reads of a checker, from a reference."""

    def __init__(self, ref, props, found):
        self.ref, self.props, self.found = ref, props, found

    def properties(self):
        return self.props

    def discoveries(self):
        return self.found

    def unique_state_count(self):
        return self.ref["unique"]

    def state_count(self):
        return self.ref["state_count"]

    def max_depth(self):
        return self.ref["max_depth"]


def test_assert_certified_accepts_a_clean_certificate_and_refuses_every_error():
    props = TWO_PHASE_PROPS
    ref = certify_lib.reference(TwoPhaseSys(3), props)
    found = {name: [0] * ref["first_level"][p] for p, (name, _) in enumerate(props) if ref["holds"][p]}
    fake = _Fake(ref, props, found)
    clean = {e: 0 for e in certify_lib.ERRORS}
    clean.update(ran=1, skipped=0, fifo=1, explored_all=1, states=ref["states"], levels=len(ref["levels"]), inits=ref["inits"],
                 repeated_inits=0, edges=ref["edges"], repeated_edges=0, pmask=7, nprops=3,
                 holds=[ref["holds"][p] for p in range(3)], first_index=[ref["first_index"][p] for p in range(3)],
                 disc_index=[ref["first_index"][p] for p in range(3)], disc_wrong=[0, 0, 0],
                 first_level=[ref["first_level"][p] if ref["holds"][p] else 2 ** 32 - 1 for p in range(3)],
                 disc_level=[ref["first_level"][p] if ref["holds"][p] else 2 ** 32 - 1 for p in range(3)])
    certify_lib.assert_certified(fake, cert=dict(clean))
    certify_lib.assert_matches_reference(clean, ref)
    for e in certify_lib.ERRORS:
        with pytest.raises(AssertionError):
            certify_lib.assert_certified(fake, cert=dict(clean, **{e: 1}))
    for change in ({"states": ref["states"] - 1}, {"edges": ref["edges"] + 1}, {"levels": len(ref["levels"]) + 1}, {"ran": 0},
                   {"disc_wrong": [1, 0, 0]}, {"disc_index": [clean["disc_index"][0] + 1] + clean["disc_index"][1:]},
                   {"disc_level": [clean["disc_level"][0] + 1] + clean["disc_level"][1:]}, {"holds": [0] + clean["holds"][1:]}):
        with pytest.raises(AssertionError):
            certify_lib.assert_certified(fake, cert=dict(clean, **change))
