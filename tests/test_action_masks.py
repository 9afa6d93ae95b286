"""2pc's optional FAST-expansion hooks against its own `enabled`, `self_loops` and `apply`, on the
host (no GPU): sr_selftest_action_masks walks every reachable state for N <= 4 and draws 10 000
random states for each N = 1..14 of the runtime-n form and the compiled-in 9, 10 and 11."""
from stateright_amd import _native


def test_action_masks_selftest():
    # for every enabled slot (s & ~clr) | set == apply(s, slot); enabled_moves == enabled & ~self_loops
    # and returns the self-loops' popcount; every slot it leaves changes the state (SELF_LOOPS_EXACT).
    # The action table is held one slot per lane (no packed descriptor to decode); the Ladder
    # fixture's hooks, whose slots pass 64, are checked the same way.
    lib = _native.load()
    assert lib.sr_selftest_action_masks() == 0, _native.last_error()
