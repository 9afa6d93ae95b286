"""The clean-audit assertion shared by the growth tests: a check run with counters() audits its final
visited set against its arena (csrc/kernels_audit.hpp, checker.table_audit()). All expectations
are exact."""

ERROR_FIELDS = ("misplaced", "duplicates", "arena_missing", "arena_shared", "meta_wrong")


def assert_clean_audit(c, complete=True, fifo=None):
    """Every error field is 0; a check that explored everything has exactly its unique states in the
    table and in the arena (`occupied == unique` is what catches stale entries of a recycled table
    that happen not to collide). complete=False (an early exit or a target stop: a level past the
    end may have claimed slots): the table holds at least the arena's states."""
    a = c.table_audit()
    assert a["ran"] == 1, a
    assert {k: a[k] for k in ERROR_FIELDS} == dict.fromkeys(ERROR_FIELDS, 0), a
    if complete:
        assert a["occupied"] == a["arena_states"] == c.unique_state_count(), (a, c.unique_state_count())
    else:
        assert a["occupied"] >= a["arena_states"] > 0, a
    if fifo is not None:
        assert a["fifo"] == (1 if fifo else 0), a
    return a
