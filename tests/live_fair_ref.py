"""An independent pure-Python restatement of the complete `eventually` check with its progress-fairness
switch: the fixpoint as a backward worklist over predecessor lists (tests/
live_ref.py runs Jacobi rounds over the successors; with `skip_self` off the two must agree on every
graph used, which the tests assert), the deterministic witness, and two-phase commit with the two
`eventually` properties of TwoPhaseLiveSys. Nothing here calls the engine.

A graph is `succ`: dict state -> list of (action id, next state) in slot order, closed under
successors; `inits` lists the init states in order; `cond(s)` is the property's condition at s.
skip_self: a successor equal to its state is no successor (succ'), and a state whose successors all
are the state itself is a sink (a stutter end), as a state without successors is (terminal).
"""
END_NONE, END_TERMINAL, END_LOOP, END_STUTTER = 0, 1, 2, 3


def moves(succ, s, skip_self):
    return [(a, t) for a, t in succ[s] if not (skip_self and t == s)]


def fixpoint(succ, cond, skip_self=False):
    """(N_p, F_p): F_p the greatest subset of N_p in which every state is a sink or has a successor
    (other than itself with skip_self) in F_p. A state leaves when the count of its successor SLOTS
    that lead into the set drops to zero; removals propagate to predecessors."""
    n = {s for s in succ if not cond(s)}
    live, preds = {}, {}
    for s in n:
        out = moves(succ, s, skip_self)
        live[s] = None if not out else sum(1 for _, t in out if t in n)  # None: a sink, never removed
        for _, t in out:
            preds.setdefault(t, []).append(s)
    f = set(n)
    todo = [s for s in n if live[s] == 0]
    while todo:
        s = todo.pop()
        if s not in f:
            continue
        f.discard(s)
        for q in preds.get(s, ()):
            if q in f and live[q] is not None:
                live[q] -= 1
                if live[q] == 0:
                    todo.append(q)
    return n, f


def witness(succ, inits, f, skip_self=False):
    """None if no init state is in F, else dict(init_index, states, actions, loop_start, end_kind)."""
    start = [i for i, s in enumerate(inits) if s in f]
    if not start:
        return None
    s = inits[start[0]]
    states, actions, seen = [s], [], {s: 0}
    while True:
        out = moves(succ, s, skip_self)
        if not out:
            kind = END_STUTTER if succ[s] else END_TERMINAL
            return {"init_index": start[0], "states": states, "actions": actions, "loop_start": -1, "end_kind": kind}
        a, s = [(a, t) for a, t in out if t in f][0]
        actions.append(a)
        states.append(s)
        if s in seen:
            return {"init_index": start[0], "states": states, "actions": actions, "loop_start": seen[s], "end_kind": END_LOOP}
        seen[s] = len(states) - 1


def check(succ, inits, cond, skip_self=False):
    """dict(unique, not_p_states, surviving, witness) of one graph."""
    n, f = fixpoint(succ, cond, skip_self)
    return {"unique": len(succ), "not_p_states": len(n), "surviving": len(f), "witness": witness(succ, inits, f, skip_self)}


def outcome(want):
    w = want["witness"]
    return "none" if w is None else {END_TERMINAL: "terminal", END_LOOP: "lasso", END_STUTTER: "stutter"}[w["end_kind"]]


def sinks(succ):
    """(terminal states, stutter ends) of a graph."""
    return ([s for s in succ if not succ[s]], [s for s in succ if succ[s] and all(t == s for _, t in succ[s])])


# ---- two-phase commit (examples/2pc.rs), restated -------------------------------------------------------
WORKING, PREPARED, COMMITTED, ABORTED = 0, 1, 2, 3
TM_INIT, TM_COMMITTED, TM_ABORTED = 0, 1, 2


def two_phase(n):
    """(succ, inits) of 2pc with n resource managers. A state is (rm_state tuple, tm_state, tm_prepared
    tuple, msgs frozenset of ("P", rm) / "C" / "A"); the action id is the slot in `actions()` order: 0
    TmCommit, 1 TmAbort, then per rm 2 + 5 rm + (0 TmRcvPrepared, 1 RmPrepare, 2 RmChooseToAbort,
    3 RmRcvCommitMsg, 4 RmRcvAbortMsg). Every enabled action yields a state, its own state included."""
    def actions(s):
        rm_state, tm, prepared, msgs = s
        out = []
        if tm == TM_INIT and all(prepared):
            out.append((0, (rm_state, TM_COMMITTED, prepared, msgs | {"C"})))
        if tm == TM_INIT:
            out.append((1, (rm_state, TM_ABORTED, prepared, msgs | {"A"})))
        for rm in range(n):
            def with_rm(v):
                return rm_state[:rm] + (v,) + rm_state[rm + 1:]
            if tm == TM_INIT and ("P", rm) in msgs:
                out.append((2 + 5 * rm, (rm_state, tm, prepared[:rm] + (True,) + prepared[rm + 1:], msgs)))
            if rm_state[rm] == WORKING:
                out.append((3 + 5 * rm, (with_rm(PREPARED), tm, prepared, msgs | {("P", rm)})))
                out.append((4 + 5 * rm, (with_rm(ABORTED), tm, prepared, msgs)))
            if "C" in msgs:
                out.append((5 + 5 * rm, (with_rm(COMMITTED), tm, prepared, msgs)))
            if "A" in msgs:
                out.append((6 + 5 * rm, (with_rm(ABORTED), tm, prepared, msgs)))
        return out

    init = ((WORKING,) * n, TM_INIT, (False,) * n, frozenset())
    succ, todo = {}, [init]
    while todo:
        s = todo.pop()
        if s in succ:
            continue
        succ[s] = actions(s)
        todo.extend(t for _, t in succ[s])
    return succ, [init]


def every_rm_decides(s):
    return all(r in (COMMITTED, ABORTED) for r in s[0])


def every_rm_commits(s):
    return all(r == COMMITTED for r in s[0])


TWO_PHASE_LIVE_PROPS = {3: ("every RM decides", every_rm_decides), 4: ("every RM commits", every_rm_commits)}
