"""An independent pure-Python restatement of the complete `eventually` check under weak fairness
(DESIGN.md section 12): the progress fixpoint of tests/live_fair_ref.py, the strongly connected
components of F_p' by Kosaraju's two passes, the fairness of a component, the goal set, BFS ranks over
predecessor lists, the first init state, the stem, and a validity check of a given loop. Nothing here
calls the engine.

A graph is `succ`: dict state -> list of (action id, next state) in slot order, closed under
successors. For every model used here the action id IS the slot (the fairness class): DGraph's
destination node, LiveGraph's edge number, 2pc's action slot, SpinLock's slot. `nslots` is the
model's `max_actions()`.
  me(s, a): slot a is listed at s and leads to a state other than s.
  A component (two or more states, edges between distinct states of F_p') is FAIR iff for every slot
  a: some member has not me(., a), or some member's a-step stays in the component.
"""
import live_fair_ref as LF


def moves(succ, s):
    return [(a, t) for a, t in succ[s] if t != s]


def me_slots(succ, s):
    return {a for a, t in succ[s] if t != s}


def components(succ, f):
    """The strongly connected components of the graph on f (edges between distinct states), those
    with two or more states, as a list of frozensets (Kosaraju, iterative)."""
    out = {s: [t for _, t in moves(succ, s) if t in f] for s in f}
    order, seen = [], set()
    for root in f:
        if root in seen:
            continue
        seen.add(root)
        stack = [(root, iter(out[root]))]
        while stack:
            s, it = stack[-1]
            for t in it:
                if t not in seen:
                    seen.add(t)
                    stack.append((t, iter(out[t])))
                    break
            else:
                order.append(s)
                stack.pop()
    preds = {s: [] for s in f}
    for s in f:
        for t in out[s]:
            preds[t].append(s)
    comps, done = [], set()
    for root in reversed(order):
        if root in done:
            continue
        done.add(root)
        comp, todo = [root], [root]
        while todo:
            s = todo.pop()
            for q in preds[s]:
                if q not in done:
                    done.add(q)
                    comp.append(q)
                    todo.append(q)
        if len(comp) >= 2:
            comps.append(frozenset(comp))
    return comps


def is_fair(succ, comp, nslots):
    for a in range(nslots):
        if any(a not in me_slots(succ, s) for s in comp):
            continue
        if any(x == a and t in comp for s in comp for x, t in moves(succ, s)):
            continue
        return False
    return True


def cyclic(succ, f):
    """F_p' without its sinks, trimmed to the states with a successor (other than itself) in the set."""
    u = {s for s in f if moves(succ, s)}
    while True:
        g = {s for s in u if any(t in u for _, t in moves(succ, s))}
        if g == u:
            return u
        u = g


def ranks(succ, domain, targets):
    """BFS distance to `targets` inside `domain` over edges between distinct states."""
    preds = {}
    for s in domain:
        for _, t in moves(succ, s):
            if t in domain:
                preds.setdefault(t, []).append(s)
    rank = {s: 0 for s in targets}
    level = list(targets)
    while level:
        nxt = []
        for t in level:
            for q in preds.get(t, ()):
                if q not in rank:
                    rank[q] = rank[t] + 1
                    nxt.append(q)
        level = nxt
    return rank


def descend(succ, rank, s):
    """From s along the lowest slot whose result has a lower rank, to rank 0: (actions, states after s)."""
    actions, states = [], []
    while rank[s]:
        a, s = next((a, t) for a, t in moves(succ, s) if t in rank and rank[t] < rank[s])
        actions.append(a)
        states.append(s)
    return actions, states


def check(succ, inits, cond, nslots):
    """Every unique figure of one graph: dict(unique, not_p_states, surviving, cyclic_states, components,
    fair_components, goal_states, fair_states, init_index, stem (actions), stem_states, end_kind of a
    witness that closes no loop (0 otherwise), comp (the fair component the stem ends in, or None))."""
    n, f = LF.fixpoint(succ, cond, skip_self=True)
    comps = components(succ, f)
    fair = [c for c in comps if is_fair(succ, c, nslots)]
    sinks = {s for s in f if not moves(succ, s)}
    goal = set(sinks)
    for c in fair:
        goal |= c
    rank = ranks(succ, f, goal)
    res = {"unique": len(succ), "not_p_states": len(n), "surviving": len(f), "cyclic_states": len(cyclic(succ, f)),
           "components": len(comps), "fair_components": len(fair), "goal_states": len(goal), "fair_states": len(rank),
           "init_index": -1, "stem": None, "stem_states": None, "end_kind": LF.END_NONE, "comp": None}
    start = [i for i, s in enumerate(inits) if s in rank]
    if not start:
        return res
    res["init_index"] = start[0]
    s = inits[start[0]]
    acts, sts = descend(succ, rank, s)
    res["stem"], res["stem_states"] = acts, [s] + sts
    g = res["stem_states"][-1]
    if g in sinks:
        res["end_kind"] = LF.END_STUTTER if succ[g] else LF.END_TERMINAL
    else:
        res["end_kind"] = LF.END_LOOP
        res["comp"] = next(c for c in fair if g in c)
    return res


def loop_problems(succ, cond, nslots, start, actions, inside=None):
    """What is wrong with the closed walk that `actions` take from `start` as a weakly fair loop on
    which the condition never holds ([] if nothing): it is closed, lies inside N_p (and inside the set
    `inside`, if given), has no self step, every step is listed at its state, and every slot is either
    not moving-enabled at some state of the loop or taken by one of its steps."""
    bad, s, states = [], start, [start]
    for a in actions:
        nxt = [t for x, t in succ[s] if x == a]
        if not nxt:
            return bad + [f"action {a} is not listed at {s!r}"]
        if nxt[0] == s:
            bad.append(f"action {a} at {s!r} returns the state itself")
        s = nxt[0]
        states.append(s)
    if not actions:
        bad.append("the loop has no step")
    if s != start:
        bad.append("the walk is not closed")
    bad += [f"the condition holds at {x!r}" for x in states if cond(x)]
    if inside is not None:
        bad += [f"{x!r} is outside the component" for x in states if x not in inside]
    taken = set(actions)
    for a in range(nslots):
        if a not in taken and all(a in me_slots(succ, x) for x in states):
            bad.append(f"slot {a} is moving-enabled at every state of the loop and never taken")
    return bad


# ---- SpinLock(n): a spin lock with a clock (stateright_amd/csrc/models.hpp SpinLock), restated ----------
def spin_lock(n):
    """(succ, inits) of SpinLock(n). A state is (holder, served, tick): holder 0 = free, i + 1 = thread
    i; served a bit set; tick 0 / 1. Slots: i < n Acquire(i) (the lock is free), n + i Release(i)
    (thread i holds it: serves i and frees the lock), 2n Tick (always: flips tick)."""
    def actions(s):
        holder, served, tick = s
        out = []
        if holder == 0:
            out += [(i, (i + 1, served, tick)) for i in range(n)]
        else:
            i = holder - 1
            out.append((n + i, (0, served | 1 << i, tick)))
        out.append((2 * n, (holder, served, tick ^ 1)))
        return sorted(out)

    init = (0, 0, 0)
    succ, todo = {}, [init]
    while todo:
        s = todo.pop()
        if s in succ:
            continue
        succ[s] = actions(s)
        todo.extend(t for _, t in succ[s])
    return succ, [init]


def some_served(s):
    return s[1] != 0


def every_served(n):
    return lambda s: s[1] == (1 << n) - 1


def spin_lock_word(s, n):
    """The model's one-word state of (holder, served, tick): holder in bits [0,5), served in [5,5+n),
    tick in bit 5 + n."""
    return s[0] | s[1] << 5 | s[2] << (5 + n)


# ---- the graphs of the tests and the issue's anchors ----------------------------------------------------
# A case is ("dgraph", paths) | ("live", (n_bits, degree, seed, p_mod, t_mod, roots)) | ("spin", n, prop) |
# ("2pc", n, prop). ANCHORS: case -> (unique, |N_p|, |F_p'|, components, fair components, goal, FairF, first
# init (-1: the property holds), stem steps, end_kind); None where the issue gives no figure.
ANCHORS = {
    ("dgraph", ((0, 2, 4, 2),)): (3, 3, 3, 1, 1, 2, 3, 0, 1, LF.END_LOOP),
    ("dgraph", ((0, 2, 4, 2), (2, 6), (4, 6), (6, 1))): (5, 4, 3, 1, 0, 0, 0, -1, None, LF.END_NONE),
    ("dgraph", ((0, 2, 4, 2), (2, 6), (4, 6))): (4, 4, 4, 1, 0, 1, 4, 0, 2, LF.END_TERMINAL),
    ("dgraph", ((0, 2, 4, 2), (2, 6, 8, 6), (4, 6))): (5, 5, 5, 2, 1, 2, 5, 0, 2, LF.END_LOOP),
    ("live", (8, 2, 20, 2, 0, 1)): (208, 100, 9, 1, 0, 0, 0, -1, None, LF.END_NONE),
    ("live", (8, 3, 26, 2, 0, 1)): (247, 126, 83, 5, 2, 18, 35, -1, None, LF.END_NONE),
    ("live", (12, 2, 26, 2, 0, 1)): (3265, 1621, 568, 6, 5, 77, 565, 0, 9, None),
    ("live", (12, 2, 1, 2, 0, 64)): (3306, 1655, 476, 6, 3, 50, 449, 10, 0, None),
    ("live", (12, 2, 1, 3, 16, 1)): (3146, 2096, 1702, 2, 2, 934, 1702, 0, 2, None),
    ("spin", 3, 0): (64, 8, 8, 4, 0, 0, 0, -1, None, LF.END_NONE),
    ("spin", 3, 1): (64, None, 56, 19, 6, 30, 50, 0, 2, None),
    ("spin", 10, 1): (22528, None, 22506, 6143, 1022, 12264, 22486, 0, 2, None),
    ("2pc", 3, 3): (288, None, 0, 0, 0, 0, 0, -1, None, LF.END_NONE),
    ("2pc", 3, 4): (288, None, 280, 0, 0, 27, 280, 0, 4, LF.END_STUTTER),
}
# A terminal state that the search's own rule does not flag: 6 is first reached through 1, where "odd" held
# (depth 2), and later along 0, 2, 4, 8, 6, on which it never holds. The pass must end its witness there.
LATE_TERMINAL = ("dgraph", ((0, 1, 6), (0, 2, 4, 8, 6)))

# Duplicate init states: LiveGraph's optional `dup` repeats the roots 0 .. dup-1 after the 64 roots. Root 10,
# the first one in FairF, is among the repeated ones, so the arena holds its state twice.
DUP_ROOTS = ((12, 2, 1, 2, 0, 64), 16)


def dup_roots_graph():
    succ, inits, cond = __import__("live_ref").live_graph(*DUP_ROOTS[0])
    return succ, inits + list(range(DUP_ROOTS[1])), cond, DUP_ROOTS[0][1]


# too large for the restatement in a test that takes seconds: the device is compared with these figures
GPU_ANCHORS = {
    ("live", (16, 3, 26, 2, 0, 1)): (61601, 30816, 23183, 2, 1, 14261, 23181, 0, 0, None),
    ("live", (20, 2, 1, 3, 0, 1)): (836531, 557136, 415058, 3, 2, 236254, 415058, 0, None, None),
}
ANCHOR_KEYS = ("unique", "not_p_states", "surviving", "components", "fair_components", "goal_states", "fair_states",
               "init_index")


def graph_of(case):
    """(succ, inits, cond, nslots) of a case."""
    import live_ref
    if case[0] == "dgraph":
        return live_ref.dgraph([list(p) for p in case[1]]) + (256,)
    if case[0] == "live":
        return live_ref.live_graph(*case[1]) + (case[1][1],)
    if case[0] == "spin":
        succ, inits = spin_lock(case[1])
        return succ, inits, (some_served if case[2] == 0 else every_served(case[1])), 2 * case[1] + 1
    succ, inits = LF.two_phase(case[1])
    return succ, inits, LF.TWO_PHASE_LIVE_PROPS[case[2]][1], 2 + 5 * case[1]
