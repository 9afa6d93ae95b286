"""An independent pure-Python restatement of the complete `eventually` check:
the LiveGraph fixture, the fixpoint F_p as plain Jacobi rounds over a dict of successors, and the
deterministic witness. Nothing here calls the engine.

A graph is `succ`: dict state -> list of (action id, next state) in slot order (a slot whose `apply`
refuses is simply absent), closed under successors; `inits` lists the init states in order; `cond(s)`
is the property's condition at s.
"""
M64 = (1 << 64) - 1

# (n_bits, degree, seed, p_mod, t_mod, roots) -> (unique, |N|, |F|, first init in F or None,
# witness steps or None, loop_start (-1: terminal) or None): the issue's anchors
ANCHORS = {
    (8, 2, 1, 3, 0, 1): (209, 129, 85, 0, 8, 3),
    (12, 2, 1, 2, 0, 1): (3278, 1642, 475, None, None, None),
    (12, 2, 3, 2, 0, 1): (3269, 1628, 104, 0, 20, 18),
    (12, 2, 1, 3, 16, 1): (3146, 2096, 1702, 0, 12, -1),
    (12, 2, 1, 2, 0, 64): (3306, 1655, 477, 10, 15, 7),
    (16, 2, 1, 2, 0, 1): (52173, 26005, 1507, None, None, None),
    (16, 3, 7, 4, 0, 1): (61630, 46288, 45479, 0, 614, 217),
}


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def live_graph(n_bits, degree, seed, p_mod, t_mod, roots):
    """(succ, inits, cond) of LiveGraph(n_bits, degree, seed, p_mod, t_mod, roots), reachable part."""
    def r(v, k):
        return fmix64((fmix64((seed & M64) ^ v) + k) & M64)

    def actions(v):
        if t_mod > 0 and r(v, degree) % t_mod == 0:
            return []
        return [(k, r(v, k) & ((1 << n_bits) - 1)) for k in range(degree)]

    inits = list(range(roots))
    succ, todo = {}, list(inits)
    while todo:
        v = todo.pop()
        if v in succ:
            continue
        succ[v] = actions(v)
        todo.extend(n for _, n in succ[v])
    return succ, inits, (lambda v: p_mod > 0 and r(v, degree + 1) % p_mod == 0)


def dgraph(paths):
    """(succ, inits, cond) of the reference's DGraph fixture built from `paths` (property "odd")."""
    edges, inits = {}, set()
    for p in paths:
        inits.add(p[0])
        for a, b in zip(p, p[1:]):
            edges.setdefault(a, set()).add(b)
    succ, todo = {}, sorted(inits)
    while todo:
        v = todo.pop()
        if v in succ:
            continue
        succ[v] = [(b, b) for b in sorted(edges.get(v, ()))]
        todo.extend(b for _, b in succ[v])
    return succ, sorted(inits), (lambda v: v % 2 == 1)


def fixpoint(succ, cond):
    """(N_p, F_p, rounds): F_p is the greatest subset of N_p = {s: not cond(s)} in which every state
    is terminal or has a successor in F_p. Jacobi: every round tests against the previous round's set."""
    n = {s for s in succ if not cond(s)}
    f, rounds = set(n), 0
    while True:
        rounds += 1
        g = {s for s in f if not succ[s] or any(t in f for _, t in succ[s])}
        if g == f:
            return n, f, rounds
        f = g


def witness(succ, inits, f):
    """None if no init state is in F, else dict(init_index, states, actions, loop_start)."""
    for i, s in enumerate(inits):
        if s in f:
            break
    else:
        return None
    states, actions, seen = [s], [], {s: 0}
    while succ[s]:
        a, s = next((a, t) for a, t in succ[s] if t in f)
        actions.append(a)
        states.append(s)
        if s in seen:
            return {"init_index": i, "states": states, "actions": actions, "loop_start": seen[s]}
        seen[s] = len(states) - 1
    return {"init_index": i, "states": states, "actions": actions, "loop_start": -1}


def check(succ, inits, cond):
    """dict(unique, not_p_states, surviving, rounds, witness) of one graph."""
    n, f, rounds = fixpoint(succ, cond)
    return {"unique": len(succ), "not_p_states": len(n), "surviving": len(f), "rounds": rounds,
            "witness": witness(succ, inits, f)}
