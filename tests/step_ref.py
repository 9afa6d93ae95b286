"""An independent pure-Python restatement of the step pass: the StepGraph and
StepDGraph fixtures, breadth-first depths and the FIFO tree, the three counts per step property and the
seed. Nothing here calls the engine.

A graph is `succ`: dict state -> list of (slot, action id, next state) in slot order (a slot whose `apply`
refuses is simply absent), closed under successors; `inits` lists the init states in order; a step property
is `holds(s, slot, t)`.
"""
M64 = (1 << 64) - 1

# (n_bits, degree, seed, f_mod, t_mod, roots) -> (unique, edges,
#   "no forbidden step": (violations, sources, seed (depth, v, slot) or None),
#   "never down":        (violations, sources, seed)): the issue's anchors
ANCHORS = {
    (6, 2, 1, 5, 0, 1): (44, 88, (13, 13, (2, 29, 1)), (45, 29, (1, 34, 1))),
    (8, 2, 1, 7, 0, 1): (209, 418, (64, 62, (2, 160, 1)), (212, 144, (1, 226, 0))),
    (12, 2, 1, 64, 0, 1): (3278, 6556, (95, 95, (3, 594, 0)), (3301, 2204, (1, 1839, 1))),
    (12, 3, 3, 1 << 40, 0, 1): (3833, 11499, (0, 0, None), (5700, 2871, (1, 2572, 1))),
    (12, 2, 1, 50, 16, 1): (3146, 5966, (124, 121, (3, 594, 0)), (2997, 1998, (1, 1839, 1))),
    (12, 2, 1, 300, 0, 64): (3306, 6612, (28, 28, (1, 3491, 1)), (3313, 2212, (0, 1, 0))),
    (16, 2, 1, 1000, 0, 1): (52173, 104346, (105, 105, (9, 30931, 0)), (52103, 34694, (1, 59183, 0))),
    (16, 3, 7, 20000, 0, 1): (61630, 184890, (9, 9, (7, 43214, 2)), (92205, 46081, (1, 28277, 0))),
}


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def step_graph(n_bits, degree, seed, f_mod, t_mod=0, roots=1, dup=0):
    """(succ, inits, props) of StepGraph(...) over the nodes v (the one-word form; the padded forms have the
    same graph): props = [holds of "no forbidden step", holds of "never down"]."""
    def r(v, k):
        return fmix64((fmix64((seed & M64) ^ v) + k) & M64)

    def actions(v):
        if t_mod > 0 and r(v, degree) % t_mod == 0:
            return []
        return [(k, k, r(v, k) & ((1 << n_bits) - 1)) for k in range(degree)]

    inits = list(range(roots)) + list(range(dup))
    succ, todo = {}, list(inits)
    while todo:
        v = todo.pop()
        if v in succ:
            continue
        succ[v] = actions(v)
        todo.extend(t for _, _, t in succ[v])
    forbidden = lambda s, k, t: not (f_mod > 0 and r(s, degree + 3 + k) % f_mod == 0)  # noqa: E731
    down = lambda s, k, t: not t < s  # noqa: E731
    return succ, inits, [forbidden, down]


def step_dgraph(forbidden, paths):
    """(succ, inits, props) of StepDGraph(forbidden, paths): the slot and the action id are the destination."""
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
        succ[v] = [(b, b, b) for b in sorted(edges.get(v, ()))]
        todo.extend(b for _, _, b in succ[v])
    bad = {tuple(f) for f in forbidden}
    return succ, sorted(inits), [lambda s, k, t: (s, k) not in bad]


def fifo_tree(succ, inits):
    """(depth, parent) of the reference's single-threaded search: level 0 is visited in REVERSE init order, a
    state's parent is the first visited state that lists it, through the first such slot: parent[s] = (state,
    action id), None for an init state."""
    depth, parent, queue = {}, {}, []
    for s in reversed(inits):
        if s not in depth:
            depth[s], parent[s] = 0, None
            queue.append(s)
    for s in queue:  # (grows while it is walked)
        for _, a, t in succ[s]:
            if t not in depth:
                depth[t], parent[t] = depth[s] + 1, (s, a)
                queue.append(t)
    return depth, parent


def check(succ, inits, holds):
    """dict(unique, edges, violations, sources, seed, depth, slot, actions, states, init_index) of one step
    property: the seed is the violating edge of the lowest source depth, then the lowest source (a node is word 0
    of its state, and no two states share it), then the lowest slot; actions / states: the FIFO tree path to the
    source, then the seed's step. seed is None where the property holds."""
    depth, parent = fifo_tree(succ, inits)
    assert set(depth) == set(succ)
    edges = violations = sources = 0
    best = None
    for s, out in succ.items():
        bad = [(k, a, t) for k, a, t in out if not holds(s, k, t)]
        edges += len(out)
        violations += len(bad)
        sources += bool(bad)
        if bad:
            cand = (depth[s], s, bad[0][0], s, bad[0][1], bad[0][2])
            best = cand if best is None or cand[:3] < best[:3] else best
    res = {"unique": len(succ), "edges": edges, "violations": violations, "sources": sources, "seed": None}
    if best is not None:
        d, _, slot, s, a, t = best
        states, actions = [t, s], [a]
        while parent[states[-1]] is not None:
            ps, pa = parent[states[-1]]
            states.append(ps)
            actions.append(pa)
        states.reverse()
        actions.reverse()
        res.update(seed=s, depth=d, slot=slot, actions=actions, states=states, init_index=inits.index(states[0]))
    return res


def replay(succ, init, actions):
    """The states of the path that the action ids describe from `init` (the first slot of each id), or None."""
    states = [init]
    for a in actions:
        nxt = [t for _, b, t in succ[states[-1]] if b == a]
        if not nxt:
            return None
        states.append(nxt[0])
    return states
