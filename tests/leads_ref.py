"""An independent pure-Python restatement of the leads-to check (`P ~> Q`, and
always-eventually where P is true), built on the four restatements of the complete `eventually` check
(tests/live_ref.py, live_fair_ref.py, live_weak_ref.py, live_strong_ref.py). Nothing here calls the engine.

A graph is `succ`: dict state -> list of (action id, next state) in slot order, closed under successors;
`inits` lists the init states in order; `cond(s)` is the TARGET condition Q, `trig(s)` the TRIGGER P;
`nslots` is the model's `max_actions()`; `key(s)` is the state as the engine's words, compared as a tuple
from word 0 (every model here has one word that decides: LeadsGraph's v, ReqLock's packed word, a node).

For a mode in MODES, X_Q is the mode's set for the condition Q: F_p (none), F_p' (progress), FairF (weak,
strong). violating = {s : trig(s) and s in X_Q}; the seed is the violating state of lowest breadth-first
depth, then of lowest key; the witness is the FIFO tree path to the seed followed by the mode's own witness
started at the seed.
"""
import live_fair_ref as LF
import live_ref as LR
import live_strong_ref as LS
import live_weak_ref as LW

MODES = ("none", "progress", "weak", "strong")
FAIRNESS = {"none": 0, "progress": 1, "weak": 2, "strong": 3}


def fifo_tree(succ, inits):
    """(depth, parent) of the reference's single-threaded order: level 0 is popped in REVERSE init order, a
    popped state queues its successors in slot order, and the first state to generate t is its parent.
    parent[t] = (parent state, action id); None for level 0."""
    depth, parent, queue = {}, {}, []
    for s in reversed(inits):
        if s not in depth:
            depth[s], parent[s] = 0, None
            queue.append(s)
    head = 0
    while head < len(queue):
        s = queue[head]
        head += 1
        for a, t in succ[s]:
            if t not in depth:
                depth[t], parent[t] = depth[s] + 1, (s, a)
                queue.append(t)
    assert len(depth) == len(succ)
    return depth, parent


def x_set(succ, cond, mode, nslots):
    """(X_Q, context): context holds what the mode's witness needs (the fixpoint, and for the fair modes the
    ranks, the sinks and the fair components or nodes)."""
    if mode in ("none", "progress"):
        _, f = LF.fixpoint(succ, cond, skip_self=mode == "progress")
        if mode == "none":  # (the two fixpoints must agree with the mode off: live_fair_ref's own claim)
            assert f == LR.fixpoint(succ, cond)[1]
        return f, {"f": f}
    _, f = LF.fixpoint(succ, cond, skip_self=True)
    if mode == "weak":
        fair = [c for c in LW.components(succ, f) if LW.is_fair(succ, c, nslots)]
    else:
        fair = [c for _, c, ok in LS.tree(succ, f) if ok]
    sinks = {s for s in f if not LW.moves(succ, s)}
    goal = set(sinks)
    for c in fair:
        goal |= c
    rank = LW.ranks(succ, f, goal)
    return set(rank), {"f": f, "rank": rank, "sinks": sinks, "fair": fair}


def check(succ, inits, cond, trig, mode, nslots, key=lambda s: s):
    """dict(unique, triggered, pending, violating, x (|X_Q|), seed, depth, init_index, prefix_states (init ..
    seed), prefix_actions, and the mode's own witness from the seed: none / progress: suffix_states,
    suffix_actions, loop_start (index into the suffix; -1), end_kind; weak / strong: stem (actions),
    stem_states, end_kind, comp (the fair component or node the stem ends in, or None)). seed is None and
    the rest absent if nothing violates."""
    x, ctx = x_set(succ, cond, mode, nslots)
    assert not any(cond(s) for s in x)  # X_Q is a subset of N_p
    depth, parent = fifo_tree(succ, inits)
    res = {"unique": len(succ), "triggered": sum(1 for s in succ if trig(s)),
           "pending": sum(1 for s in succ if trig(s) and not cond(s)), "x": len(x), "seed": None}
    viol = [s for s in succ if trig(s) and s in x]
    res["violating"] = len(viol)
    if not viol:
        return res
    seed = min(viol, key=lambda s: (depth[s], key(s)))
    chain, acts, s = [seed], [], seed
    while parent[s] is not None:
        s, a = parent[s]
        chain.append(s)
        acts.append(a)
    chain.reverse()
    acts.reverse()
    res.update(seed=seed, depth=depth[seed], prefix_states=chain, prefix_actions=acts, init_index=inits.index(chain[0]))
    if mode in ("none", "progress"):
        w = LF.witness(succ, [seed], ctx["f"], skip_self=mode == "progress")
        res.update(suffix_states=w["states"], suffix_actions=w["actions"], loop_start=w["loop_start"], end_kind=w["end_kind"])
    else:
        acts, sts = LW.descend(succ, ctx["rank"], seed)
        g = ([seed] + sts)[-1]
        res.update(stem=acts, stem_states=[seed] + sts, comp=None)
        if g in ctx["sinks"]:
            res["end_kind"] = LF.END_STUTTER if succ[g] else LF.END_TERMINAL
        else:
            res["end_kind"] = LF.END_LOOP
            res["comp"] = next(c for c in ctx["fair"] if g in c)
    return res


def replay(succ, start, actions):
    """The states the action ids lead through from `start` (the first listed step with that id), or None."""
    states, s = [start], start
    for a in actions:
        nxt = [t for x, t in succ[s] if x == a]
        if not nxt:
            return None
        s = nxt[0]
        states.append(s)
    return states


def problems(succ, inits, cond, trig, mode, nslots, init_index, actions, trigger_index, loop_start, end_kind):
    """What is wrong with a whole leads-to witness by the acceptance rule ([] if nothing): every step is listed,
    the trigger holds at trigger_index, the condition holds on no state from there on, and the suffix ends as
    the mode allows: at a terminal state, (any mode but none) at a stutter end, or closing a loop on a state of
    the suffix; a fair mode's loop is fair (loop_problems of that mode's restatement)."""
    states = replay(succ, inits[init_index], actions)
    if states is None:
        return ["the actions cannot be replayed"]
    bad = []
    if not 0 <= trigger_index < len(states):
        return ["trigger_index is outside the path"]
    if not trig(states[trigger_index]):
        bad.append("the trigger does not hold at trigger_index")
    bad += [f"the condition holds at index {i}" for i in range(trigger_index, len(states)) if cond(states[i])]
    last = states[-1]
    if end_kind == LF.END_LOOP:
        if not trigger_index <= loop_start < len(states) - 1:
            bad.append("loop_start is before trigger_index or not before the last state")
        elif states[loop_start] != last:
            bad.append("the last state does not repeat the state at loop_start")
        elif mode == "weak":
            bad += LW.loop_problems(succ, cond, nslots, last, actions[loop_start:])
        elif mode == "strong":
            bad += LS.loop_problems(succ, cond, nslots, last, actions[loop_start:])
        if mode != "none" and any(a == b for a, b in zip(states[trigger_index:], states[trigger_index + 1:])):
            bad.append("a step of the suffix returns its own state")
    elif end_kind == LF.END_TERMINAL:
        if succ[last]:
            bad.append("the last state is not terminal")
    elif end_kind == LF.END_STUTTER:
        if mode == "none" or not succ[last] or any(t != last for _, t in succ[last]):
            bad.append("the last state is no stutter end (or the mode has none)")
    else:
        bad.append("no end kind")
    return bad


# ---- the models, restated ------------------------------------------------------------------------------------

def leads_graph(n_bits, degree, seed, p_mod, t_mod, roots, q_mod, dup=0):
    """(succ, inits, cond, trig_by_property, nslots) of LeadsGraph: LiveGraph's graph; property 1 "armed ~>
    marked" triggers where q_mod > 0 and r(v, degree + 2) % q_mod == 0, property 2 everywhere."""
    succ, inits, cond = LR.live_graph(n_bits, degree, seed, p_mod, t_mod, roots)
    inits = inits + list(range(dup))

    def r(v, k):
        return LR.fmix64((LR.fmix64((seed & LR.M64) ^ v) + k) & LR.M64)

    trig = {1: (lambda v: q_mod > 0 and r(v, degree + 2) % q_mod == 0), 2: (lambda v: True)}
    return succ, inits, cond, trig, degree


def req_lock(n):
    """(succ, inits) of ReqLock(n). A state is (holder, waiting, tick): holder 0 = free, i + 1 = thread i;
    waiting a bit set. Slots: i < n Request(i) (i neither waits nor holds), n + i Acquire(i) (free, i waits),
    2n + i Release(i) (i holds), 3n Tick. The action id is the slot."""
    def actions(s):
        holder, waiting, tick = s
        out = []
        for i in range(n):
            if not waiting >> i & 1 and holder != i + 1:
                out.append((i, (holder, waiting | 1 << i, tick)))
        for i in range(n):
            if holder == 0 and waiting >> i & 1:
                out.append((n + i, (i + 1, waiting & ~(1 << i), tick)))
        for i in range(n):
            if holder == i + 1:
                out.append((2 * n + i, (0, waiting, tick)))
        out.append((3 * n, (holder, waiting, tick ^ 1)))
        return out

    init = (0, 0, 0)
    succ, todo = {}, [init]
    while todo:
        s = todo.pop()
        if s in succ:
            continue
        succ[s] = actions(s)
        todo.extend(t for _, t in succ[s])
    return succ, [init]


def req_lock_word(s, n):
    return s[0] | s[1] << 5 | s[2] << (5 + n)


def req_lock_states(n):
    return ((1 << n) + n * (1 << (n - 1))) * 2


def leads_dgraph(paths, triggers):
    """(succ, inits, cond, trig, nslots) of LeadsDGraph: DGraph's graph from paths, "trigger ~> odd"."""
    succ, inits, cond = LR.dgraph(paths)
    t = set(triggers)
    return succ, inits, cond, (lambda v: v in t), 256


# ---- the anchors (computed with this module; the issue's table) ----------------------------------------------
# LeadsGraph (n_bits, degree, seed, p_mod, t_mod, roots, q_mod) -> (unique, triggered, pending,
#   {mode: (violating, seed or None, depth or None)} for property 1, (violating, seed, depth) of property 2 in mode none)
GRAPH_ANCHORS = {
    (12, 2, 1, 2, 0, 1, 7): (3278, 467, 237, {"none": (68, 333, 5), "progress": (68, 333, 5), "weak": (63, 333, 5), "strong": (63, 333, 5)},
                             (475, 594, 3)),
    (12, 2, 3, 2, 0, 1, 7): (3269, 461, 235, {"none": (9, 3324, 9), "progress": (7, 3324, 9), "weak": (7, None, None), "strong": (7, None, None)},
                             (104, 0, 0)),
    (12, 2, 1, 3, 16, 1, 5): (3146, 631, 413, {"none": (330, 1696, 4), "progress": (330, None, None), "weak": (330, None, None),
                                               "strong": (330, None, None)}, (1702, 0, 0)),
    (12, 2, 1, 2, 0, 64, 7): (3306, 471, 240, {"none": (68, 3326, 1), "progress": (68, None, None), "weak": (63, None, None),
                                               "strong": (63, None, None)}, (477, 10, 0)),
    (16, 3, 7, 4, 0, 1, 9): (61630, 6855, 5143, {"none": (5048, 43794, 2), "progress": (5048, None, None), "weak": (5048, None, None),
                                                 "strong": (5048, None, None)}, (45479, 0, 0)),
    (12, 2, 1, 2, 0, 1, 0): (3278, 0, 0, {"none": (0, None, None), "progress": (0, None, None), "weak": (0, None, None), "strong": (0, None, None)},
                             (475, 594, 3)),
}
# the 12-bit rows (3 K states each); the 16-bit row (61 K states, a second per mode here) has tests of its own
SMALL_ROWS = [k for k in GRAPH_ANCHORS if k[0] == 12]
