// The complete `eventually` check (opt-in: sr_opts.liveness, `CheckerBuilder.complete_liveness()`;
// DESIGN.md §12). The search refutes an `eventually` property only at a terminal state reached with
// the property's bit still set, and the bits are not part of the visited key (src/checker/bfs.rs:
// 212-272), so two families of counterexamples are reported as "holds": a state first reached along
// a path on which the property held and later along one on which it did not (the FIXME at bfs.rs:
// 239-245), and a path that runs round a cycle on which it never holds (bfs.rs:249-256). Once a
// search has explored everything, the arena holds the reachable set and the visited set finds any
// successor, so the exact answer is a backward fixpoint over that set.
//
// For an `eventually` property p without a discovery:
//   R        the reachable set (the arena);
//   succ(s)  the states `apply` yields over the slots of enabled(s), in slot order; a slot whose
//            `apply` returns false contributes nothing, exactly as in expansion; succ(s) is in R;
//   terminal(s)  succ(s) is empty (`is_terminal` without its "already generated" clause);
//   N_p      { s in R : the condition of p does not hold at s };
//   F_p      the greatest subset of N_p in which every state is terminal or has a successor in F_p
//            (EG !p with deadlock states as sinks; no fairness, as the reference defines `eventually`).
// p has a counterexample iff some init state is in F_p. F_p is unique, so states may be removed in
// place, in any order, until nothing changes; the number of rounds is an implementation detail.
// The witness is deterministic: start at the init state of lowest index (order of `init_states`) in
// F_p; from s_t go to apply(s_t, a) for the lowest slot a whose result is in F_p; stop at a terminal
// s_t (loop_start = -1), otherwise at the first s_t equal to an earlier s_j (loop_start = j). The
// walk follows a function on a finite set, so it ends within |F_p| steps. It is not the shortest
// counterexample.
//
// PROGRESS FAIRNESS (opt-in: sr_opts.liveness = SR_LIVENESS_PROGRESS, `complete_liveness(fairness=
// "progress")`): the same rule over the graph without its self-loops, so that an action that leaves
// the state as it is ("nothing changed": 2pc's RmRcvCommitMsg at a Committed rm) is no step.
//   succ'(s)      succ(s) \ {s}: a successor whose W words all equal those of s is no successor;
//   terminal'(s)  succ'(s) is empty: s is terminal (succ(s) is empty), or a STUTTER END (succ(s) is
//                 not empty and every member is s). Both are sinks: a run that can only stutter stays
//                 there legitimately;
//   N_p           as above;
//   F_p'          the greatest subset of N_p in which every state is terminal' or has a successor in
//                 succ'(s) and F_p'.
// The witness steps over succ' only: from the init state of lowest index in F_p', the lowest slot
// whose result differs from s_t and is in F_p', to a terminal' state (loop_start = -1) or the first
// repeated state, so a closed loop has at least two distinct states. No discovery then means: p holds
// on every maximal path that does not stay forever in ONE state that has a successor other than
// itself. It is NOT per-action weak fairness: a cycle through two or more distinct states still
// refutes p, however unfair the run round it is; fair strongly connected components are not built
// in THIS mode (weak fairness, below, builds them). The simulation checker's loop detection is not
// changed (a self-loop still closes a lasso there), and what the plain mode refuses (plugins,
// partitions, symmetry, target_state_count) this mode refuses too.
//
// WEAK FAIRNESS (opt-in: sr_opts.liveness = SR_LIVENESS_WEAK, `CheckerBuilder.weak_fairness()`). The terms
// of the progress mode (succ', terminal', N_p, F_p') stay as defined.
//   fairness class  an action SLOT: an action of 2pc, a thread's step. A model opts in with `static
//                   constexpr bool FAIR_SLOTS = true` (models.hpp fair_slots_model): DGraph, LiveGraph,
//                   TwoPhase (so TwoPhaseLive), SpinLock. Every other model is refused at spawn: where a
//                   slot is a network position (the actor encodings, paxos, the registers) it names no
//                   action. The refusals of the other modes apply unchanged.
//   me(s, a)        "moving-enabled": slot a is in enabled(s), apply(s, a) succeeds and its result differs
//                   from s (TLA's ENABLED <A>_v: a no-op step neither creates nor discharges an
//                   obligation). Where live_moves_model<M> holds, `enabled_moves` gives the mask.
//   G'              the graph on F_p' with the succ' edges that stay in F_p' (no self edge).
//   fair component  a strongly connected component C of G' with two or more states such that for every
//                   slot a < max_actions(): some s in C has !me(s, a), or some s in C has me(s, a) and
//                   apply(s, a) in C.
//   goal            the terminal' states of F_p' and the members of fair components;
//   FairF           the states of F_p' from which goal is reachable in G'; rank(s) is the length of the
//                   shortest such path (computed level by level, so it is unique).
// p has a counterexample iff some init state is in FairF; no discovery means p holds on every maximal run
// that is weakly fair to every slot. MAXIMAL components suffice: if a strongly connected S inside C meets
// the condition, so does C, because both disjuncts ("some state has !me", "some state's a-step stays
// inside") only become easier in a larger set, and C is strongly connected; so a fair run that stays in
// N_p for ever exists iff a maximal component is fair, and no recursive decomposition is needed. STRONG
// fairness is not monotone like this (a larger set may enable a slot that the smaller never enables)
// and is a mode of its own (STRONG FAIRNESS, below). Weak fairness subsumes progress fairness: a run that stutters for ever at a state
// with a moving slot is unfair to that slot.
// The witness is deterministic. Start at the init state of lowest index in FairF. STEM: from s take the
// lowest slot whose result t != s is in FairF with rank(t) < rank(s), until rank 0 at a state g. If g
// is terminal' the witness ends there (end_kind 1 or 3, loop_start -1). Otherwise g lies in a fair
// component C and a CLOSED WALK inside C from g follows; with cur = g, for the slots a = 0, 1, .. in
// order: skip a if the loop so far discharges it (a state on the loop, g included, has !me(., a), or a
// step of the loop took a); else, if some state of C has !me(., a), go from cur to the nearest such state
// (ranks towards that target set inside C, lowest rank-decreasing slot); else go the same way to the
// nearest s in C with apply(s, a) in C and take a. After the last slot go to g the same way. The path's
// last state equals path[loop_start], loop_start the index of g, end_kind 2; the loop may pass a state
// more than once, and loop_start still means "the state the last state repeats". Cost: at most
// max_actions() + 1 rank fixpoints over C (reported as `segments`, not bounded).
//
// STRONG FAIRNESS (opt-in: sr_opts.liveness = SR_LIVENESS_STRONG, `CheckerBuilder.strong_fairness()`). The
// terms above (succ', terminal', F_p', G', me(s, a), a slot as the fairness class of a FAIR_SLOTS model)
// stay as defined.
//   strongly fair set  S, two or more states of F_p', strongly connected in G'[S], such that for every slot
//                   a < max_actions(): no s in S has me(s, a), or some s in S has me(s, a) and apply(s, a) in
//                   S. A step counts for every slot whose successor it reaches, as live_loop_fair counts it.
//   decomposition   for a component C (two or more states) of G'[X], bad(C) is the set of slots that are
//                   moving-enabled somewhere in C and whose steps all leave C. With bad(C) empty, C is a FAIR
//                   NODE and is decomposed no further; otherwise X' = C \ { s : me(s, a) for some a in bad(C) }
//                   is decomposed in the same way; the start is X = F_p' at depth 1. The result is a tree whose
//                   nodes, fair nodes and depth (`levels`) do not depend on the order of work.
//   goal            the sinks of F_p' and the members of fair nodes (which are pairwise disjoint);
//   FairF, rank     as in the weak mode, towards this goal.
// p has a counterexample iff some init state is in FairF; no discovery means p holds on every maximal run that
// is strongly fair to every slot (a slot that is moving-enabled again and again is taken again and again),
// which subsumes weak fairness. The maximal components do NOT suffice here, as they do above: a larger set may
// enable a slot that a smaller one never enables, so a strongly fair S may lie inside a component C that is
// not fair. But S cannot hold a state that enables a slot a of bad(C): S would have to take a inside S, so
// inside C, and no a-step stays in C. So S lies in X', it is strongly connected there, hence inside one
// component of G'[X'], and by induction inside a fair node; nothing is lost by taking those states out. A
// fair node is itself a strongly fair set, and a run that stays in N_p for ever and is strongly fair visits
// some strongly connected set S infinitely often and takes inside S every slot that S enables: it exists
// iff a fair node or a sink is reachable.
// The witness is deterministic: the weak mode's stem to rank 0 at a state g. A sink g ends it (end_kind 1 or
// 3, loop_start -1, loop_len 0). Otherwise a CLOSED WALK inside g's fair node C follows; with cur = g, for the
// slots a = 0, 1, .. in order: skip a if no member of C has me(., a) or a step of the loop so far took it;
// else go from cur to the nearest s in C with me(s, a) and apply(s, a) in C (ranks inside C, lowest rank-
// lowering slot: the weak mode's LIVE_PLAN_TAKE segment) and take a. After the last slot go home to g
// (LIVE_PLAN_HOME). There is no NOTME segment. The walk takes every slot that C enables anywhere, so it is
// strongly fair on its own states (live_loop_strong_fair); end_kind 2, loop_start = stem_len.
//
// The per-state rule and the witness step are ONE function, live_step below, which the kernels
// (kernels_live.hpp: live_trim, live_walk) and the host form (live_host, the sr_liveness_host entry
// point) instantiate; they differ only in how "is this successor in the set" is answered (the alive
// bitmap by visited-set slot on the device, a hash map on the host).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/stateright_gpu.h"
#include "device.hpp"
#include "kernels.hpp"

namespace sr {

enum LiveStep : int { LIVE_TERMINAL = -1, LIVE_DEAD = -2, LIVE_STUTTER = -3 };

// Whether s is in N_p (p an `eventually` property: discovers() is its condition).
template <class M>
SR_HD bool live_not_p(const M& m, int p, const u64* s) {
    return !m.discovers(p, s);
}

template <int W>
SR_HD bool live_same(const u64* a, const u64* b) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < W; ++i) eq = eq && a[i] == b[i];
    return eq;
}

// Whether the model's own hook names its self-loops exactly (2pc: `enabled_moves` leaves the slots
// that change the state, and only those), so that the progress mode need not compare states.
template <class M>
constexpr bool live_moves_model = exact_moves_model<M> && has_enabled_moves<M>::value;

// The successors of s in slot order, among the enabled slots of rank first, first + stride, ...
// (stride a power of two; the host and live_trim take all of them: 0, 1; the lanes of live_walk
// share them: lane, 64), up to the first one for which alive(ns) holds. Returns that slot, with
// the successor in out; else LIVE_DEAD if some slot had a successor, LIVE_TERMINAL if none had.
// FAIR (progress fairness, above): a successor equal to s is skipped and is no successor; with none
// left the result is LIVE_STUTTER if a slot gave s itself (among ALL enabled slots where the model's
// hook counts them, among this call's share of them otherwise), LIVE_TERMINAL if no slot gave
// anything. MOVES = false compares the states even where the model's hook would answer (tests).
template <bool FAIR = false, bool MOVES = true, class M, class Alive>
SR_HD int live_step(const M& m, const u64* s, Alive&& alive, u64* out, u32 first = 0, u32 stride = 1) {
    u64 mask[M::MW];
    bool any = false;
    u32 r = 0;
    if constexpr (!FAIR) {
        m.enabled(s, mask);
        for (int w = 0; w < M::MW; ++w)
            for (u64 bits = mask[w]; bits; bits &= bits - 1, ++r) {
                if ((r & (stride - 1)) != first) continue;
                const int a = w * 64 + __builtin_ctzll(bits);
                if (!m.apply(s, a, out)) continue;
                any = true;
                if (alive(out)) return a;
            }
        return any ? LIVE_DEAD : LIVE_TERMINAL;
    } else {
        bool self = false;
        if constexpr (MOVES && live_moves_model<M>) self = m.enabled_moves(s, mask) != 0;
        else m.enabled(s, mask);
        for (int w = 0; w < M::MW; ++w)
            for (u64 bits = mask[w]; bits; bits &= bits - 1, ++r) {
                if ((r & (stride - 1)) != first) continue;
                const int a = w * 64 + __builtin_ctzll(bits);
                if (!m.apply(s, a, out)) continue;
                if constexpr (!(MOVES && live_moves_model<M>)) {
                    if (live_same<M::W>(out, s)) {
                        self = true;
                        continue;
                    }
                }
                any = true;
                if (alive(out)) return a;
            }
        return any ? LIVE_DEAD : self ? LIVE_STUTTER : LIVE_TERMINAL;
    }
}

// ---- weak fairness: the per-state pieces, shared by the kernels (kernels_live.hpp) and live_host_weak ----

// The moving successors of s in slot order, among the enabled slots of rank first, first + stride, ..
// (as live_step shares them): f(a, ns) for every slot a with me(s, a), ns = apply(s, a), and `me` the
// mask of those slots. MOVES as in live_step.
template <bool MOVES = true, class M, class F>
SR_HD void live_moving(const M& m, const u64* s, u64* me, F&& f, u32 first = 0, u32 stride = 1) {
    u64 mask[M::MW], out[M::W];
    if constexpr (MOVES && live_moves_model<M>) (void)m.enabled_moves(s, mask);
    else m.enabled(s, mask);
    u32 r = 0;
    for (int w = 0; w < M::MW; ++w) {
        me[w] = 0;
        for (u64 bits = mask[w]; bits; bits &= bits - 1, ++r) {
            if ((r & (stride - 1)) != first) continue;
            const int b = __builtin_ctzll(bits);
            if (!m.apply(s, w * 64 + b, out)) continue;
            if constexpr (!(MOVES && live_moves_model<M>)) {
                if (live_same<M::W>(out, s)) continue;
            }
            me[w] |= 1ull << b;
            f(w * 64 + b, out);
        }
    }
}

// The fairness predicate of a component from its two accumulators: and_me, the AND over its members of
// their me masks; or_took, the OR over its members of the slots whose successor is a member.
template <int MW>
SR_HD bool live_fair_masks(const u64* and_me, const u64* or_took) {
    bool fair = true;
#pragma unroll
    for (int w = 0; w < MW; ++w) fair = fair && (and_me[w] & ~or_took[w]) == 0;
    return fair;
}

// The witness' step choice: the lowest slot (of this call's share) whose moving successor has a rank
// below `below`, with the successor in out; -1 if none. rank_of(ns) is the successor's rank in the
// current domain (~0u outside it) and is asked in slot order up to the first hit; `me` is the mask
// of this call's share of the moving slots, all of them.
template <bool MOVES = true, class M, class Rank>
SR_HD int live_descend_step(const M& m, const u64* s, u32 below, Rank&& rank_of, u64* me, u64* out, u32 first = 0,
                            u32 stride = 1) {
    int best = -1;
    live_moving<MOVES>(
        m, s, me,
        [&](int a, const u64* ns) {
            if (best >= 0 || !below || !(rank_of(ns) < below)) return;
            best = a;
#pragma unroll
            for (int i = 0; i < M::W; ++i) out[i] = ns[i];
        },
        first, stride);
    return best;
}

// What the closed walk does about slot a, given the loop so far (notme: slots not moving-enabled at some
// state of it; taken: slots its steps took) and the component's and_me accumulator.
enum LivePlan : int { LIVE_PLAN_SKIP = 0, LIVE_PLAN_NOTME = 1, LIVE_PLAN_TAKE = 2, LIVE_PLAN_HOME = 3 };
inline int live_loop_plan(int a, const u64* notme, const u64* taken, const u64* and_me) {
    const u64 bit = 1ull << (a & 63);
    if ((notme[a >> 6] | taken[a >> 6]) & bit) return LIVE_PLAN_SKIP;
    return and_me[a >> 6] & bit ? LIVE_PLAN_TAKE : LIVE_PLAN_NOTME;
}

// Whether the closed walk states[0 .. len] (W words each; states[len] equals states[0]) is weakly fair,
// on its own states and steps: every slot below max_actions() is not moving-enabled at some state of
// it, or some step i goes to that slot's successor of state i.
template <class M>
bool live_loop_fair(const M& m, const u64* states, size_t len) {
    constexpr int W = M::W;
    if (!len || !std::equal(states, states + W, states + len * W)) return false;
    u64 notme[M::MW] = {}, taken[M::MW] = {}, me[M::MW];
    for (size_t i = 0; i < len; ++i) {
        live_moving<false>(m, states + i * W, me, [&](int a, const u64* ns) {
            if (std::equal(ns, ns + W, states + (i + 1) * W)) taken[a >> 6] |= 1ull << (a & 63);
        });
        for (int w = 0; w < M::MW; ++w) notme[w] |= ~me[w];
    }
    for (int a = 0; a < m.max_actions(); ++a)
        if (!((notme[a >> 6] | taken[a >> 6]) >> (a & 63) & 1)) return false;
    return true;
}

// ---- strong fairness: the predicate shared by the kernels (live_refine) and live_host_strong ----

// Whether a component is a fair node, from its two accumulators: or_me, the OR over its members of their me
// masks; or_took as above. The slots left in or_me & ~or_took are bad(C).
template <int MW>
SR_HD bool live_strong_masks(const u64* or_me, const u64* or_took) {
    bool fair = true;
#pragma unroll
    for (int w = 0; w < MW; ++w) fair = fair && (or_me[w] & ~or_took[w]) == 0;
    return fair;
}

// What the strong mode's closed walk does about slot a, given the slots its steps took so far and the fair
// node's or_me accumulator: there is no NOTME segment.
inline int live_strong_plan(int a, const u64* taken, const u64* or_me) {
    const u64 bit = 1ull << (a & 63);
    return (or_me[a >> 6] & bit) && !(taken[a >> 6] & bit) ? LIVE_PLAN_TAKE : LIVE_PLAN_SKIP;
}

// Whether the closed walk states[0 .. len] (as for live_loop_fair) is strongly fair on its own states and
// steps: every slot that is moving-enabled at some state of it is taken by one of its steps.
template <class M>
bool live_loop_strong_fair(const M& m, const u64* states, size_t len) {
    constexpr int W = M::W;
    if (!len || !std::equal(states, states + W, states + len * W)) return false;
    u64 some[M::MW] = {}, taken[M::MW] = {}, me[M::MW];
    for (size_t i = 0; i < len; ++i) {
        live_moving<false>(m, states + i * W, me, [&](int a, const u64* ns) {
            if (std::equal(ns, ns + W, states + (i + 1) * W)) taken[a >> 6] |= 1ull << (a & 63);
        });
        for (int w = 0; w < M::MW; ++w) some[w] |= me[w];
    }
    return live_strong_masks<M::MW>(some, taken);
}

inline sr_live_strong live_strong_none() {
    sr_live_strong s;
    std::memset(&s, 0, sizeof(s));
    s.stem_len = s.loop_len = -1;
    return s;
}

inline sr_live_weak live_weak_none() {
    sr_live_weak w;
    std::memset(&w, 0, sizeof(w));
    w.stem_len = w.loop_len = -1;
    return w;
}

inline sr_live_result live_result_none() {
    sr_live_result r;
    std::memset(&r, 0, sizeof(r));
    r.init_index = -1;
    r.witness_len = -1;
    r.loop_start = -1;
    return r;
}

}  // namespace sr

#include "kernels_live.hpp"

namespace sr {

template <class M>
std::vector<u64> init_states_of(const M& m);  // (engine.hpp)

// The check on the host, with no device: a search over at most max_states states, the fixpoint (in
// place, worklist by worklist as the device runs it) and the witness. FAIR: progress fairness; MOVES:
// see live_step.
struct LiveHost {
    sr_live_result r = live_result_none();
    u64 unique = 0;
    std::vector<u64> words;    // the witness' states, W words each (empty: no init state in F_p)
    std::vector<i64> actions;  // its canonical action ids, one per step
};

template <bool FAIR = false, bool MOVES = true, class M>
LiveHost live_host(const M& m, int p, u64 max_states) {
    constexpr int W = M::W;
    if (p < 0 || p >= M::NPROPS || m.expectation(p) != EVENTUALLY)
        throw Error(SR_ERR_ARG, "liveness: property " + std::to_string(p) + " is not an `eventually` property");
    struct H {
        size_t operator()(const std::vector<u64>& v) const {
            u64 h = 0;
            for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
            return (size_t)h;
        }
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<std::vector<u64>, u32, H> index;
    std::vector<std::vector<u64>> st;
    auto add = [&](const u64* s) {
        std::vector<u64> v(s, s + W);
        auto it = index.find(v);
        if (it != index.end()) return it->second;
        if (st.size() >= max_states)
            throw Error(SR_ERR_CAPACITY, "liveness: the model has more than " + std::to_string(max_states) + " reachable states (max_states)");
        const u32 i = (u32)st.size();
        index.emplace(v, i);
        st.push_back(std::move(v));
        return i;
    };
    const std::vector<u64> inits = init_states_of(m);
    const int k = (int)(inits.size() / W);
    std::vector<u32> init_idx;
    for (int i = 0; i < k; ++i) init_idx.push_back(add(&inits[(size_t)i * W]));
    for (size_t q = 0; q < st.size(); ++q) {
        const std::vector<u64> s = st[q];  // (a copy: add() grows st)
        for_each_successor(m, s.data(), [&](int, const u64* ns) { add(ns); });
    }
    LiveHost h;
    h.unique = st.size();
    h.r.ran = 1;
    std::vector<char> alive(st.size(), 0);
    std::vector<u32> wl, next;
    for (u32 i = 0; i < (u32)st.size(); ++i)
        if (live_not_p(m, p, st[i].data())) {
            alive[i] = 1;
            wl.push_back(i);
        }
    h.r.not_p_states = h.r.surviving = wl.size();
    auto is_alive = [&](const u64* ns) {
        auto it = index.find(std::vector<u64>(ns, ns + W));
        if (it == index.end()) throw Error(SR_ERR_NONDETERMINISM, "liveness: a successor of a reachable state is not in the reachable set");
        return alive[it->second] != 0;
    };
    u64 out[W];
    for (;;) {
        u64 removed = 0;
        next.clear();
        h.r.rounds += 1;
        h.r.examined += wl.size();
        for (u32 i : wl) {
            const int a = live_step<FAIR, MOVES>(m, st[i].data(), is_alive, out);
            if (a >= 0) next.push_back(i);
            else if (a == LIVE_DEAD) alive[i] = 0, ++removed;
        }
        wl.swap(next);
        h.r.surviving -= removed;
        if (!removed) break;
    }
    for (int i = 0; i < k && h.r.init_index < 0; ++i)
        if (alive[init_idx[i]]) h.r.init_index = i;
    if (h.r.init_index >= 0) {
        std::unordered_map<u32, i64> at;  // state -> its position on the path
        u32 cur = init_idx[h.r.init_index];
        for (i64 t = 0;; ++t) {
            h.words.insert(h.words.end(), st[cur].begin(), st[cur].end());
            auto seen = at.find(cur);
            if (seen != at.end()) {
                h.r.witness_len = t;
                h.r.loop_start = seen->second;
                h.r.end_kind = SR_LIVE_END_LOOP;
                break;
            }
            at.emplace(cur, t);
            const int a = live_step<FAIR, MOVES>(m, st[cur].data(), is_alive, out);
            if (a == LIVE_TERMINAL || a == LIVE_STUTTER) {
                h.r.witness_len = t;
                h.r.end_kind = a == LIVE_TERMINAL ? SR_LIVE_END_TERMINAL : SR_LIVE_END_STUTTER;
                break;
            }
            if (a < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a state of the fixpoint has no successor in it");
            h.actions.push_back(m.action_id(st[cur].data(), a));
            cur = index.at(std::vector<u64>(out, out + W));
        }
    }
    h.r.pass_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return h;
}

// The check under WEAK FAIRNESS on the host, with no device, by other algorithms than the device's:
// the host search and the progress fixpoint as live_host runs them, then Tarjan's algorithm
// (iterative) for the components of G', breadth-first ranks over predecessor lists, and the witness
// rule of the header. The per-state pieces (live_moving, live_fair_masks, live_descend_step,
// live_loop_plan) are the kernels'.
struct LiveHostWeak {
    LiveHost h;
    sr_live_weak w = live_weak_none();
};

template <bool MOVES = true, class M>
LiveHostWeak live_host_weak(const M& m, int p, u64 max_states) {
    constexpr int W = M::W, MW = M::MW;
    constexpr u32 NONE = ~0u;
    if constexpr (!fair_slots_model<M>) {
        throw Error(SR_ERR_UNSUPPORTED, "weak fairness: this model's slots are not fairness classes");
    } else {
        if (p < 0 || p >= M::NPROPS || m.expectation(p) != EVENTUALLY)
            throw Error(SR_ERR_ARG, "liveness: property " + std::to_string(p) + " is not an `eventually` property");
        struct H {
            size_t operator()(const std::vector<u64>& v) const {
                u64 h = 0;
                for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
                return (size_t)h;
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        std::unordered_map<std::vector<u64>, u32, H> index;
        std::vector<std::vector<u64>> st;
        auto add = [&](const u64* s) {
            std::vector<u64> v(s, s + W);
            auto it = index.find(v);
            if (it != index.end()) return it->second;
            if (st.size() >= max_states)
                throw Error(SR_ERR_CAPACITY, "liveness: the model has more than " + std::to_string(max_states) + " reachable states (max_states)");
            const u32 i = (u32)st.size();
            index.emplace(v, i);
            st.push_back(std::move(v));
            return i;
        };
        const std::vector<u64> inits = init_states_of(m);
        const int k = (int)(inits.size() / W);
        std::vector<u32> init_idx;
        for (int i = 0; i < k; ++i) init_idx.push_back(add(&inits[(size_t)i * W]));
        for (size_t q = 0; q < st.size(); ++q) {
            const std::vector<u64> s = st[q];  // (a copy: add() grows st)
            for_each_successor(m, s.data(), [&](int, const u64* ns) { add(ns); });
        }
        LiveHostWeak res;
        LiveHost& h = res.h;
        sr_live_weak& wk = res.w;
        h.unique = st.size();
        h.r.ran = wk.ran = 1;
        auto find = [&](const u64* ns) {
            auto it = index.find(std::vector<u64>(ns, ns + W));
            if (it == index.end()) throw Error(SR_ERR_NONDETERMINISM, "liveness: a successor of a reachable state is not in the reachable set");
            return it->second;
        };
        // the progress fixpoint, as live_host<true> runs it
        std::vector<char> alive(st.size(), 0);
        {
            std::vector<u32> wl, next;
            for (u32 i = 0; i < (u32)st.size(); ++i)
                if (live_not_p(m, p, st[i].data())) alive[i] = 1, wl.push_back(i);
            h.r.not_p_states = h.r.surviving = wl.size();
            auto is_alive = [&](const u64* ns) { return alive[find(ns)] != 0; };
            u64 out[W];
            for (;;) {
                u64 removed = 0;
                next.clear();
                h.r.rounds += 1;
                h.r.examined += wl.size();
                for (u32 i : wl) {
                    const int a = live_step<true, MOVES>(m, st[i].data(), is_alive, out);
                    if (a >= 0) next.push_back(i);
                    else if (a == LIVE_DEAD) alive[i] = 0, ++removed;
                }
                wl.swap(next);
                h.r.surviving -= removed;
                if (!removed) break;
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        // G': the states of F_p' (numbered by `pos`), their edges to other states of F_p', predecessors
        std::vector<u32> fs, pos(st.size(), NONE);
        for (u32 i = 0; i < (u32)st.size(); ++i)
            if (alive[i]) pos[i] = (u32)fs.size(), fs.push_back(i);
        const u32 nf = (u32)fs.size();
        struct Edge {
            u32 a, t;
        };
        std::vector<std::vector<Edge>> out_e(nf);
        std::vector<std::vector<u32>> preds(nf);
        std::vector<u64> me((size_t)nf * MW);
        std::vector<char> sink(nf, 0);
        for (u32 v = 0; v < nf; ++v) {
            live_moving<MOVES>(m, st[fs[v]].data(), &me[(size_t)v * MW], [&](int a, const u64* ns) {
                const u32 t = pos[find(ns)];
                if (t != NONE) out_e[v].push_back({(u32)a, t}), preds[t].push_back(v);
            });
            bool any = false;
            for (int w = 0; w < MW; ++w) any = any || me[(size_t)v * MW + w];
            sink[v] = !any;
        }
        // |U|: F_p' without its sinks, trimmed to the states with a successor in it
        {
            std::vector<char> in_u(nf);
            std::vector<u32> cnt(nf, 0), todo;
            for (u32 v = 0; v < nf; ++v) in_u[v] = !sink[v];
            for (u32 v = 0; v < nf; ++v) {
                for (const Edge& e : out_e[v]) cnt[v] += in_u[e.t];
                if (in_u[v] && !cnt[v]) todo.push_back(v);
            }
            while (!todo.empty()) {
                const u32 v = todo.back();
                todo.pop_back();
                in_u[v] = 0;
                for (u32 q : preds[v])
                    if (in_u[q] && --cnt[q] == 0) todo.push_back(q);
            }
            for (u32 v = 0; v < nf; ++v) wk.cyclic_states += in_u[v];
        }
        // Tarjan, iterative: comp[v] = the component's number for a component of two or more states
        std::vector<u32> comp(nf, NONE);
        std::vector<std::vector<u32>> members;
        {
            std::vector<u32> num(nf, NONE), low(nf, 0), stack, at(nf, 0);
            std::vector<char> on(nf, 0);
            std::vector<u32> call;
            u32 counter = 0;
            for (u32 root = 0; root < nf; ++root) {
                if (num[root] != NONE) continue;
                call.push_back(root);
                while (!call.empty()) {
                    const u32 v = call.back();
                    if (num[v] == NONE) num[v] = low[v] = counter++, stack.push_back(v), on[v] = 1;
                    bool down = false;
                    while (at[v] < out_e[v].size()) {
                        const u32 t = out_e[v][at[v]].t;
                        if (num[t] == NONE) {
                            call.push_back(t);
                            down = true;
                            break;
                        }
                        if (on[t]) low[v] = std::min(low[v], num[t]);
                        ++at[v];
                    }
                    if (down) continue;
                    call.pop_back();
                    if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[v]);
                    if (low[v] == num[v]) {
                        std::vector<u32> c;
                        for (;;) {
                            const u32 x = stack.back();
                            stack.pop_back();
                            on[x] = 0;
                            c.push_back(x);
                            if (x == v) break;
                        }
                        if (c.size() >= 2) {
                            for (u32 x : c) comp[x] = (u32)members.size();
                            members.push_back(std::move(c));
                        }
                    }
                }
            }
        }
        wk.components = members.size();
        std::vector<u64> and_me(members.size() * MW, ~0ull), or_took(members.size() * MW, 0);
        for (u32 v = 0; v < nf; ++v) {
            if (comp[v] == NONE) continue;
            for (int w = 0; w < MW; ++w) and_me[(size_t)comp[v] * MW + w] &= me[(size_t)v * MW + w];
            for (const Edge& e : out_e[v])
                if (comp[e.t] == comp[v]) or_took[(size_t)comp[v] * MW + (e.a >> 6)] |= 1ull << (e.a & 63);
        }
        std::vector<char> fair(members.size(), 0);
        for (size_t c = 0; c < members.size(); ++c) {
            fair[c] = live_fair_masks<MW>(&and_me[c * MW], &or_took[c * MW]);
            wk.fair_components += fair[c];
        }
        // breadth-first ranks towards `targets` over the predecessors inside a domain (dom(v))
        auto ranks_to = [&](const std::vector<u32>& targets, auto&& dom, std::vector<u32>& rank) -> u32 {
            std::vector<u32> level = targets, nxt;
            for (u32 v : targets) rank[v] = 0;
            u32 rounds = 0;
            for (u32 r = 1; !level.empty(); ++r, ++rounds) {
                nxt.clear();
                for (u32 t : level)
                    for (u32 q : preds[t])
                        if (dom(q) && rank[q] == NONE) rank[q] = r, nxt.push_back(q);
                level.swap(nxt);
            }
            return rounds;
        };
        std::vector<u32> rank(nf, NONE), goal;
        for (u32 v = 0; v < nf; ++v)
            if (sink[v] || (comp[v] != NONE && fair[comp[v]])) goal.push_back(v);
        wk.goal_states = goal.size();
        wk.reach_rounds += ranks_to(goal, [](u32) { return true; }, rank);
        for (u32 v = 0; v < nf; ++v) wk.fair_states += rank[v] != NONE;
        for (int i = 0; i < k && h.r.init_index < 0; ++i)
            if (alive[init_idx[i]] && rank[pos[init_idx[i]]] != NONE) h.r.init_index = i;
        if (h.r.init_index >= 0) {
            u64 notme[MW] = {}, taken[MW] = {};
            u32 cur = pos[init_idx[h.r.init_index]];
            h.words.assign(st[fs[cur]].begin(), st[fs[cur]].end());
            // follows the lowest rank-decreasing slot from cur to rank 0, then takes slot `then` (if >= 0)
            auto walk = [&](const std::vector<u32>& rk, int then, bool all) {
                u64 mk[MW], nx[W];
                auto step_to = [&](int a) {
                    h.actions.push_back(m.action_id(st[fs[cur]].data(), a));
                    cur = pos[find(nx)];
                    if (cur == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness leaves F_p'");
                    h.words.insert(h.words.end(), nx, nx + W);
                };
                for (;;) {
                    const u32 r = rk[cur];
                    if (r == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness is at a state without a rank");
                    const int a = live_descend_step<MOVES>(
                        m, st[fs[cur]].data(), r,
                        [&](const u64* ns) {
                            const u32 t = pos[find(ns)];
                            return t == NONE ? NONE : rk[t];
                        },
                        mk, nx);
                    if (all || !r)
                        for (int w = 0; w < MW; ++w) notme[w] |= ~mk[w];
                    if (!r) break;
                    if (a < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a ranked state has no successor of a lower rank");
                    if (all) taken[a >> 6] |= 1ull << (a & 63);
                    step_to(a);
                }
                if (then >= 0) {
                    if (!m.apply(st[fs[cur]].data(), then, nx)) throw Error(SR_ERR_NONDETERMINISM, "liveness: the slot to take is refused");
                    taken[then >> 6] |= 1ull << (then & 63);
                    step_to(then);
                    live_moving<MOVES>(m, st[fs[cur]].data(), mk, [](int, const u64*) {});
                    for (int w = 0; w < MW; ++w) notme[w] |= ~mk[w];
                }
            };
            walk(rank, -1, false);
            wk.stem_len = (int64_t)h.actions.size();
            const u32 g = cur;
            if (sink[g]) {
                u64 all = 0;
                for_each_successor(m, st[fs[g]].data(), [&](int, const u64*) { ++all; });
                h.r.end_kind = all ? SR_LIVE_END_STUTTER : SR_LIVE_END_TERMINAL;
                wk.loop_len = 0;
            } else {
                const u32 c = comp[g];
                if (c == NONE || !fair[c]) throw Error(SR_ERR_NONDETERMINISM, "liveness: the stem ends outside every fair component");
                std::vector<u32> lrank(nf, NONE), targets;
                auto in_c = [&](u32 v) { return comp[v] == c; };
                auto segment = [&](int then) {
                    for (u32 v : members[c]) lrank[v] = NONE;
                    wk.reach_rounds += ranks_to(targets, in_c, lrank);
                    wk.segments += 1;
                    walk(lrank, then, true);
                };
                for (int a = 0; a < m.max_actions(); ++a) {
                    const int plan = live_loop_plan(a, notme, taken, &and_me[(size_t)c * MW]);
                    if (plan == LIVE_PLAN_SKIP) continue;
                    targets.clear();
                    for (u32 v : members[c]) {
                        const bool mv = me[(size_t)v * MW + (a >> 6)] >> (a & 63) & 1;
                        bool hit = plan == LIVE_PLAN_NOTME && !mv;
                        if (plan == LIVE_PLAN_TAKE && mv)
                            for (const Edge& e : out_e[v]) hit = hit || ((int)e.a == a && comp[e.t] == c);
                        if (hit) targets.push_back(v);
                    }
                    segment(plan == LIVE_PLAN_TAKE ? a : -1);
                }
                targets.assign(1, g);
                segment(-1);
                h.r.end_kind = SR_LIVE_END_LOOP;
                h.r.loop_start = wk.stem_len;
                wk.loop_len = (int64_t)h.actions.size() - wk.stem_len;
                if (!live_loop_fair(m, &h.words[(size_t)wk.stem_len * W], (size_t)wk.loop_len))
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: the closed walk of the witness is not weakly fair");
            }
            h.r.witness_len = (int64_t)h.actions.size();
        }
        const auto t2 = std::chrono::steady_clock::now();
        h.r.pass_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
        wk.pass_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
        return res;
    }
}

// The check under STRONG FAIRNESS on the host, with no device, deliberately by another algorithm than the
// device's level-synchronous rounds: the host search and the progress fixpoint as live_host runs them, then
// the decomposition tree component by component (a work stack of vertex sets, Tarjan's algorithm on each),
// breadth-first ranks over predecessor lists, and the witness rule of the header. Only the per-state pieces
// (live_moving, live_strong_masks, live_descend_step, live_strong_plan) are the kernels'.
struct LiveHostStrong {
    LiveHost h;
    sr_live_strong s = live_strong_none();
};

template <bool MOVES = true, class M>
LiveHostStrong live_host_strong(const M& m, int p, u64 max_states) {
    constexpr int W = M::W, MW = M::MW;
    constexpr u32 NONE = ~0u;
    if constexpr (!fair_slots_model<M>) {
        throw Error(SR_ERR_UNSUPPORTED, "strong fairness: this model's slots are not fairness classes");
    } else {
        if (p < 0 || p >= M::NPROPS || m.expectation(p) != EVENTUALLY)
            throw Error(SR_ERR_ARG, "liveness: property " + std::to_string(p) + " is not an `eventually` property");
        struct H {
            size_t operator()(const std::vector<u64>& v) const {
                u64 h = 0;
                for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
                return (size_t)h;
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        std::unordered_map<std::vector<u64>, u32, H> index;
        std::vector<std::vector<u64>> st;
        auto add = [&](const u64* s) {
            std::vector<u64> v(s, s + W);
            auto it = index.find(v);
            if (it != index.end()) return it->second;
            if (st.size() >= max_states)
                throw Error(SR_ERR_CAPACITY, "liveness: the model has more than " + std::to_string(max_states) + " reachable states (max_states)");
            const u32 i = (u32)st.size();
            index.emplace(v, i);
            st.push_back(std::move(v));
            return i;
        };
        const std::vector<u64> inits = init_states_of(m);
        const int k = (int)(inits.size() / W);
        std::vector<u32> init_idx;
        for (int i = 0; i < k; ++i) init_idx.push_back(add(&inits[(size_t)i * W]));
        for (size_t q = 0; q < st.size(); ++q) {
            const std::vector<u64> s = st[q];  // (a copy: add() grows st)
            for_each_successor(m, s.data(), [&](int, const u64* ns) { add(ns); });
        }
        LiveHostStrong res;
        LiveHost& h = res.h;
        sr_live_strong& sg = res.s;
        h.unique = st.size();
        h.r.ran = sg.ran = 1;
        auto find = [&](const u64* ns) {
            auto it = index.find(std::vector<u64>(ns, ns + W));
            if (it == index.end()) throw Error(SR_ERR_NONDETERMINISM, "liveness: a successor of a reachable state is not in the reachable set");
            return it->second;
        };
        // the progress fixpoint, as live_host<true> runs it
        std::vector<char> alive(st.size(), 0);
        {
            std::vector<u32> wl, next;
            for (u32 i = 0; i < (u32)st.size(); ++i)
                if (live_not_p(m, p, st[i].data())) alive[i] = 1, wl.push_back(i);
            h.r.not_p_states = h.r.surviving = wl.size();
            auto is_alive = [&](const u64* ns) { return alive[find(ns)] != 0; };
            u64 out[W];
            for (;;) {
                u64 removed = 0;
                next.clear();
                h.r.rounds += 1;
                h.r.examined += wl.size();
                for (u32 i : wl) {
                    const int a = live_step<true, MOVES>(m, st[i].data(), is_alive, out);
                    if (a >= 0) next.push_back(i);
                    else if (a == LIVE_DEAD) alive[i] = 0, ++removed;
                }
                wl.swap(next);
                h.r.surviving -= removed;
                if (!removed) break;
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        // G': the states of F_p' (numbered by `pos`), their edges to other states of F_p', predecessors
        std::vector<u32> fs, pos(st.size(), NONE);
        for (u32 i = 0; i < (u32)st.size(); ++i)
            if (alive[i]) pos[i] = (u32)fs.size(), fs.push_back(i);
        const u32 nf = (u32)fs.size();
        struct Edge {
            u32 a, t;
        };
        std::vector<std::vector<Edge>> out_e(nf);
        std::vector<std::vector<u32>> preds(nf);
        std::vector<u64> me((size_t)nf * MW);
        std::vector<char> sink(nf, 0);
        for (u32 v = 0; v < nf; ++v) {
            live_moving<MOVES>(m, st[fs[v]].data(), &me[(size_t)v * MW], [&](int a, const u64* ns) {
                const u32 t = pos[find(ns)];
                if (t != NONE) out_e[v].push_back({(u32)a, t}), preds[t].push_back(v);
            });
            bool any = false;
            for (int w = 0; w < MW; ++w) any = any || me[(size_t)v * MW + w];
            sink[v] = !any;
        }
        // |U|: F_p' without its sinks, trimmed to the states with a successor in it
        {
            std::vector<char> in_u(nf);
            std::vector<u32> cnt(nf, 0), todo;
            for (u32 v = 0; v < nf; ++v) in_u[v] = !sink[v];
            for (u32 v = 0; v < nf; ++v) {
                for (const Edge& e : out_e[v]) cnt[v] += in_u[e.t];
                if (in_u[v] && !cnt[v]) todo.push_back(v);
            }
            while (!todo.empty()) {
                const u32 v = todo.back();
                todo.pop_back();
                in_u[v] = 0;
                for (u32 q : preds[v])
                    if (in_u[q] && --cnt[q] == 0) todo.push_back(q);
            }
            for (u32 v = 0; v < nf; ++v) sg.cyclic_states += in_u[v];
        }
        // The decomposition tree. A job is a vertex set X and its depth; in_x[v] == the job's number while
        // it runs. Tarjan (iterative) yields the components of G'[X]; a fair node keeps its number in node[v]
        // and its or_me mask, an unfair one puts X' on the stack.
        std::vector<u32> node(nf, NONE);
        std::vector<std::vector<u32>> members;  // per fair node
        std::vector<u64> node_or_me;            // per fair node, MW words
        {
            struct Job {
                std::vector<u32> x;
                u32 depth;
            };
            std::vector<Job> jobs;
            {
                Job all{{}, 1};
                for (u32 v = 0; v < nf; ++v) all.x.push_back(v);
                jobs.push_back(std::move(all));
            }
            std::vector<u32> in_x(nf, NONE), in_c(nf, NONE), num(nf), low(nf), at(nf), stack, call;
            std::vector<char> on(nf, 0);
            u32 job_no = 0, comp_no = 0;
            while (!jobs.empty()) {
                const Job job = std::move(jobs.back());
                jobs.pop_back();
                const u32 tag = job_no++;
                for (u32 v : job.x) in_x[v] = tag, num[v] = NONE, at[v] = 0;
                u32 counter = 0;
                for (u32 root : job.x) {
                    if (num[root] != NONE) continue;
                    call.push_back(root);
                    while (!call.empty()) {
                        const u32 v = call.back();
                        if (num[v] == NONE) num[v] = low[v] = counter++, stack.push_back(v), on[v] = 1;
                        bool down = false;
                        while (at[v] < out_e[v].size()) {
                            const u32 t = out_e[v][at[v]].t;
                            if (in_x[t] == tag) {
                                if (num[t] == NONE) {
                                    call.push_back(t);
                                    down = true;
                                    break;
                                }
                                if (on[t]) low[v] = std::min(low[v], num[t]);
                            }
                            ++at[v];
                        }
                        if (down) continue;
                        call.pop_back();
                        if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[v]);
                        if (low[v] != num[v]) continue;
                        std::vector<u32> c;
                        for (;;) {
                            const u32 x = stack.back();
                            stack.pop_back();
                            on[x] = 0;
                            c.push_back(x);
                            if (x == v) break;
                        }
                        if (c.size() < 2) continue;
                        sg.components += 1;
                        sg.levels = std::max(sg.levels, job.depth);
                        const u32 cn = comp_no++;
                        for (u32 x : c) in_c[x] = cn;
                        u64 or_me[MW] = {}, or_took[MW] = {};
                        for (u32 x : c) {
                            for (int w = 0; w < MW; ++w) or_me[w] |= me[(size_t)x * MW + w];
                            for (const Edge& e : out_e[x])
                                if (in_c[e.t] == cn) or_took[e.a >> 6] |= 1ull << (e.a & 63);
                        }
                        if (live_strong_masks<MW>(or_me, or_took)) {
                            for (u32 x : c) node[x] = (u32)members.size();
                            members.push_back(std::move(c));
                            node_or_me.insert(node_or_me.end(), or_me, or_me + MW);
                            sg.fair_components += 1;
                            continue;
                        }
                        Job sub{{}, job.depth + 1};
                        for (u32 x : c) {
                            bool hit = false;
                            for (int w = 0; w < MW; ++w) hit = hit || (me[(size_t)x * MW + w] & or_me[w] & ~or_took[w]);
                            if (!hit) sub.x.push_back(x);
                        }
                        if (sub.x.size() >= c.size()) throw Error(SR_ERR_NONDETERMINISM, "liveness: an unfair component loses no state");
                        if (sub.x.size() >= 2) jobs.push_back(std::move(sub));
                    }
                }
            }
        }
        // breadth-first ranks towards `targets` over the predecessors inside a domain (dom(v))
        auto ranks_to = [&](const std::vector<u32>& targets, auto&& dom, std::vector<u32>& rank) -> u32 {
            std::vector<u32> level = targets, nxt;
            for (u32 v : targets) rank[v] = 0;
            u32 rounds = 0;
            for (u32 r = 1; !level.empty(); ++r, ++rounds) {
                nxt.clear();
                for (u32 t : level)
                    for (u32 q : preds[t])
                        if (dom(q) && rank[q] == NONE) rank[q] = r, nxt.push_back(q);
                level.swap(nxt);
            }
            return rounds;
        };
        std::vector<u32> rank(nf, NONE), goal;
        for (u32 v = 0; v < nf; ++v)
            if (sink[v] || node[v] != NONE) goal.push_back(v);
        sg.goal_states = goal.size();
        sg.reach_rounds += ranks_to(goal, [](u32) { return true; }, rank);
        for (u32 v = 0; v < nf; ++v) sg.fair_states += rank[v] != NONE;
        for (int i = 0; i < k && h.r.init_index < 0; ++i)
            if (alive[init_idx[i]] && rank[pos[init_idx[i]]] != NONE) h.r.init_index = i;
        if (h.r.init_index >= 0) {
            u64 taken[MW] = {};
            u32 cur = pos[init_idx[h.r.init_index]];
            h.words.assign(st[fs[cur]].begin(), st[fs[cur]].end());
            // follows the lowest rank-lowering slot from cur to rank 0, then takes slot `then` (if >= 0)
            auto walk = [&](const std::vector<u32>& rk, int then, bool loop) {
                u64 mk[MW], nx[W];
                auto step_to = [&](int a) {
                    h.actions.push_back(m.action_id(st[fs[cur]].data(), a));
                    if (loop) taken[a >> 6] |= 1ull << (a & 63);
                    cur = pos[find(nx)];
                    if (cur == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness leaves F_p'");
                    h.words.insert(h.words.end(), nx, nx + W);
                };
                for (;;) {
                    const u32 r = rk[cur];
                    if (r == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness is at a state without a rank");
                    if (!r) break;
                    const int a = live_descend_step<MOVES>(
                        m, st[fs[cur]].data(), r,
                        [&](const u64* ns) {
                            const u32 t = pos[find(ns)];
                            return t == NONE ? NONE : rk[t];
                        },
                        mk, nx);
                    if (a < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a ranked state has no successor of a lower rank");
                    step_to(a);
                }
                if (then >= 0) {
                    if (!m.apply(st[fs[cur]].data(), then, nx)) throw Error(SR_ERR_NONDETERMINISM, "liveness: the slot to take is refused");
                    step_to(then);
                }
            };
            walk(rank, -1, false);
            sg.stem_len = (int64_t)h.actions.size();
            const u32 g = cur;
            if (sink[g]) {
                u64 all = 0;
                for_each_successor(m, st[fs[g]].data(), [&](int, const u64*) { ++all; });
                h.r.end_kind = all ? SR_LIVE_END_STUTTER : SR_LIVE_END_TERMINAL;
                sg.loop_len = 0;
            } else {
                const u32 c = node[g];
                if (c == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the stem ends outside every fair node");
                std::vector<u32> lrank(nf, NONE), targets;
                auto in_c = [&](u32 v) { return node[v] == c; };
                auto segment = [&](int then) {
                    for (u32 v : members[c]) lrank[v] = NONE;
                    sg.reach_rounds += ranks_to(targets, in_c, lrank);
                    sg.segments += 1;
                    walk(lrank, then, true);
                };
                for (int a = 0; a < m.max_actions(); ++a) {
                    if (live_strong_plan(a, taken, &node_or_me[(size_t)c * MW]) == LIVE_PLAN_SKIP) continue;
                    targets.clear();
                    for (u32 v : members[c])
                        for (const Edge& e : out_e[v])
                            if ((int)e.a == a && node[e.t] == c) {
                                targets.push_back(v);
                                break;
                            }
                    segment(a);
                }
                targets.assign(1, g);
                segment(-1);
                h.r.end_kind = SR_LIVE_END_LOOP;
                h.r.loop_start = sg.stem_len;
                sg.loop_len = (int64_t)h.actions.size() - sg.stem_len;
                if (!live_loop_strong_fair(m, &h.words[(size_t)sg.stem_len * W], (size_t)sg.loop_len))
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: the closed walk of the witness is not strongly fair");
            }
            h.r.witness_len = (int64_t)h.actions.size();
        }
        const auto t2 = std::chrono::steady_clock::now();
        h.r.pass_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
        sg.pass_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
        return res;
    }
}

}  // namespace sr
