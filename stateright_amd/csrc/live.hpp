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
// LEADS-TO (a property kind of its own: `expectation(p) == LEADS_TO`, models.hpp has_lmask; TLA+'s P ~> Q, and
// []<>Q where the trigger is true). `discovers(p, .)` is the TARGET condition Q, `leads_from(p, .)` the TRIGGER
// P. For a leads-to property p in mode m (any of the four above):
//   X_Q        the mode's set for the condition Q, exactly as defined above: F_p, F_p' or FairF, the reachable
//              states from which a (fair) maximal run exists on which Q never holds. X_Q is a subset of N_p, so
//              a state where Q holds is never in it;
//   triggered  |{ s in R : P(s) }|;   pending  |{ s in R : P(s) and not Q(s) }|;
//   violating  |{ s in R : P(s) and s in X_Q }| (a state counts once, however many runs from it avoid Q).
// p has a counterexample iff violating > 0; triggered == 0 is reported as vacuous. Where `eventually` asks
// "is some INIT state in X_Q", leads-to asks "is some REACHABLE state where P holds in X_Q": everything
// before that question (mark, trim, components, ranks) is the `eventually` pass unchanged.
//   SEED      depth(s) is the breadth-first distance of s from the init states (its level in the search). The
//             seed is the violating state of lowest depth, among those the lowest compared word by word from
//             word 0, unsigned (live_leads_less). Never the arena index: in FAST order it differs from run to
//             run, and the seed must not.
//   WITNESS   prefix ++ suffix. The suffix is the mode's witness above started at the seed in place of an
//             init state (live_walk, or the stem and the closed walk). The prefix is the search's own tree
//             path from an init state to the seed: depth(seed) steps; Q may hold on it; the unique reference-
//             order path in FIFO order, some shortest path in FAST order. trigger_index = depth(seed) is the
//             seed's index on the path; loop_start is an index into the whole path and >= trigger_index; a
//             fair mode's stem_len counts from the seed. init_index is the lowest index of an init state
//             equal to the path's first state.
//   ACCEPTANCE  (host, Engine::live_accept / live_accept_loop / live_replay with the offset trigger_index):
//             every step of the whole path is a successor in `actions()` order; P holds at trigger_index; Q
//             holds on no state from trigger_index on; the terminal, stutter-end, loop-equality and loop-
//             fairness checks apply to the suffix; a loop that closes on a prefix state is an engine error.
// One seed only: the other violating states are counted, not witnessed. The witness is not the shortest
// beyond its prefix.
//
// The per-state rule and the witness step are ONE function, live_step below, which the kernels
// (kernels_live.hpp: live_trim, live_walk) and the host form (live_host, the sr_liveness_host entry
// point) instantiate; they differ only in how "is this successor in the set" is answered (the alive
// bitmap by visited-set slot on the device, a hash map on the host).
//
// This file, in order: the per-state pieces shared with the kernels (live_step; for the fair modes live_moving,
// live_descend_step, the *_masks and *_plan functions and the two loop-fairness checks); then, behind the
// kernels' header, the host forms: LiveHostSet, live_host_fixpoint and live_host (plain and progress),
// LiveHostGraph and live_host_fair_witness (what the weak and the strong form share), and live_host_weak and
// live_host_strong, which hold their mode's decomposition only. The device's driver is in engine.hpp (live_pass,
// LiveFair, live_weak_pass, live_strong_pass).
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

// ---- leads-to: the rule's per-state pieces, shared by the kernels (live_leads_scan, live_leads_min) and the
// host form (LiveLeadsStart) ----

// The trigger of property p at s (false for a model without leads-to properties).
template <class M>
SR_HD bool live_leads_from(const M& m, int p, const u64* s) {
    if constexpr (has_lmask<M>::value) return m.leads_from(p, s);
    else return false;
}

// What a state adds to the three counts: bit 0 triggered, bit 1 pending, bit 2 violating. in_x: s is in X_Q.
enum LiveLeadsBits : u32 { LIVE_LEADS_TRIGGERED = 1, LIVE_LEADS_PENDING = 2, LIVE_LEADS_VIOLATING = 4 };
template <class M, class InX>
SR_HD u32 live_leads_class(const M& m, int p, const u64* s, InX&& in_x) {
    if (!live_leads_from(m, p, s)) return 0;
    if (!live_not_p(m, p, s)) return LIVE_LEADS_TRIGGERED;
    return LIVE_LEADS_TRIGGERED | LIVE_LEADS_PENDING | (in_x() ? (u32)LIVE_LEADS_VIOLATING : 0u);
}

// The seed's tie-break among violating states of one depth: a before b iff a is lower word by word from
// word 0, unsigned.
template <int W>
SR_HD bool live_leads_less(const u64* a, const u64* b) {
#pragma unroll
    for (int i = 0; i < W; ++i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
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

// sr_live_weak and sr_live_strong name their fields alike (but reserved0 / levels), so what fills them is
// written once, over the type.
template <class Stats>
Stats live_fair_none() {
    Stats s;
    std::memset(&s, 0, sizeof(s));
    s.stem_len = s.loop_len = -1;
    return s;
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

// ---- The check on the host, with no device (the sr_liveness_host* entry points). The three forms are built
// from pieces that are each written once: the reachable set (LiveHostSet), the fixpoint (live_host_fixpoint),
// and for the weak and the strong form the graph G' with its |U| count, Tarjan's algorithm and breadth-first
// ranks (LiveHostGraph) and the witness (live_host_fair_witness: the stem, the sink ending, the closed walk).
// The fair forms deliberately run other algorithms than the device's (Tarjan and predecessor lists against
// colouring rounds); only the per-state pieces above (live_step, live_moving, live_descend_step, the *_masks
// and *_plan functions) are the kernels'.

struct LiveHost {
    sr_live_result r = live_result_none();
    u64 unique = 0;
    std::vector<u64> words;    // the witness' states, W words each (empty: no init state in F_p)
    std::vector<i64> actions;  // its canonical action ids, one per step
};

template <class Stats>  // sr_live_weak or sr_live_strong
struct LiveHostFair {
    LiveHost h;
    Stats s = live_fair_none<Stats>();
};

// The reachable set: a search over at most max_states states, which numbers them in the order it finds
// them. Refuses a p that is no `eventually` property (leads: no leads-to property). tree() gives every
// state's depth and its parent in the reference's FIFO order, for the prefix of a leads-to witness.
template <class M>
struct LiveHostSet {
    static constexpr int W = M::W;
    struct H {
        size_t operator()(const std::vector<u64>& v) const {
            u64 h = 0;
            for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
            return (size_t)h;
        }
    };
    const M& m;
    const u64 max_states;
    std::unordered_map<std::vector<u64>, u32, H> index;
    std::vector<std::vector<u64>> st;
    std::vector<u32> init_idx;  // the init states' numbers, in the order of `init_states`

    LiveHostSet(const M& m_, int p, u64 max_states_, bool leads = false) : m(m_), max_states(max_states_) {
        if (p < 0 || p >= M::NPROPS || m.expectation(p) != (leads ? LEADS_TO : EVENTUALLY))
            throw Error(SR_ERR_ARG, "liveness: property " + std::to_string(p) + (leads ? " is not a leads-to property" : " is not an `eventually` property"));
        const std::vector<u64> inits = init_states_of(m);
        for (size_t i = 0; i < inits.size() / W; ++i) init_idx.push_back(add(&inits[i * W]));
        for (size_t q = 0; q < st.size(); ++q) {
            const std::vector<u64> s = st[q];  // (a copy: add() grows st)
            for_each_successor(m, s.data(), [&](int, const u64* ns) { add(ns); });
        }
    }
    u32 add(const u64* s) {
        std::vector<u64> v(s, s + W);
        auto it = index.find(v);
        if (it != index.end()) return it->second;
        if (st.size() >= max_states)
            throw Error(SR_ERR_CAPACITY, "liveness: the model has more than " + std::to_string(max_states) + " reachable states (max_states)");
        const u32 i = (u32)st.size();
        index.emplace(v, i);
        st.push_back(std::move(v));
        return i;
    }
    u32 find(const u64* ns) const {
        auto it = index.find(std::vector<u64>(ns, ns + W));
        if (it == index.end()) throw Error(SR_ERR_NONDETERMINISM, "liveness: a successor of a reachable state is not in the reachable set");
        return it->second;
    }
    // The search tree of the reference's single-threaded FIFO order (bfs.rs: pop_back / push_front): level 0 is
    // popped in REVERSE init order, a popped state's successors are queued in `actions()` order, and the first
    // state to generate t is its parent. depth[t] is t's breadth-first distance; parent ~0 for level 0.
    void tree(std::vector<u32>& depth, std::vector<u32>& parent) const {
        depth.assign(st.size(), ~0u);
        parent.assign(st.size(), ~0u);
        std::vector<u32> q;
        for (size_t i = init_idx.size(); i-- > 0;)
            if (depth[init_idx[i]] == ~0u) depth[init_idx[i]] = 0, q.push_back(init_idx[i]);
        for (size_t head = 0; head < q.size(); ++head) {
            const u32 v = q[head];
            for_each_successor(m, st[v].data(), [&](int, const u64* ns) {
                const u32 t = find(ns);
                if (depth[t] == ~0u) depth[t] = depth[v] + 1, parent[t] = v, q.push_back(t);
            });
        }
    }
};

// Where a host form's witness starts: start(R, in, h) returns the number of its first state in R (~0: there is
// none, the property holds), having put what precedes that state (nothing, or a leads-to prefix: its states
// but the last, and its actions) into h.words and h.actions and set h.r.init_index; in(i) says whether state
// i is in the mode's set X. The default: the init state of lowest index in X.
struct LiveInitStart {
    static constexpr bool leads = false;
    template <class M, class In>
    u32 operator()(const LiveHostSet<M>& R, In&& in, LiveHost& h) const {
        for (size_t i = 0; i < R.init_idx.size(); ++i)
            if (in(R.init_idx[i])) {
                h.r.init_index = (int32_t)i;
                return R.init_idx[i];
            }
        return ~0u;
    }
};

// The start of a leads-to property's witness (the header's LEADS-TO rule): the three counts over R, the seed,
// and the FIFO tree path to it as the prefix.
struct LiveLeadsStart {
    static constexpr bool leads = true;
    int p;
    sr_live_leads& L;
    template <class M, class In>
    u32 operator()(const LiveHostSet<M>& R, In&& in, LiveHost& h) const {
        constexpr int W = M::W;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<u32> depth, parent;
        R.tree(depth, parent);
        u32 seed = ~0u;
        for (u32 i = 0; i < (u32)R.st.size(); ++i) {
            const u32 c = live_leads_class(R.m, p, R.st[i].data(), [&] { return in(i); });
            L.triggered += c & LIVE_LEADS_TRIGGERED ? 1 : 0;
            L.pending += c & LIVE_LEADS_PENDING ? 1 : 0;
            if (!(c & LIVE_LEADS_VIOLATING)) continue;
            L.violating += 1;
            if (seed == ~0u || depth[i] < depth[seed] || (depth[i] == depth[seed] && live_leads_less<W>(R.st[i].data(), R.st[seed].data())))
                seed = i;
        }
        L.ran = 1;
        if (seed != ~0u) {
            std::vector<u32> chain;
            for (u32 v = seed; v != ~0u; v = parent[v]) chain.push_back(v);
            std::reverse(chain.begin(), chain.end());
            for (size_t i = 0; i < R.init_idx.size() && h.r.init_index < 0; ++i)
                if (R.init_idx[i] == chain[0]) h.r.init_index = (int32_t)i;
            for (size_t k = 0; k + 1 < chain.size(); ++k) {
                const std::vector<u64>& s = R.st[chain[k]];
                h.words.insert(h.words.end(), s.begin(), s.end());
                i64 id = -1;
                for_each_successor(R.m, s.data(), [&](int a, const u64* ns) {
                    if (id < 0 && std::equal(ns, ns + W, R.st[chain[k + 1]].data())) id = R.m.action_id(s.data(), a);
                });
                if (id < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a tree edge of the prefix is no step of the model");
                h.actions.push_back(id);
            }
            L.trigger_index = L.trigger_depth = (int64_t)chain.size() - 1;
        }
        L.seed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return seed;
    }
};

inline sr_live_leads live_leads_none() {
    sr_live_leads l;
    std::memset(&l, 0, sizeof(l));
    l.trigger_index = l.trigger_depth = -1;
    return l;
}

// The fixpoint over R (in place, worklist by worklist as the device runs it): fills r's counters and returns
// the alive vector, F_p (FAIR: F_p'). FAIR: progress fairness; MOVES: see live_step.
template <bool FAIR, bool MOVES, class M>
std::vector<char> live_host_fixpoint(const LiveHostSet<M>& R, int p, sr_live_result& r) {
    std::vector<char> alive(R.st.size(), 0);
    std::vector<u32> wl, next;
    for (u32 i = 0; i < (u32)R.st.size(); ++i)
        if (live_not_p(R.m, p, R.st[i].data())) alive[i] = 1, wl.push_back(i);
    r.not_p_states = r.surviving = wl.size();
    auto is_alive = [&](const u64* ns) { return alive[R.find(ns)] != 0; };
    u64 out[M::W];
    for (;;) {
        u64 removed = 0;
        next.clear();
        r.rounds += 1;
        r.examined += wl.size();
        for (u32 i : wl) {
            const int a = live_step<FAIR, MOVES>(R.m, R.st[i].data(), is_alive, out);
            if (a >= 0) next.push_back(i);
            else if (a == LIVE_DEAD) alive[i] = 0, ++removed;
        }
        wl.swap(next);
        r.surviving -= removed;
        if (!removed) break;
    }
    return alive;
}

// The plain and the progress form: the reachable set, the fixpoint and the witness from where `start` says
// (LiveInitStart: an `eventually` property; LiveLeadsStart: a leads-to property, behind its prefix).
template <bool FAIR = false, bool MOVES = true, class M, class Start = LiveInitStart>
LiveHost live_host(const M& m, int p, u64 max_states, const Start& start = Start{}) {
    constexpr int W = M::W;
    const auto t0 = std::chrono::steady_clock::now();
    const LiveHostSet<M> R(m, p, max_states, Start::leads);
    LiveHost h;
    h.unique = R.st.size();
    h.r.ran = 1;
    const std::vector<char> alive = live_host_fixpoint<FAIR, MOVES>(R, p, h.r);
    u32 cur = start(R, [&](u32 i) { return alive[i] != 0; }, h);
    if (cur != ~0u) {
        auto is_alive = [&](const u64* ns) { return alive[R.find(ns)] != 0; };
        std::unordered_map<u32, i64> at;  // state -> its position on the path (from the start on)
        u64 out[W];
        for (i64 t = (i64)h.actions.size();; ++t) {
            h.words.insert(h.words.end(), R.st[cur].begin(), R.st[cur].end());
            auto seen = at.find(cur);
            if (seen != at.end()) {
                h.r.witness_len = t;
                h.r.loop_start = seen->second;
                h.r.end_kind = SR_LIVE_END_LOOP;
                break;
            }
            at.emplace(cur, t);
            const int a = live_step<FAIR, MOVES>(m, R.st[cur].data(), is_alive, out);
            if (a == LIVE_TERMINAL || a == LIVE_STUTTER) {
                h.r.witness_len = t;
                h.r.end_kind = a == LIVE_TERMINAL ? SR_LIVE_END_TERMINAL : SR_LIVE_END_STUTTER;
                break;
            }
            if (a < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a state of the fixpoint has no successor in it");
            h.actions.push_back(m.action_id(R.st[cur].data(), a));
            cur = R.find(out);
        }
    }
    h.r.pass_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return h;
}

// G': the states of F_p' (numbered by `pos`), their succ' edges to other states of F_p', the predecessors, the
// me masks and the sinks; with what both fair forms run on it.
template <bool MOVES, class M>
struct LiveHostGraph {
    static constexpr int MW = M::MW;
    static constexpr u32 NONE = ~0u;
    struct Edge {
        u32 a, t;
    };
    const LiveHostSet<M>& R;
    std::vector<u32> fs, pos;
    u32 nf = 0;
    std::vector<std::vector<Edge>> out_e;
    std::vector<std::vector<u32>> preds;
    std::vector<u64> me;  // MW words per state
    std::vector<char> sink;

    LiveHostGraph(const LiveHostSet<M>& R_, const std::vector<char>& alive) : R(R_), pos(R_.st.size(), NONE) {
        for (u32 i = 0; i < (u32)R.st.size(); ++i)
            if (alive[i]) pos[i] = (u32)fs.size(), fs.push_back(i);
        nf = (u32)fs.size();
        out_e.resize(nf), preds.resize(nf), me.resize((size_t)nf * MW), sink.assign(nf, 0);
        num.resize(nf), low.resize(nf), next_e.resize(nf), on.assign(nf, 0);
        for (u32 v = 0; v < nf; ++v) {
            live_moving<MOVES>(R.m, state(v), &me[(size_t)v * MW], [&](int a, const u64* ns) {
                const u32 t = at(ns);
                if (t != NONE) out_e[v].push_back({(u32)a, t}), preds[t].push_back(v);
            });
            bool any = false;
            for (int w = 0; w < MW; ++w) any = any || me[(size_t)v * MW + w];
            sink[v] = !any;
        }
    }
    const u64* state(u32 v) const { return R.st[fs[v]].data(); }
    u32 at(const u64* ns) const { return pos[R.find(ns)]; }  // (NONE: a reachable state outside F_p')
    bool moving(u32 v, int a) const { return me[(size_t)v * MW + (a >> 6)] >> (a & 63) & 1; }

    // |U|: F_p' without its sinks, trimmed to the states with a successor in it
    u64 cyclic_states() const {
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
        u64 n = 0;
        for (u32 v = 0; v < nf; ++v) n += in_u[v];
        return n;
    }

    // Tarjan, iterative, on G'[X]: X the vertices `verts` (roots are tried in that order), in(t) whether t is
    // in X. Every component of two or more states goes to f(c) (c may be moved from), in the order found.
    template <class In, class F>
    void components(const std::vector<u32>& verts, In&& in, F&& f) {
        for (u32 v : verts) num[v] = NONE, next_e[v] = 0;
        u32 counter = 0;
        for (u32 root : verts) {
            if (num[root] != NONE) continue;
            call.push_back(root);
            while (!call.empty()) {
                const u32 v = call.back();
                if (num[v] == NONE) num[v] = low[v] = counter++, stack.push_back(v), on[v] = 1;
                bool down = false;
                while (next_e[v] < out_e[v].size()) {
                    const u32 t = out_e[v][next_e[v]].t;
                    if (in(t)) {
                        if (num[t] == NONE) {
                            call.push_back(t);
                            down = true;
                            break;
                        }
                        if (on[t]) low[v] = std::min(low[v], num[t]);
                    }
                    ++next_e[v];
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
                if (c.size() >= 2) f(c);
            }
        }
    }

    // breadth-first ranks towards `targets` over the predecessors inside a domain (dom(v)); the levels it took
    template <class Dom>
    u32 ranks_to(const std::vector<u32>& targets, Dom&& dom, std::vector<u32>& rank) const {
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
    }

private:
    std::vector<u32> num, low, next_e, stack, call;  // Tarjan's scratch, kept across calls
    std::vector<char> on;
};

// What differs between the two fair forms' witnesses: how the closed walk plans slot a from the loop's masks
// so far and the component's accumulator (and_me of a fair component, or_me of a fair node), whether the
// walk records notme at all, and the fairness the finished loop is checked for.
struct LiveWeakWalk {
    static constexpr bool NOTME = true;
    static constexpr const char* NAME = "weak fairness";
    static constexpr const char* FAIR = "weakly";
    static int plan(int a, const u64* notme, const u64* taken, const u64* and_me) { return live_loop_plan(a, notme, taken, and_me); }
    template <class M>
    static bool loop_fair(const M& m, const u64* states, size_t len) {
        return live_loop_fair(m, states, len);
    }
};
struct LiveStrongWalk {
    static constexpr bool NOTME = false;
    static constexpr const char* NAME = "strong fairness";
    static constexpr const char* FAIR = "strongly";
    static int plan(int a, const u64*, const u64* taken, const u64* or_me) { return live_strong_plan(a, taken, or_me); }
    template <class M>
    static bool loop_fair(const M& m, const u64* states, size_t len) {
        return live_loop_strong_fair(m, states, len);
    }
};

// The goal set, FairF and the witness rule of the header, given the decomposition: node[v] the fair component
// (fair node) of v or NONE, members and masks (MW words: Walk::plan's accumulator) by that number. The stem,
// then the sink ending, or the closed walk inside g's component: per slot the plan, the target set (NOTME: the
// members with !me(., a); TAKE: those whose a-step stays inside), ranks towards it inside the component, the
// walk; then home to g.
// The witness starts where `start` says (LiveInitStart, or LiveLeadsStart behind its prefix of `off` steps: stem_len
// counts from there, loop_start is an index into the whole path).
template <class Walk, bool MOVES, class M, class Stats, class Start>
void live_host_fair_witness(const LiveHostGraph<MOVES, M>& G, const std::vector<u32>& node, const std::vector<std::vector<u32>>& members,
                            const std::vector<u64>& masks, LiveHost& h, Stats& s, const Start& start) {
    constexpr int W = M::W, MW = M::MW;
    constexpr u32 NONE = ~0u;
    const M& m = G.R.m;
    std::vector<u32> rank(G.nf, NONE), goal;
    for (u32 v = 0; v < G.nf; ++v)
        if (G.sink[v] || node[v] != NONE) goal.push_back(v);
    s.goal_states = goal.size();
    s.reach_rounds += G.ranks_to(goal, [](u32) { return true; }, rank);
    for (u32 v = 0; v < G.nf; ++v) s.fair_states += rank[v] != NONE;
    const u32 first = start(G.R, [&](u32 i) { return G.pos[i] != NONE && rank[G.pos[i]] != NONE; }, h);
    if (first == NONE) return;
    const int64_t off = (int64_t)h.actions.size();
    u64 notme[MW] = {}, taken[MW] = {}, mk[MW], nx[W];
    u32 cur = G.pos[first];
    h.words.insert(h.words.end(), G.state(cur), G.state(cur) + W);
    auto step_to = [&](int a, bool loop) {  // the step by slot a, whose successor is in nx
        h.actions.push_back(m.action_id(G.state(cur), a));
        if (loop) taken[a >> 6] |= 1ull << (a & 63);
        cur = G.at(nx);
        if (cur == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness leaves F_p'");
        h.words.insert(h.words.end(), nx, nx + W);
    };
    // follows the lowest rank-lowering slot from cur to rank 0, then takes slot `then` (if >= 0). loop (a segment
    // of the closed walk, not the stem): the steps count as taken, and with Walk::NOTME every state passed adds
    // to notme; the stem adds only its last state, g.
    auto walk = [&](const std::vector<u32>& rk, int then, bool loop) {
        for (;;) {
            const u32 r = rk[cur];
            if (r == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness is at a state without a rank");
            if (!r && !Walk::NOTME) break;
            const int a = live_descend_step<MOVES>(
                m, G.state(cur), r,
                [&](const u64* ns) {
                    const u32 t = G.at(ns);
                    return t == NONE ? NONE : rk[t];
                },
                mk, nx);
            if (Walk::NOTME && (loop || !r))
                for (int w = 0; w < MW; ++w) notme[w] |= ~mk[w];
            if (!r) break;
            if (a < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: a ranked state has no successor of a lower rank");
            step_to(a, loop);
        }
        if (then >= 0) {
            if (!m.apply(G.state(cur), then, nx)) throw Error(SR_ERR_NONDETERMINISM, "liveness: the slot to take is refused");
            step_to(then, true);
            if (Walk::NOTME) {
                live_moving<MOVES>(m, G.state(cur), mk, [](int, const u64*) {});
                for (int w = 0; w < MW; ++w) notme[w] |= ~mk[w];
            }
        }
    };
    walk(rank, -1, false);
    s.stem_len = (int64_t)h.actions.size() - off;
    const u32 g = cur;
    if (G.sink[g]) {
        u64 all = 0;
        for_each_successor(m, G.state(g), [&](int, const u64*) { ++all; });
        h.r.end_kind = all ? SR_LIVE_END_STUTTER : SR_LIVE_END_TERMINAL;
        s.loop_len = 0;
    } else {
        const u32 c = node[g];
        if (c == NONE) throw Error(SR_ERR_NONDETERMINISM, "liveness: the stem ends outside every fair component");
        std::vector<u32> lrank(G.nf, NONE), targets;
        auto segment = [&](int then) {
            for (u32 v : members[c]) lrank[v] = NONE;
            s.reach_rounds += G.ranks_to(targets, [&](u32 v) { return node[v] == c; }, lrank);
            s.segments += 1;
            walk(lrank, then, true);
        };
        for (int a = 0; a < m.max_actions(); ++a) {
            const int plan = Walk::plan(a, notme, taken, &masks[(size_t)c * MW]);
            if (plan == LIVE_PLAN_SKIP) continue;
            targets.clear();
            for (u32 v : members[c]) {
                bool hit = plan == LIVE_PLAN_NOTME && !G.moving(v, a);
                if (plan == LIVE_PLAN_TAKE && G.moving(v, a))
                    for (const auto& e : G.out_e[v]) hit = hit || ((int)e.a == a && node[e.t] == c);
                if (hit) targets.push_back(v);
            }
            segment(plan == LIVE_PLAN_TAKE ? a : -1);
        }
        targets.assign(1, g);
        segment(-1);
        h.r.end_kind = SR_LIVE_END_LOOP;
        h.r.loop_start = off + s.stem_len;
        s.loop_len = (int64_t)h.actions.size() - off - s.stem_len;
        if (!Walk::loop_fair(m, &h.words[(size_t)(off + s.stem_len) * W], (size_t)s.loop_len))
            throw Error(SR_ERR_NONDETERMINISM, std::string("liveness: the closed walk of the witness is not ") + Walk::FAIR + " fair");
    }
    h.r.witness_len = (int64_t)h.actions.size();
}

// A fair form: the host search and the progress fixpoint as live_host<true> runs them, G' and |U|, the mode's
// decomposition (decompose(G, s, node, members, masks): see live_host_fair_witness), the witness, the times.
template <class Walk, class Stats, bool MOVES, class M, class Decompose, class Start>
LiveHostFair<Stats> live_host_fair(const M& m, int p, u64 max_states, Decompose&& decompose, const Start& start) {
    if constexpr (!fair_slots_model<M>) {
        throw Error(SR_ERR_UNSUPPORTED, std::string(Walk::NAME) + ": this model's slots are not fairness classes");
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        const LiveHostSet<M> R(m, p, max_states, Start::leads);
        LiveHostFair<Stats> res;
        res.h.unique = R.st.size();
        res.h.r.ran = res.s.ran = 1;
        const std::vector<char> alive = live_host_fixpoint<true, MOVES>(R, p, res.h.r);
        const auto t1 = std::chrono::steady_clock::now();
        LiveHostGraph<MOVES, M> G(R, alive);
        res.s.cyclic_states = G.cyclic_states();
        std::vector<u32> node(G.nf, ~0u);
        std::vector<std::vector<u32>> members;
        std::vector<u64> masks;
        decompose(G, res.s, node, members, masks);
        live_host_fair_witness<Walk>(G, node, members, masks, res.h, res.s, start);
        const auto t2 = std::chrono::steady_clock::now();
        res.h.r.pass_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
        res.s.pass_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
        return res;
    }
}

// WEAK FAIRNESS on the host: the maximal components of G' (one Tarjan over everything), their and_me and
// or_took accumulators and live_fair_masks; the fair ones are the witness' components.
template <bool MOVES = true, class M, class Start = LiveInitStart>
LiveHostFair<sr_live_weak> live_host_weak(const M& m, int p, u64 max_states, const Start& start = Start{}) {
    return live_host_fair<LiveWeakWalk, sr_live_weak, MOVES>(
        m, p, max_states, [](auto& G, sr_live_weak& wk, std::vector<u32>& node, std::vector<std::vector<u32>>& members, std::vector<u64>& and_me) {
            constexpr int MW = M::MW;
            constexpr u32 NONE = ~0u;
            std::vector<u32> all(G.nf), comp(G.nf, NONE);
            for (u32 v = 0; v < G.nf; ++v) all[v] = v;
            G.components(all, [](u32) { return true; }, [&](std::vector<u32>& c) {
                for (u32 x : c) comp[x] = (u32)members.size();
                members.push_back(std::move(c));
            });
            wk.components = members.size();
            and_me.assign(members.size() * MW, ~0ull);
            std::vector<u64> or_took(members.size() * MW, 0);
            for (u32 v = 0; v < G.nf; ++v) {
                if (comp[v] == NONE) continue;
                for (int w = 0; w < MW; ++w) and_me[(size_t)comp[v] * MW + w] &= G.me[(size_t)v * MW + w];
                for (const auto& e : G.out_e[v])
                    if (comp[e.t] == comp[v]) or_took[(size_t)comp[v] * MW + (e.a >> 6)] |= 1ull << (e.a & 63);
            }
            std::vector<char> fair(members.size(), 0);
            for (size_t c = 0; c < members.size(); ++c) {
                fair[c] = live_fair_masks<MW>(&and_me[c * MW], &or_took[c * MW]);
                wk.fair_components += fair[c];
            }
            for (u32 v = 0; v < G.nf; ++v)
                if (comp[v] != NONE && fair[comp[v]]) node[v] = comp[v];
        }, start);
}

// STRONG FAIRNESS on the host: the decomposition tree component by component. A job is a vertex set X and its
// depth; in_x[v] == the job's number while it runs. Tarjan yields the components of G'[X]; a fair node keeps
// its number in node[v] and its or_me mask, an unfair one puts X' on the stack.
template <bool MOVES = true, class M, class Start = LiveInitStart>
LiveHostFair<sr_live_strong> live_host_strong(const M& m, int p, u64 max_states, const Start& start = Start{}) {
    return live_host_fair<LiveStrongWalk, sr_live_strong, MOVES>(
        m, p, max_states, [](auto& G, sr_live_strong& sg, std::vector<u32>& node, std::vector<std::vector<u32>>& members, std::vector<u64>& node_or_me) {
            constexpr int MW = M::MW;
            constexpr u32 NONE = ~0u;
            struct Job {
                std::vector<u32> x;
                u32 depth;
            };
            std::vector<Job> jobs(1, Job{{}, 1});
            for (u32 v = 0; v < G.nf; ++v) jobs[0].x.push_back(v);
            std::vector<u32> in_x(G.nf, NONE), in_c(G.nf, NONE);
            u32 job_no = 0, comp_no = 0;
            while (!jobs.empty()) {
                const Job job = std::move(jobs.back());
                jobs.pop_back();
                const u32 tag = job_no++;
                for (u32 v : job.x) in_x[v] = tag;
                G.components(job.x, [&](u32 t) { return in_x[t] == tag; }, [&](std::vector<u32>& c) {
                    sg.components += 1;
                    sg.levels = std::max(sg.levels, job.depth);
                    const u32 cn = comp_no++;
                    for (u32 x : c) in_c[x] = cn;
                    u64 or_me[MW] = {}, or_took[MW] = {};
                    for (u32 x : c) {
                        for (int w = 0; w < MW; ++w) or_me[w] |= G.me[(size_t)x * MW + w];
                        for (const auto& e : G.out_e[x])
                            if (in_c[e.t] == cn) or_took[e.a >> 6] |= 1ull << (e.a & 63);
                    }
                    if (live_strong_masks<MW>(or_me, or_took)) {
                        for (u32 x : c) node[x] = (u32)members.size();
                        members.push_back(std::move(c));
                        node_or_me.insert(node_or_me.end(), or_me, or_me + MW);
                        sg.fair_components += 1;
                        return;
                    }
                    Job sub{{}, job.depth + 1};
                    for (u32 x : c) {
                        bool hit = false;
                        for (int w = 0; w < MW; ++w) hit = hit || (G.me[(size_t)x * MW + w] & or_me[w] & ~or_took[w]);
                        if (!hit) sub.x.push_back(x);
                    }
                    if (sub.x.size() >= c.size()) throw Error(SR_ERR_NONDETERMINISM, "liveness: an unfair component loses no state");
                    if (sub.x.size() >= 2) jobs.push_back(std::move(sub));
                });
            }
        }, start);
}

}  // namespace sr
