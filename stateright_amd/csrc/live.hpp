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
// (DESIGN.md §10). The simulation checker's loop detection is not changed (a self-loop still closes
// a lasso there), and what the plain mode refuses (plugins, partitions, symmetry,
// target_state_count) this mode refuses too.
//
// The per-state rule and the witness step are ONE function, live_step below, which the kernels
// (kernels_live.hpp: live_trim, live_walk) and the host form (live_host, the sr_liveness_host entry
// point) instantiate; they differ only in how "is this successor in the set" is answered (the alive
// bitmap by visited-set slot on the device, a hash map on the host).
#pragma once
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

}  // namespace sr
