// The step pass: STEP properties, invariants over transitions (TLA+'s [][A]_v), decided over
// the edges of the reachable set of a check that explored everything. A state property cannot say "an RM
// that has decided never changes its decision" or "no action takes the counter down" without a history
// variable, which would change the state space and its counts; a step property says it directly.
//
// A model declares a step property p with `expectation(p) == ALWAYS_STEP`, bit p of the host member
// `smask()` (models.hpp has_smask) and the hook
//     SR_HD bool step_holds(int p, const u64* s, int a, const u64* t) const
// `discovers(p, .)` is false for it, so the search itself never discovers it.
//
//   R         the set of distinct reachable states: the arena, an init state that repeats an earlier init
//             state counted once (the coverage pass' skip mask);
//   an EDGE   a pair (s, a) with s in R, slot a in enabled(s) and apply(s, a, t) succeeding: the coverage
//             pass' "taken". A slot whose apply refuses (or whose successor is outside the boundary) is no
//             edge; a step whose successor equals its state is an edge like any other.
// Per step property p, 64 bits and exact:
//   edges       the number of edges (the same for every property, the sum of the coverage pass' taken);
//   violations  the edges where step_holds(p, s, a, t) is false;
//   sources     the states with at least one violating edge.
// p has a counterexample iff violations > 0. The SEED is the violating edge whose source has the lowest depth
// (its level in the search), then the source that is lowest compared word by word from word 0, unsigned
// (live_leads_less), then the lowest slot. Never the arena index: in FAST order it differs from run to run.
// The WITNESS is the search's own tree path from an init state to the seed's source, followed by the seed's
// action: depth + 1 actions, step_index = depth, the last state is t; init_index is the lowest index of an init
// state equal to its first state. No earlier step of it can violate p: its source has a lower depth than the
// seed's, which is the lowest of a violating source. Accepted (before a path is returned): every step is a
// successor in `actions()` order, no step before the last violates p, and the last one does.
//
// The rule's pieces (step_holds_of, step_violated) are SR_HD and written once here; the kernels
// (kernels_step.hpp step_scan, step_min) and the host form (step_host below, behind sr_step_host) differ only
// in how they walk R and where they add. The device's driver is Engine<M>::step_pass (engine.hpp).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/stateright_gpu.h"
#include "cover.hpp"
#include "device.hpp"
#include "kernels.hpp"
#include "live.hpp"

namespace sr {

template <class M>
SR_HD bool step_holds_of(const M& m, int p, const u64* s, int a, const u64* t) {
    if constexpr (has_smask<M>::value) return m.step_holds(p, s, a, t);
    else return (void)m, (void)p, (void)s, (void)a, (void)t, true;
}

// The step properties of `smask` that the edge (s, a) -> t violates, as a bit mask.
template <class M>
SR_HD u32 step_violated(const M& m, u32 smask, const u64* s, int a, const u64* t) {
    u32 v = 0;
#pragma unroll
    for (int p = 0; p < M::NPROPS; ++p)
        if ((smask >> p & 1) && !step_holds_of(m, p, s, a, t)) v |= 1u << p;
    return v;
}

inline sr_step_result step_none() {
    sr_step_result r{};
    r.struct_size = (u32)sizeof(sr_step_result);
    r.step_index = r.step_action = r.witness_len = -1;
    r.init_index = -1;
    return r;
}

// The declared mask, checked: every bit names a property whose expectation is ALWAYS_STEP, and no other
// property has that expectation.
template <class M>
inline u32 step_checked_mask(const M& m) {
    const u32 sm = model_smask(m);
    for (int p = 0; p < 32; ++p) {
        const bool bit = sm >> p & 1, step = p < M::NPROPS && m.expectation(p) == ALWAYS_STEP;
        if (bit != step)
            throw Error(SR_ERR_ARG, "step properties: smask() and expectation() disagree about property " + std::to_string(p));
    }
    return sm;
}

// The lowest index of an init state equal to s (-1: none).
template <class M>
inline int32_t step_init_index(const std::vector<u64>& inits, const u64* s) {
    for (size_t i = 0; i < inits.size() / M::W; ++i)
        if (std::equal(&inits[i * M::W], &inits[i * M::W] + M::W, s)) return (int32_t)i;
    return -1;
}

// The acceptance of a witness (states: W words each, depth + 2 of them; last_slot: the seed's slot): every
// step of the tree path is a successor (the first in `actions()` order that leads to the next state, as
// concrete_path of engine.hpp takes it), the last state is apply(source, last_slot), no earlier step violates p
// and the last one does. Returns the canonical action ids.
template <class M>
inline std::vector<i64> step_accept(const M& m, int p, const std::vector<u64>& states, int last_slot) {
    constexpr int W = M::W;
    const std::string name = m.prop_name(p);
    const size_t len = states.size() / W;
    if (len < 2) throw Error(SR_ERR_NONDETERMINISM, "step pass: the witness of \"" + name + "\" has no step");
    std::vector<i64> acts;
    for (size_t i = 0; i + 2 < len; ++i) {
        bool bad = false, found = false;
        for_each_successor(m, &states[i * W], [&](int a, const u64* ns) {
            if (found || !std::equal(ns, ns + W, &states[(i + 1) * W])) return;
            found = true;
            bad = !step_holds_of(m, p, &states[i * W], a, ns);
            acts.push_back(m.action_id(&states[i * W], a));
        });
        if (!found) throw Error(SR_ERR_NONDETERMINISM, "step pass: step " + std::to_string(i) + " of the witness of \"" + name + "\" is no successor of its state");
        if (bad) throw Error(SR_ERR_NONDETERMINISM, "step pass: step " + std::to_string(i) + " of the witness of \"" + name + "\" violates it before the seed");
    }
    const u64* src = &states[(len - 2) * W];
    u64 mask[M::MW], out[W];
    m.enabled(src, mask);
    if (last_slot < 0 || last_slot >= 64 * M::MW || !(mask[last_slot >> 6] >> (last_slot & 63) & 1) || !m.apply(src, last_slot, out) ||
        !std::equal(out, out + W, &states[(len - 1) * W]))
        throw Error(SR_ERR_NONDETERMINISM, "step pass: the last step of the witness of \"" + name + "\" is no edge of its source");
    if (step_holds_of(m, p, src, last_slot, out))
        throw Error(SR_ERR_NONDETERMINISM, "step pass: the last step of the witness of \"" + name + "\" does not violate it");
    acts.push_back(m.action_id(src, last_slot));
    return acts;
}

template <class M>
std::vector<u64> init_states_of(const M& m);  // (engine.hpp)

// The host form (sr_step_host): a host search of m in the reference's FIFO order over at most max_states states
// (SR_ERR_CAPACITY beyond), the three counts and the seed of property p by the rule above, and the witness along
// that search's tree.
struct StepHost {
    sr_step_result r;
    std::vector<i64> actions;
    u64 unique = 0;
};
template <class M>
inline StepHost step_host(const M& m, int p, u64 max_states) {
    constexpr int W = M::W;
    const auto t0 = std::chrono::steady_clock::now();
    const u32 sm = step_checked_mask(m);
    if (p < 0 || p >= M::NPROPS || !(sm >> p & 1)) throw Error(SR_ERR_ARG, "step pass: property " + std::to_string(p) + " is not a step property");
    std::map<std::vector<u64>, u64> index;
    std::vector<std::vector<u64>> st;
    std::vector<u64> parent;
    std::vector<u32> depth;
    auto add = [&](const u64* s, u64 par, u32 d) {
        std::vector<u64> v(s, s + W);
        if (index.count(v)) return;
        if (st.size() >= max_states)
            throw Error(SR_ERR_CAPACITY, "sr_step_host: more than " + std::to_string(max_states) + " reachable states (max_states)");
        index.emplace(v, (u64)st.size());
        st.push_back(std::move(v));
        parent.push_back(par);
        depth.push_back(d);
    };
    const std::vector<u64> inits = init_states_of(m);
    const size_t k = inits.size() / W;
    for (size_t i = k; i-- > 0;) add(&inits[i * W], ~0ull, 0);  // (level 0 is visited in reverse init order)
    StepHost h;
    h.r = step_none();
    u64 seed = ~0ull;
    int seed_slot = -1;
    for (size_t q = 0; q < st.size(); ++q) {
        const std::vector<u64> s = st[q];  // (a copy: add() grows st)
        if constexpr (has_faulted<M>::value) {
            if (m.faulted(s.data())) throw Error(SR_ERR_UNSUPPORTED, model_fault_text(m));
        }
        int first_bad = -1;
        for_each_successor(m, s.data(), [&](int a, const u64* ns) {
            h.r.edges += 1;
            if (!step_holds_of(m, p, s.data(), a, ns)) {
                h.r.violations += 1;
                if (first_bad < 0) first_bad = a;
            }
            add(ns, (u64)q, depth[q] + 1);
        });
        if (first_bad < 0) continue;
        h.r.sources += 1;
        if (seed == ~0ull || depth[q] < depth[seed] || (depth[q] == depth[seed] && live_leads_less<W>(s.data(), st[seed].data())))
            seed = (u64)q, seed_slot = first_bad;
    }
    h.unique = (u64)st.size();
    h.r.ran = 1;
    if (seed != ~0ull) {
        std::vector<u64> chain;
        for (u64 q = seed; q != ~0ull; q = parent[q]) chain.push_back(q);
        std::vector<u64> states;
        for (size_t i = chain.size(); i-- > 0;) states.insert(states.end(), st[chain[i]].begin(), st[chain[i]].end());
        u64 out[W];
        m.apply(st[seed].data(), seed_slot, out);
        states.insert(states.end(), out, out + W);
        h.actions = step_accept(m, p, states, seed_slot);
        h.r.step_index = (int64_t)depth[seed];
        h.r.step_action = h.actions.back();
        h.r.witness_len = (int64_t)h.actions.size();
        h.r.init_index = step_init_index<M>(inits, states.data());
    }
    h.r.scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return h;
}

// sr_gpu_bfs_replay_step: the actions are replayed from init state `init` as replay_model replays them; 1: the
// last step holds for the step property p, 0: it violates it; -1: no such path, no step, or p is no step property.
template <class M>
int step_replay_model(const M& m, int init, const i64* ids, int n, int p) {
    constexpr int W = M::W;
    if (p < 0 || p >= M::NPROPS || !(model_smask(m) >> p & 1) || n < 1) return -1;
    const std::vector<u64> inits = init_states_of(m);
    if (init < 0 || init >= (int)(inits.size() / W)) return -1;
    std::vector<u64> cur(&inits[(size_t)init * W], &inits[(size_t)init * W] + W);
    int holds = -1;
    for (int i = 0; i < n; ++i) {
        bool found = false;
        std::vector<u64> nx;
        for_each_successor(m, cur.data(), [&](int a, const u64* ns) {
            if (found || m.action_id(cur.data(), a) != ids[i]) return;
            nx.assign(ns, ns + W), found = true;
            holds = step_holds_of(m, p, cur.data(), a, ns) ? 1 : 0;
        });
        if (!found) return -1;
        cur = nx;
    }
    return holds;
}

}  // namespace sr

#include "kernels_step.hpp"
