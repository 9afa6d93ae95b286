// The coverage pass (opt-in: sr_opts.coverage, `CheckerBuilder.coverage()`): what each
// action class and each property did over the reachable set of a check that explored everything. A
// "no discovery over N states" answer says nothing about whether the model did what its author believes:
// an action that is never enabled, or always cut by the boundary, makes every `always` property hold
// vacuously, and so does a property whose condition is true nowhere or everywhere.
//
//   R            the set of distinct reachable states: the arena, with an init state that repeats an
//                earlier init state counted once (the arena holds level 0 as given);
//   class(s, a)  the action class of slot a at s, in [0, cover_classes()): the slot itself, or the
//                model's `cover_class` hook (include/stateright_gpu_model.hpp; cover_hook_model below).
// For each s in R and each slot a of enabled(s), in slot order, with c = class(s, a):
//   enabled[c] += 1;  taken[c] += 1 if apply(s, a, out);  moved[c] += 1 if also out differs from s.
// Per state, deg = its taken slots and mdeg = its moved slots:
//   terminal += (deg == 0);  stutter_ends += (deg > 0 && mdeg == 0);
//   out_degree[min(deg, 63)] += 1;  max_out_degree = max(deg).
// Per property p: holds[p] += condition(p, s), condition = (expectation(p) == ALWAYS) != discovers(p, s)
// (sr_host_graph's convention). states = |R|.
//
// The rule's pieces (cover_class_of, cover_moved, cover_conditions, cover_bucket) are SR_HD and written
// once here; the kernel (kernels_cover.hpp cover_count) and the host form (cover_host below, behind
// sr_coverage_host) differ only in how they walk R and where they add. The device's driver is
// Engine<M>::cover_pass (engine.hpp).
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/stateright_gpu.h"
#include "device.hpp"
#include "kernels.hpp"

namespace sr {

constexpr int COVER_MAX_CLASSES = 1024;  // more is SR_ERR_UNSUPPORTED at spawn
constexpr int COVER_DEGREES = 64;        // out_degree's buckets: 0 .. 62, and 63 for "63 or more"

// The optional hook: SR_HD int cover_class(const u64* s, int a) const, with the host members
// int cover_classes() const and std::string cover_class_name(int c) const.
template <class M, class = void>
struct has_cover_class : std::false_type {};
template <class M>
struct has_cover_class<M, std::void_t<decltype(std::declval<const M&>().cover_class((const u64*)nullptr, 0)),
                                      decltype(std::declval<const M&>().cover_classes()),
                                      decltype(std::declval<const M&>().cover_class_name(0))>> : std::true_type {};
template <class M>
constexpr bool cover_hook_model = has_cover_class<M>::value;

template <class M>
SR_HD int cover_class_of(const M& m, const u64* s, int a) {
    if constexpr (cover_hook_model<M>) return m.cover_class(s, a);
    else return (void)m, (void)s, a;
}
template <class M>
inline int cover_classes_of(const M& m) {
    if constexpr (cover_hook_model<M>) return m.cover_classes();
    else return m.max_actions();
}
// The default name is the action's where the model's action ids are its slots, "slot <a>" otherwise.
template <class M>
inline std::string cover_class_name_of(const M& m, int c) {
    if constexpr (cover_hook_model<M>) return m.cover_class_name(c);
    else return m.action_id_bound() == (i64)m.max_actions() ? m.action_name(c) : "slot " + std::to_string(c);
}

template <int W>
SR_HD bool cover_moved(const u64* s, const u64* out) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < W; ++i) eq = eq && s[i] == out[i];
    return !eq;
}
// The properties whose CONDITION holds at s, as a bit mask; `always` has bit p set iff expectation(p)
// is ALWAYS (cover_always_mask: expectation() is a host member).
template <class M>
SR_HD u32 cover_conditions(const M& m, u32 always, const u64* s) {
    u32 h = 0;
    for (int p = 0; p < M::NPROPS; ++p)
        if (((always >> p & 1) != 0) != m.discovers(p, s)) h |= 1u << p;
    return h;
}
template <class M>
inline u32 cover_always_mask(const M& m) {
    u32 a = 0;
    for (int p = 0; p < M::NPROPS; ++p)
        if (m.expectation(p) == ALWAYS) a |= 1u << p;
    return a;
}
SR_HD u32 cover_bucket(u32 deg) { return deg < (u32)COVER_DEGREES - 1 ? deg : (u32)COVER_DEGREES - 1; }

// The figures of a pass: the fixed part (sr_coverage) and the per-class and per-property counts.
struct CoverFigures {
    sr_coverage c{};
    std::vector<u64> enabled, taken, moved, holds;
    std::vector<std::string> names;
};

inline sr_coverage cover_none() {
    sr_coverage c{};
    c.struct_size = (u32)sizeof(sr_coverage);
    return c;
}

// The class count of m, checked; and a CoverFigures with its names and zeroed counts.
template <class M>
inline int cover_checked_classes(const M& m) {
    const int C = cover_classes_of(m);
    if (C < 0 || C > COVER_MAX_CLASSES)
        throw Error(SR_ERR_UNSUPPORTED, "coverage: the model has " + std::to_string(C) + " action classes; at most " +
                                            std::to_string(COVER_MAX_CLASSES) + " are counted");
    return C;
}
template <class M>
inline CoverFigures cover_figures_for(const M& m) {
    CoverFigures f;
    const int C = cover_checked_classes(m);
    f.c = cover_none();
    f.c.classes = C;
    f.c.nprops = M::NPROPS;
    f.enabled.assign((size_t)C, 0);
    f.taken.assign((size_t)C, 0);
    f.moved.assign((size_t)C, 0);
    f.holds.assign((size_t)M::NPROPS, 0);
    for (int c = 0; c < C; ++c) f.names.push_back(cover_class_name_of(m, c));
    return f;
}

// One state's contribution, on the host.
template <class M>
inline void cover_add_state(const M& m, u32 always, const u64* s, CoverFigures& f) {
    u64 mask[M::MW], out[M::W];
    m.enabled(s, mask);
    u32 deg = 0, mdeg = 0;
    for (int w = 0; w < M::MW; ++w)
        for (u64 bits = mask[w]; bits; bits &= bits - 1) {
            const int a = w * 64 + __builtin_ctzll(bits);
            const int c = cover_class_of(m, s, a);
            if (c < 0 || c >= f.c.classes)
                throw Error(SR_ERR_NONDETERMINISM, "coverage: cover_class returned " + std::to_string(c) + " for slot " + std::to_string(a) +
                                                       "; the model declares " + std::to_string(f.c.classes) + " classes");
            f.enabled[(size_t)c] += 1;
            if (!m.apply(s, a, out)) continue;
            f.taken[(size_t)c] += 1;
            deg += 1;
            if (!cover_moved<M::W>(s, out)) continue;
            f.moved[(size_t)c] += 1;
            mdeg += 1;
        }
    f.c.states += 1;
    f.c.terminal += deg == 0;
    f.c.stutter_ends += deg > 0 && mdeg == 0;
    f.c.out_degree[cover_bucket(deg)] += 1;
    if (deg > f.c.max_out_degree) f.c.max_out_degree = deg;
    const u32 h = cover_conditions(m, always, s);
    for (int p = 0; p < M::NPROPS; ++p) f.holds[(size_t)p] += h >> p & 1;
}

template <class M>
std::vector<u64> init_states_of(const M& m);  // (engine.hpp)

// The host form (sr_coverage_host): a host search of m over at most max_states states (SR_ERR_CAPACITY
// beyond), every distinct state counted once by the rule above.
template <class M>
inline CoverFigures cover_host(const M& m, u64 max_states) {
    constexpr int W = M::W;
    const auto t0 = std::chrono::steady_clock::now();
    CoverFigures f = cover_figures_for(m);
    const u32 always = cover_always_mask(m);
    std::map<std::vector<u64>, u64> index;
    std::vector<std::vector<u64>> st;
    auto add = [&](const u64* s) {
        std::vector<u64> v(s, s + W);
        if (index.count(v)) return;
        if (st.size() >= max_states)
            throw Error(SR_ERR_CAPACITY, "sr_coverage_host: more than " + std::to_string(max_states) + " reachable states (max_states)");
        index.emplace(v, (u64)st.size());
        st.push_back(std::move(v));
    };
    const std::vector<u64> inits = init_states_of(m);
    for (size_t i = 0; i + W <= inits.size(); i += W) add(&inits[i]);
    for (size_t q = 0; q < st.size(); ++q) {
        const std::vector<u64> s = st[q];  // (a copy: add() grows st)
        if constexpr (has_faulted<M>::value) {
            if (m.faulted(s.data())) throw Error(SR_ERR_UNSUPPORTED, model_fault_text(m));
        }
        cover_add_state(m, always, s.data(), f);
        for_each_successor(m, s.data(), [&](int, const u64* ns) { add(ns); });
    }
    f.c.ran = 1;
    f.c.pass_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return f;
}

}  // namespace sr

#include "kernels_cover.hpp"
