// MI355X breadth-first model-checking engine: the host level loop over the HIP kernels, as a
// header of templates over a GpuModel M (models.hpp), so that the engine library (engine.hip: the
// compiled-in registry + the C ABI) and a user's own plugin build (include/stateright_gpu_model.hpp)
// instantiate the same code.
//
// Replaces `BfsChecker` (src/checker/bfs.rs). The reference's T worker threads, job market and
// 1500-state blocks (bfs.rs:75-152) become one host driver thread per GPU that runs the search
// level by level; each level is one pass of HIP kernels over the frontier held in HBM (kernels.hpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <immintrin.h>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/stateright_gpu.h"
#include "device.hpp"
#include "kernels.hpp"
#include "kernels_audit.hpp"
#include "live.hpp"
#include "cover.hpp"
#include "step.hpp"
#include "certify.hpp"

namespace sr {


using Clock = std::chrono::steady_clock;
static double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

static inline u32 blocks_for(u64 n, u32 bs) { return (u32)((n + bs - 1) / bs); }

using Ctx = DeviceContext<LevelCounters, HostCounters>;
using CtxPool = ContextPool<Ctx>;

// Holds a pooled device context for the duration of a scope.
struct CtxLease {
    Ctx* c;
    explicit CtxLease(int dev) : c(CtxPool::get().acquire(dev)) {}
    ~CtxLease() { CtxPool::get().release(c); }
};

struct DiscoveryRec {
    bool found = false;
    u32 level = 0, rank = 0;  // the discovering state: rank in the visit order of its level
};

class EngineBase {
  public:
    virtual ~EngineBase() = default;
    virtual void run() = 0;
    virtual int nprops() const = 0;
    virtual const char* prop_name(int p) const = 0;
    virtual int expectation(int p) const = 0;
    virtual int width() const = 0;
    virtual std::string action_name(i64 id) const = 0;
    virtual int chain(int p, std::vector<u64>& out) = 0;
    virtual int path(int p, std::vector<i64>& actions, std::vector<i64>& states) = 0;
    virtual std::vector<i64> visits() const = 0;
    // Per visit (visit order): the visit index of its BFS-tree parent (-1 for an init state) and
    // the canonical id of the first action leading there (-1 for an init state). Returns false if
    // the engine keeps no visit record.
    virtual bool visit_tree(std::vector<i64>&, std::vector<i64>&) const { return false; }
    virtual i64 action_id_bound() const = 0;
    virtual int init_count() const = 0;
    // `Path::from_actions` (src/checker/path.rs:90-112) from init state `init`: the states, each
    // property's CONDITION on the last state, optionally on every state ((n + 1) x nprops), and
    // whether the last state is terminal (`actions()` lists nothing). -1: an action is not enabled.
    virtual int replay(int init, const i64* ids, int n, std::vector<i64>& states, std::vector<int>& conds,
                       std::vector<int>* all_conds = nullptr, int* terminal = nullptr) const = 0;
    virtual int explore(const u64* fps, int n, std::vector<i64>& action, std::vector<int>& has, std::vector<u64>& fp,
                        std::vector<i64>& states) const = 0;
    // The sink kind of the state the actions lead to from init state `init` (sr_gpu_bfs_sink_kind).
    virtual int sink_kind(int init, const i64* ids, int n) const {
        (void)init, (void)ids, (void)n;
        return -1;
    }
    // The complete `eventually` check's outcome for property p (live.hpp); false: p is no property.
    virtual bool live_result(int p, sr_live_result* out) const {
        if (p < 0 || p >= nprops()) return false;
        *out = p < (int)live.size() ? live[p] : live_result_none();
        return true;
    }

    // The weak-fairness figures of that check (sr_gpu_bfs_liveness_weak); false: p is no property.
    virtual bool live_weak_result(int p, sr_live_weak* out) const {
        if (p < 0 || p >= nprops()) return false;
        *out = p < (int)live_weak.size() ? live_weak[p] : live_fair_none<sr_live_weak>();
        return true;
    }
    // Whether the loop of the lasso that the actions describe from init state `init` is weakly fair
    // (sr_gpu_bfs_loop_fair); strong: strongly fair (sr_gpu_bfs_loop_strongly_fair).
    virtual int loop_fair(int init, const i64* ids, int n, int loop_start, bool strong = false) const {
        (void)init, (void)ids, (void)n, (void)loop_start, (void)strong;
        return -1;
    }
    // The trigger of the leads-to property p on every state of the path that the actions describe from init state
    // `init` (sr_gpu_bfs_replay_triggers): n + 1 entries; -1: no such path, or p is no leads-to property.
    virtual int triggers(int init, const i64* ids, int n, int p, std::vector<int>& out) const {
        (void)init, (void)ids, (void)n, (void)p, (void)out;
        return -1;
    }
    // The strong-fairness figures of that check (sr_gpu_bfs_liveness_strong); false: p is no property.
    bool live_strong_result(int p, sr_live_strong* out) const {
        if (p < 0 || p >= nprops()) return false;
        *out = p < (int)live_strong.size() ? live_strong[p] : live_fair_none<sr_live_strong>();
        return true;
    }

    std::vector<sr_live_result> live;  // per property (empty: the pass never ran)
    std::vector<sr_live_weak> live_weak;  // per property (empty: the pass never ran in the weak mode)
    std::vector<sr_live_strong> live_strong;  // per property (empty: the pass never ran in the strong mode)
    std::vector<sr_live_leads> live_leads;  // per property (empty: the pass never ran; ran = 0: no leads-to property)
    // The leads-to figures of that check (sr_gpu_bfs_liveness_leads); false: p is no property.
    bool live_leads_result(int p, sr_live_leads* out) const {
        if (p < 0 || p >= nprops()) return false;
        *out = p < (int)live_leads.size() ? live_leads[p] : live_leads_none();
        return true;
    }
    CoverFigures cover;  // the coverage pass' figures (cover.hpp; c.ran = 0: it did not run)
    std::vector<sr_step_result> step;  // per property (empty: the step pass never ran; ran = 0: no step property)
    // The step pass' figures for property p (sr_gpu_bfs_step); false: p is no property.
    bool step_result(int p, sr_step_result* out) const {
        if (p < 0 || p >= nprops()) return false;
        *out = p < (int)step.size() ? step[p] : step_none();
        return true;
    }
    // Whether the last step of the path that the actions describe from init state `init` holds for the step
    // property p (sr_gpu_bfs_replay_step): 1 / 0; -1: no such path, no step, or p is no step property.
    virtual int step_replay(int init, const i64* ids, int n, int p) const {
        (void)init, (void)ids, (void)n, (void)p;
        return -1;
    }
    std::atomic<u64> state_count{0}, unique{0};
    std::atomic<u32> max_depth{0};
    std::atomic<bool> finished{false};
    bool reference_done = false;  // `is_done` (bfs.rs:307-311): explored all or discovered all
    int status = SR_OK;
    std::string error;
    sr_stats stats{};
    sr_table_audit audit{};  // the visited-set audit of a counting run (kernels_audit.hpp); ran = 0 otherwise
    sr_certificate cert = cert_none();  // the certificate pass' figures (certify.hpp; ran = 0: it did not run)
    std::vector<DiscoveryRec> disc;
    std::vector<double> launch_ms;    // per timed launch (profile=1), in launch order
    std::vector<u64> launch_frontier; // the frontier each launch expanded (0 if unknown)
    std::vector<u64> launch_probes;   // visited-set probes / CAS claims of each launch (the pipelined
    std::vector<u64> launch_cas;      // FAST loop with sr_opts.counters; 0 otherwise)
};

// The model's init states (k * W words), in a buffer sized by init_capacity; a model that reports
// more states than fit is refused (every host-side caller goes through here, and the engines call
// it once when they are created, so a bad plugin fails at spawn).
template <class M>
std::vector<u64> init_states_of(const M& m) {
    const int cap = init_capacity(m);
    std::vector<u64> v((size_t)cap * M::W + M::W);  // one spare state: a model off by one is caught, not silent
    const int k = m.init_states(v.data());
    if (k < 0 || k > cap)
        throw Error(SR_ERR_ARG, "init_states returned " + std::to_string(k) + " states; at most " + std::to_string(cap) +
                                    " fit (a model with more than " + std::to_string(MAX_INIT_STATES) +
                                    " init states must report init_count())");
    v.resize((size_t)k * M::W);
    return v;
}

// The sink kind (sr_gpu_bfs_sink_kind) of the state that the canonical action ids lead to from init
// state `init`, steps matched as replay_model matches them: -1 no such path, 0 the state has a
// successor other than itself, SR_LIVE_END_TERMINAL no successor, SR_LIVE_END_STUTTER successors, all itself.
template <class M>
int sink_kind_model(const M& m, int init, const i64* ids, int n) {
    constexpr int W = M::W;
    const std::vector<u64> inits = init_states_of(m);
    if (init < 0 || init >= (int)(inits.size() / W)) return -1;
    std::vector<u64> cur(&inits[(size_t)init * W], &inits[(size_t)init * W] + W);
    for (int i = 0; i < n; ++i) {
        bool found = false;
        std::vector<u64> nx;
        for_each_successor(m, cur.data(), [&](int a, const u64* ns) {
            if (!found && m.action_id(cur.data(), a) == ids[i]) nx.assign(ns, ns + W), found = true;
        });
        if (!found) return -1;
        cur = nx;
    }
    u64 all = 0, other = 0;
    for_each_successor(m, cur.data(), [&](int, const u64* ns) { ++all, other += !std::equal(cur.begin(), cur.end(), ns); });
    return other ? 0 : all ? SR_LIVE_END_STUTTER : SR_LIVE_END_TERMINAL;
}

// sr_gpu_bfs_loop_fair: the actions are replayed from init state `init` as sink_kind_model replays them;
// the loop is the states from index loop_start to the last. -1 no such path (or the model's slots are
// no fairness classes), 1 the loop is closed and weakly fair (live.hpp live_loop_fair; strong: strongly fair,
// live_loop_strong_fair), 0 it is not.
template <class M>
int loop_fair_model(const M& m, int init, const i64* ids, int n, int loop_start, bool strong = false) {
    constexpr int W = M::W;
    if constexpr (!fair_slots_model<M>) {
        return -1;
    } else {
        const std::vector<u64> inits = init_states_of(m);
        if (init < 0 || init >= (int)(inits.size() / W) || loop_start < 0 || loop_start > n) return -1;
        std::vector<u64> path(&inits[(size_t)init * W], &inits[(size_t)init * W] + W);
        for (int i = 0; i < n; ++i) {
            bool found = false;
            std::vector<u64> nx;
            const u64* cur = &path[(size_t)i * W];
            for_each_successor(m, cur, [&](int a, const u64* ns) {
                if (!found && m.action_id(cur, a) == ids[i]) nx.assign(ns, ns + W), found = true;
            });
            if (!found) return -1;
            path.insert(path.end(), nx.begin(), nx.end());
        }
        const u64* loop = &path[(size_t)loop_start * W];
        return (strong ? live_loop_strong_fair(m, loop, (size_t)(n - loop_start)) : live_loop_fair(m, loop, (size_t)(n - loop_start))) ? 1 : 0;
    }
}

// sr_gpu_bfs_replay_triggers: the actions are replayed from init state `init` as sink_kind_model replays them;
// out takes leads_from(p, .) of every state of the path. -1: no such path, or p is no leads-to property.
template <class M>
int triggers_model(const M& m, int init, const i64* ids, int n, int p, std::vector<int>& out) {
    constexpr int W = M::W;
    out.clear();
    if (p < 0 || p >= M::NPROPS || !(model_lmask(m) >> p & 1)) return -1;
    const std::vector<u64> inits = init_states_of(m);
    if (init < 0 || init >= (int)(inits.size() / W)) return -1;
    std::vector<u64> cur(&inits[(size_t)init * W], &inits[(size_t)init * W] + W);
    out.push_back(live_leads_from(m, p, cur.data()) ? 1 : 0);
    for (int i = 0; i < n; ++i) {
        bool found = false;
        std::vector<u64> nx;
        for_each_successor(m, cur.data(), [&](int a, const u64* ns) {
            if (!found && m.action_id(cur.data(), a) == ids[i]) nx.assign(ns, ns + W), found = true;
        });
        if (!found) return -1;
        cur = nx;
        out.push_back(live_leads_from(m, p, cur.data()) ? 1 : 0);
    }
    return n + 1;
}

template <class M>
int replay_model(const M& m, int init, const i64* ids, int n, std::vector<i64>& states, std::vector<int>& conds,
                 std::vector<int>* all_conds, int* terminal) {
    constexpr int W = M::W;
    const std::vector<u64> inits = init_states_of(m);
    const int k = (int)(inits.size() / W);
    if (init < 0 || init >= k) return -1;
    const int wd = m.describe_width();
    std::vector<u64> cur(&inits[init * W], &inits[init * W] + W);
    // the property's condition (discovers() is !condition for `always`, the condition otherwise)
    auto cond = [&](int p, const u64* s) { return m.expectation(p) == ALWAYS ? !m.discovers(p, s) : m.discovers(p, s); };
    auto emit = [&](const u64* s) {
        size_t o = states.size();
        states.resize(o + wd);
        m.describe(s, &states[o]);
        if (all_conds)
            for (int p = 0; p < M::NPROPS; ++p) all_conds->push_back(cond(p, s) ? 1 : 0);
    };
    if (all_conds) all_conds->clear();
    for (int i = 0; i < n; ++i) {
        u64 mask[M::MW];
        m.enabled(cur.data(), mask);
        bool found = false;
        for (int w = 0; w < M::MW && !found; ++w)
            for (u64 bits = mask[w]; bits && !found; bits &= bits - 1) {
                int a = w * 64 + __builtin_ctzll(bits);
                if (m.action_id(cur.data(), a) != ids[i]) continue;
                u64 ns[W];
                if (!m.apply(cur.data(), a, ns)) continue;
                emit(cur.data());
                cur.assign(ns, ns + W);
                found = true;
            }
        if (!found) return -1;
    }
    emit(cur.data());
    conds.assign(M::NPROPS, 0);
    for (int p = 0; p < M::NPROPS; ++p) conds[p] = cond(p, cur.data()) ? 1 : 0;
    if (terminal) {
        u64 mask[M::MW];
        m.enabled(cur.data(), mask);
        u64 any = 0;
        for (int w = 0; w < M::MW; ++w) any |= mask[w];
        *terminal = any == 0;
    }
    return n;
}

// Explorer's `states` route (src/checker/explorer.rs:159-240) on the host copy of the encoding:
// with no fingerprints, the init states; otherwise `Path::final_state` (src/checker/path.rs:115-136:
// the init state with the first fingerprint, then the first matching step per fingerprint) and,
// for every action `actions()` lists there in order, the next state (has = 0: `next_state` is
// None, the reference's "Action ignored" view). Returns the number of views, or -1 if no state
// follows the fingerprints.
template <class M>
int explore_model(const M& m, const u64* fps, int n, std::vector<i64>& action, std::vector<int>& has,
                  std::vector<u64>& fp_out, std::vector<i64>& states) {
    constexpr int W = M::W;
    const int wd = m.describe_width();
    auto emit = [&](i64 a, const u64* s) {
        action.push_back(a);
        has.push_back(s ? 1 : 0);
        fp_out.push_back(s ? state_fp<M>(s) : 0);
        const size_t o = states.size();
        states.resize(o + wd, 0);
        if (s) m.describe(s, &states[o]);
    };
    const std::vector<u64> inits = init_states_of(m);
    const int k = (int)(inits.size() / W);
    if (n == 0) {
        for (int i = 0; i < k; ++i) emit(-1, &inits[i * W]);
        return k;
    }
    std::vector<u64> cur;
    for (int i = 0; i < k && cur.empty(); ++i)
        if (state_fp<M>(&inits[i * W]) == fps[0]) cur.assign(&inits[i * W], &inits[i * W] + W);
    if (cur.empty()) return -1;
    for (int j = 1; j < n; ++j) {
        u64 mask[M::MW];
        m.enabled(cur.data(), mask);
        bool found = false;
        for (int w = 0; w < M::MW && !found; ++w)
            for (u64 bits = mask[w]; bits && !found; bits &= bits - 1) {
                const int a = w * 64 + __builtin_ctzll(bits);
                u64 ns[W];
                if (m.apply(cur.data(), a, ns) && state_fp<M>(ns) == fps[j]) {
                    cur.assign(ns, ns + W);
                    found = true;
                }
            }
        if (!found) return -1;
    }
    u64 mask[M::MW];
    m.enabled(cur.data(), mask);
    int views = 0;
    for (int w = 0; w < M::MW; ++w)
        for (u64 bits = mask[w]; bits; bits &= bits - 1) {
            const int a = w * 64 + __builtin_ctzll(bits);
            u64 ns[W];
            const bool ok = m.apply(cur.data(), a, ns);
            emit(m.action_id(cur.data(), a), ok ? ns : nullptr);
            ++views;
        }
    return views;
}

// The model a host-side walk runs on: the original model under the canonical symmetry reduction
// (Canon<M> steps through orbit representatives; replay, the Explorer and discovery paths speak of
// concrete states of the original model) and under EvBits<M> (whose extra word is the search's
// bookkeeping), the model itself otherwise.
template <class M>
decltype(auto) base_model(const M& m) {
    if constexpr (is_canon<M>::value || is_evbits<M>::value) return m.base();
    else return (m);
}

// `Path::from_fingerprints` (src/checker/path.rs:20-86) over the states of a BFS-tree path (W words
// each): from the init state, each step is the FIRST action in `actions()` order whose successor is
// the next state. Under the canonical symmetry reduction (Canon<M>) the tree holds orbit
// representatives; the path is then made concrete in the original model: an init state whose
// representative is the first state, and at each step the first action whose successor's
// representative is the next one. Returns the number of actions; `raw` (optional) receives the
// concrete states (W words each), whose fingerprints are the discovery's chain.
template <class M>
int concrete_path(const M& m, const std::vector<u64>& st, std::vector<i64>& actions, std::vector<i64>& states,
                  std::vector<u64>* raw = nullptr) {
    constexpr int W = M::W;
    const size_t len = st.size() / W;
    if (!len) return -1;
    const int wd = m.describe_width();
    std::vector<u64> cur(st.begin(), st.begin() + W);
    if constexpr (is_canon<M>::value) {
        const std::vector<u64> inits = init_states_of(m.base());
        const int k = (int)(inits.size() / W);
        cur.clear();
        for (int i = 0; i < k && cur.empty(); ++i) {
            u64 c[W];
            m.base().canonical(&inits[i * W], c);
            if (std::equal(c, c + W, st.begin())) cur.assign(&inits[i * W], &inits[i * W] + W);
        }
        if (cur.empty()) throw Error(SR_ERR_NONDETERMINISM, "Unable to reconstruct a `Path`: no init state has the expected representative");
    }
    auto emit = [&](const u64* s) {
        const size_t o = states.size();
        states.resize(o + wd);
        m.describe(s, &states[o]);
        if (raw) raw->insert(raw->end(), s, s + W);
    };
    for (size_t i = 1; i < len; ++i) {
        const u64* target = &st[i * W];
        u64 mask[M::MW];
        m.enabled(cur.data(), mask);
        bool found = false;
        for (int w = 0; w < M::MW && !found; ++w)
            for (u64 bits = mask[w]; bits && !found; bits &= bits - 1) {
                const int a = w * 64 + __builtin_ctzll(bits);
                u64 ns[W];
                if (!m.apply(cur.data(), a, ns) || !std::equal(ns, ns + W, target)) continue;
                u64 next[W];
                if constexpr (is_canon<M>::value) m.base().apply(cur.data(), a, next);
                else std::copy(ns, ns + W, next);
                emit(cur.data());
                actions.push_back(m.action_id(cur.data(), a));
                cur.assign(next, next + W);
                found = true;
            }
        if (!found)
            throw Error(SR_ERR_NONDETERMINISM, "Unable to reconstruct a `Path`: " + std::to_string(i) +
                                                   " previous state(s) reconstructed but no successor is the next state");
    }
    emit(cur.data());
    return (int)actions.size();
}

// `reconstruct_path`'s fingerprint chain (src/checker/bfs.rs:314-342) of a BFS-tree path: the
// fingerprints of its states, or under Canon<M> of the concrete states of the original model that
// concrete_path walks (the ones `discovery_path`, `replay` and the Explorer speak of).
template <class M>
int fingerprint_chain(const M& m, const std::vector<u64>& st, std::vector<u64>& out) {
    constexpr int W = M::W;
    out.clear();
    std::vector<u64> raw;
    if constexpr (is_canon<M>::value) {
        std::vector<i64> actions, described;
        concrete_path(m, st, actions, described, &raw);
    } else {
        raw = st;
    }
    for (size_t i = 0; i < raw.size() / W; ++i) out.push_back(state_fp<M>(&raw[i * W]));
    return (int)out.size();
}

template <class M>
class Engine final : public EngineBase {
    static constexpr int W = M::W;
    static constexpr u32 WPB = (u32)expand_wpb<M>();  // expand_fast's waves per workgroup

  public:
    Engine(M m, const sr_opts& o)
        : m_(m), o_(o), A_((u32)m.max_actions()), D_((u32)m.max_out_degree()), emask_(model_emask(m)), lmask_(model_lmask(m)),
          smask_(step_checked_mask(m)) {
        disc.resize(M::NPROPS);
        if (emask_ & lmask_) throw Error(SR_ERR_ARG, "a leads-to property is in the model's emask()");
        if ((emask_ | lmask_) & smask_) throw Error(SR_ERR_ARG, "a step property is in the model's emask() or lmask()");
        (void)init_states_of(m_);  // a model with more init states than it declares fails at spawn
        if (o_.liveness) {  // the complete `eventually` check (live.hpp): what it cannot be combined with
            if (o_.target_state_count)
                throw Error(SR_ERR_UNSUPPORTED, "liveness with target_state_count: a partial reachable set makes the fixpoint unsound");
            if (is_canon<M>::value)
                throw Error(SR_ERR_UNSUPPORTED, "liveness with symmetry: the fixpoint runs on concrete states, not on orbit representatives");
            if (o_.capacity_hint > 0xffffffffull)
                throw Error(SR_ERR_UNSUPPORTED, "liveness with more than 2^32 - 1 unique states: the pass indexes the arena with 32 bits");
            if (o_.liveness == SR_LIVENESS_WEAK && !(fair_slots_model<M> && M::MW <= LIVE_MW_MAX))
                throw Error(SR_ERR_UNSUPPORTED, "weak fairness: this model's slots are not fairness classes");
            if (o_.liveness == SR_LIVENESS_STRONG && !(fair_slots_model<M> && M::MW <= LIVE_MW_MAX))
                throw Error(SR_ERR_UNSUPPORTED, "strong fairness: this model's slots are not fairness classes");
        }
        cover.c = cover_none();
        if (o_.coverage) {  // the coverage pass (cover.hpp): what it cannot be combined with
            if (o_.target_state_count)
                throw Error(SR_ERR_UNSUPPORTED, "coverage with target_state_count: the counts are over the whole reachable set");
            if (is_canon<M>::value)
                throw Error(SR_ERR_UNSUPPORTED, "coverage with symmetry: the counts would be over orbit representatives, not over states");
            (void)cover_checked_classes(m_);
            static_assert(cover_chunk_max<M>() >= 1, "coverage: an LDS counter must hold one stride");
        }
        // Internal tuning knobs (not part of the ABI): successors per lane per probe round and
        // the visited-set load factor the capacity hint is sized for.
        if (const char* e = std::getenv("SR_PROBE_BATCH")) probe_batch_ = std::atoi(e);
        if (const char* e = std::getenv("SR_TABLE_LOAD")) table_load_ = std::atof(e), load_env_ = true;
        if (const char* e = std::getenv("SR_PPW_LOG2")) ppw_env_ = std::atoi(e);
        if (const char* e = std::getenv("SR_FILTER_LOG2")) filt_log2_ = (u32)std::atoi(e);
        // The LDS duplicate filter must be injective on states (kernels.hpp filter_key): one-word
        // states in either mode; a multi-word quotient-mode table runs without it.
        if (!filter_exact(m_)) filt_log2_ = 0;
        // 4-byte entries where they are exact: twice the entries in the same LDS (SR_FILTER_COMPACT=0: off)
        if (filt_log2_ && (!std::getenv("SR_FILTER_COMPACT") || std::atoi(std::getenv("SR_FILTER_COMPACT"))) &&
            filter_compact_ok(m_, filt_log2_ + 1))
            filt_log2_ += 1, filt_compact_ = true;
        // residencies per expand grid (expand_grid_cap): one for one-word states, two otherwise
        // (profiles/r06_grid_cap.txt). SR_GRID_RES (measurement knob) overrides.
        grid_res_ = W == 1 ? 1u : 2u;
        if (const char* e = std::getenv("SR_GRID_RES"))
            if (std::atoi(e) > 0) grid_res_ = (u32)std::atoi(e);
        if (const char* e = std::getenv("SR_PIPELINE")) pipeline_ = std::atoi(e) != 0;
        if (const char* e = std::getenv("SR_QUERY_LOG2")) query_mask_ = (1ull << std::atoi(e)) - 1;
        if (const char* e = std::getenv("SR_GRID_MAX")) grid_env_ = (u32)std::max(0, std::atoi(e));  // <= 0: unset
        if (const char* e = std::getenv("SR_WIDE_NOPF")) wide_nopf_ = std::atoi(e) ? 1 : 0;
        if (const char* e = std::getenv("SR_CHAIN_MAX")) chain_max_ = (u64)std::max(0ll, std::atoll(e));
        if (const char* e = std::getenv("SR_TABLE_KIND")) table_kind_ = std::atoi(e);
        if (const char* e = std::getenv("SR_TABLE_RECYCLE")) table_recycle_ = std::atoi(e) != 0;
        if (const char* e = std::getenv("SR_BALANCE")) balance_ = std::atoi(e) != 0;
        if (const char* e = std::getenv("SR_BALANCE_MIN")) balance_min_ = (u64)std::max(0ll, std::atoll(e));
        // expand_fast's action table (kernels.hpp ActionTable): a model with `action_masks` whose slots
        // fit one per lane. SR_ACTION_TABLE=0 keeps `apply` (read per engine: tests run both in one process).
        action_table_ = action_table_model<M> && A_ <= 64;
        if (const char* e = std::getenv("SR_ACTION_TABLE")) action_table_ = action_table_ && std::atoi(e) != 0;
    }
    ~Engine() override = default;

    int nprops() const override { return M::NPROPS; }
    const char* prop_name(int p) const override { return m_.prop_name(p); }
    int expectation(int p) const override { return m_.expectation(p); }
    int width() const override { return m_.describe_width(); }
    std::string action_name(i64 id) const override { return m_.action_name(id); }

    void run() override {
        SR_HIP(hipSetDevice(o_.device));
        CtxLease lease(o_.device);
        bind(lease.c);
        int order = o_.order;
        if (order == SR_ORDER_AUTO) order = o_.target_state_count ? SR_ORDER_FIFO : SR_ORDER_FAST;
        // `eventually` discoveries depend on the visit order (which generator passes its bits on,
        // which terminal state overwrites), so by default such models run in the reference's
        // single-threaded FIFO order. An explicit FAST order is honoured: each state takes the
        // bits of the generator that claims it, as in one of the reference's multi-threaded
        // orders (`threads(n)`, src/checker/bfs.rs:75-152), and the discoveries are valid
        // counterexamples of that order (the reference's false negatives may differ).
        if (emask_ && o_.order != SR_ORDER_FAST) order = SR_ORDER_FIFO;
        bool order_dependent = run_with_restart(order);
        if (order_dependent && o_.order == SR_ORDER_AUTO && order == SR_ORDER_FAST) {
            // An early exit inside a level makes counts depend on the visit order: redo the
            // check in the reference's exact FIFO order.
            if (o_.verbose) std::fprintf(stderr, "[sr] early exit in FAST order; re-running in FIFO order\n");
            run_with_restart(SR_ORDER_FIFO);
        }
        bind(nullptr);
    }

    // Capacity planning is optimistic (a chunk is sized for twice the previous level's growth, not
    // for every successor being new). If a level ever outgrows it, the device reports a full table
    // or arena and the check restarts from scratch in the pessimistic mode with larger buffers.
    bool run_with_restart(int order) {
        for (int attempt = 0;; ++attempt) {
            try {
                return run_order(order);
            } catch (const Error& e) {
                if (e.code != SR_ERR_CAPACITY || attempt >= 3) throw;
                if (o_.verbose) std::fprintf(stderr, "[sr] %s; restarting with larger buffers\n", e.what());
                pessimistic_ = true;
                restarts_++;
                grow_factor_ *= 4;
                (void)stream_sync(stream_);
                rehash_pending_ = false;  // (a failed enqueued rehash is this restart's cause, or moot)
                retired_keys_.clear();
                retired_arena_.clear();
                retired_u32_.clear();
                init_counters();
            }
        }
    }

    // `reconstruct_path` (src/checker/bfs.rs:314-342): the discovery's fingerprint chain, found by
    // walking parent ranks back through the BFS-tree arena.
    int chain(int p, std::vector<u64>& out) override {
        out.clear();
        if (p < 0 || p >= M::NPROPS || !disc[p].found) return 0;
        if (!live_path_[p].empty()) return fingerprint_chain(m_, live_path_[p], out);  // (found by the liveness pass)
        SR_HIP(hipSetDevice(o_.device));
        std::vector<u64> st;
        tree_path(disc[p].level, disc[p].rank, st);
        return fingerprint_chain(m_, st, out);
    }

    // States (W words each) from the init state down to (level, rank).
    void tree_path(u32 level, u32 rank, std::vector<u64>& st) {
        std::vector<u64> idx;
        u64 r = rank;
        for (int d = (int)level;; --d) {
            u64 a = lstart_[d] + r;
            idx.push_back(a);
            if (d == 0) break;
            u32 pr = 0;
            SR_HIP(hipMemcpy(&pr, apar_.p + a, sizeof(u32), hipMemcpyDeviceToHost));
            r = pr;
        }
        std::reverse(idx.begin(), idx.end());
        st.resize(idx.size() * W);
        for (size_t i = 0; i < idx.size(); ++i)
            SR_HIP(hipMemcpy(&st[i * W], arena_.p + idx[i] * W, W * sizeof(u64), hipMemcpyDeviceToHost));
    }

    // `Path::from_fingerprints` (src/checker/path.rs:20-86) on the host copy of the GpuModel.
    int path(int p, std::vector<i64>& actions, std::vector<i64>& states) override {
        if (p < 0 || p >= M::NPROPS || !disc[p].found) return -1;
        if (!live_path_[p].empty()) {
            const int n = concrete_path(m_, live_path_[p], actions, states);
            // (a step property's witness: its last action is the seed's, not the first that leads to the last state)
            if (n > 0 && step_action_[p] >= 0) actions.back() = step_action_[p];
            return n;
        }
        SR_HIP(hipSetDevice(o_.device));
        std::vector<u64> st;
        tree_path(disc[p].level, disc[p].rank, st);
        return concrete_path(m_, st, actions, states);
    }

    i64 action_id_bound() const override { return m_.action_id_bound(); }
    int init_count() const override { return (int)(init_states_of(base_model(m_)).size() / std::decay_t<decltype(base_model(m_))>::W); }
    // replay and the Explorer walk concrete states of the original model (under Canon<M> too)
    int replay(int init, const i64* ids, int n, std::vector<i64>& states, std::vector<int>& conds,
               std::vector<int>* all_conds, int* terminal) const override {
        return replay_model(base_model(m_), init, ids, n, states, conds, all_conds, terminal);
    }
    int sink_kind(int init, const i64* ids, int n) const override { return sink_kind_model(base_model(m_), init, ids, n); }
    int loop_fair(int init, const i64* ids, int n, int loop_start, bool strong) const override {
        return loop_fair_model(base_model(m_), init, ids, n, loop_start, strong);
    }
    int triggers(int init, const i64* ids, int n, int p, std::vector<int>& out) const override {
        return triggers_model(base_model(m_), init, ids, n, p, out);
    }
    int step_replay(int init, const i64* ids, int n, int p) const override { return step_replay_model(base_model(m_), init, ids, n, p); }
    int explore(const u64* fps, int n, std::vector<i64>& action, std::vector<int>& has, std::vector<u64>& fp,
                std::vector<i64>& states) const override {
        return explore_model(base_model(m_), fps, n, action, has, fp, states);
    }

    // The visitor's paths (src/checker/bfs.rs:187-189 builds `Path::from_fingerprints` of every
    // popped state): each visited state's BFS-tree parent and the FIRST action, in `actions()`
    // order, that leads from the parent to it (src/checker/path.rs:55-79).
    bool visit_tree(std::vector<i64>& parent, std::vector<i64>& action) const override {
        parent.clear();
        action.clear();
        std::vector<u64> prev_states;
        i64 prev_base = 0;  // visit index of the previous level's first state
        for (size_t d = 0; d < lvisited_.size(); ++d) {
            const u64 nv = lvisited_[d];
            std::vector<u64> st(nv * W);
            std::vector<u32> par(nv);
            if (nv) {
                SR_HIP(hipMemcpy(st.data(), arena_.p + lstart_[d] * W, nv * W * sizeof(u64), hipMemcpyDeviceToHost));
                SR_HIP(hipMemcpy(par.data(), apar_.p + lstart_[d], nv * sizeof(u32), hipMemcpyDeviceToHost));
            }
            const i64 base = (i64)parent.size();
            for (u64 i = 0; i < nv; ++i) {
                if (d == 0) {
                    parent.push_back(-1);
                    action.push_back(-1);
                    continue;
                }
                const u64 pr = par[i];
                if (pr >= prev_states.size() / W) throw Error(SR_ERR_NONDETERMINISM, "visit parent outside the visited prefix");
                const u64* ps = &prev_states[pr * W];
                const u64 want = state_fp<M>(&st[i * W]);
                u64 mask[M::MW];
                m_.enabled(ps, mask);
                i64 id = -1;
                for (int w = 0; w < M::MW && id < 0; ++w)
                    for (u64 bits = mask[w]; bits && id < 0; bits &= bits - 1) {
                        const int a = w * 64 + __builtin_ctzll(bits);
                        u64 ns[W];
                        if (m_.apply(ps, a, ns) && state_fp<M>(ns) == want) id = m_.action_id(ps, a);
                    }
                if (id < 0) throw Error(SR_ERR_NONDETERMINISM, "Unable to reconstruct a `Path` for a visited state");
                parent.push_back(prev_base + (i64)pr);
                action.push_back(id);
            }
            prev_states.swap(st);
            prev_base = base;
        }
        return true;
    }

    std::vector<i64> visits() const override {
        const int wd = m_.describe_width();
        std::vector<u64> st;
        for (size_t d = 0; d < lvisited_.size(); ++d) {
            size_t o = st.size();
            st.resize(o + lvisited_[d] * W);
            if (lvisited_[d])
                SR_HIP(hipMemcpy(&st[o], arena_.p + lstart_[d] * W, lvisited_[d] * W * sizeof(u64), hipMemcpyDeviceToHost));
        }
        std::vector<i64> out(st.size() / W * wd);
        for (size_t i = 0; i < st.size() / W; ++i) m_.describe(&st[i * W], &out[i * wd]);
        return out;
    }

  private:
    TableView view() const { return make_table_view(m_, keys_.p, fifo_ ? meta_.p : nullptr, cap_); }

    // zero = false: the caller writes every slot (rehash_ranges), so no clear is enqueued.
    void alloc_table(u64 cap, bool zero = true) {
        cap_ = cap;
        lmax_ = max_load(cap);
        const u64 words = table_words(make_table_view(m_, nullptr, nullptr, cap), cap);
        table_unzeroed_ = false;
        if (zero) keys_.alloc_zero(o_.device, words, stream_, table_kind_);
        else keys_.alloc(o_.device, words, table_kind_);
        if (fifo_) {
            meta_.alloc(o_.device, cap);
            SR_HIP(hipMemsetAsync(meta_.p, 0xff, cap * sizeof(u64), stream_));
        }
    }

    // Doubles the visited set (quotient mode: one more displacement bit per slot, so twice the
    // probe limit). If an entry does not fit the new table's probe limit, the rehash starts over
    // from the old table into one twice as large again. In FIFO order the level's candidate slots
    // (cand) are remapped to the new table, since the rehash moves every entry.
    // min_slots: grow to at least this many slots (one rehash, however many doublings that is).
    void grow_table(u32* cand = nullptr, u64 cand_n = 0, u64 min_slots = 0) {
        check_async_growth();  // an earlier asynchronous rehash's outcome first (aux_ is reused)
        const auto tg = Clock::now();
        DBuf<u64> ok, om;
        ok.swap(keys_);
        if (fifo_) om.swap(meta_);
        const TableView from = make_table_view(m_, ok.p, fifo_ ? om.p : nullptr, cap_);
        const u64 old_cap = cap_;
        if (!aux_.p) aux_.alloc(o_.device, 2);
        u64 f0 = 2;
        while (old_cap * f0 < min_slots) f0 *= 2;
        for (u64 f = f0;; f *= 2) {
            launch_rehash(from, old_cap, f);
            u32 err = 0;
            SR_HIP(hipMemcpyAsync(&err, aux_.p, sizeof(u32), hipMemcpyDeviceToHost, stream_));
            SR_HIP(stream_sync(stream_));
            if (!err) break;
            if (f >= 64) throw Error(SR_ERR_CAPACITY, "rehash: probe limit exceeded at 64x the capacity");
        }
        if (cand && cand_n) {
            remap_slots<<<blocks_for(cand_n, 256), 256, 0, stream_>>>(cand, cand_n, from, view());
            SR_HIP(hipGetLastError());
        }
        SR_HIP(stream_sync(stream_));
        stats.rehashes++;
        if (o_.verbose)
            std::fprintf(stderr, "[sr] visited set %llu -> %llu slots in %.3f ms\n", (unsigned long long)old_cap,
                         (unsigned long long)cap_, secs(tg, Clock::now()) * 1e3);
    }

    // The same growth ENQUEUED behind the level in flight, without waiting for it (the early growth
    // of the pipelined loop, FAST order): the rehash reads the whole old table, so it needs nothing
    // from the host, and the next level is launched on the new table right behind it. The old table
    // is retired until the stream has passed the rehash (retire / release_retired), and the rehash's
    // error word is read at the next synchronous point (check_async_growth): an entry that did not
    // fit the new table fails the check with a capacity error, and the check restarts.
    void grow_table_async(u64 min_slots) {
        check_async_growth_pending_first();
        retired_keys_.emplace_back();
        retired_keys_.back().swap(keys_);
        const TableView from = make_table_view(m_, retired_keys_.back().p, nullptr, cap_);
        const u64 old_cap = cap_;
        if (!aux_.p) aux_.alloc(o_.device, 2);
        u64 f = 2;
        while (old_cap * f < min_slots) f *= 2;
        launch_rehash(from, old_cap, f);
        rehash_pending_ = true;
        stats.rehashes++;
        if (o_.verbose)
            std::fprintf(stderr, "[sr] visited set %llu -> %llu slots enqueued\n", (unsigned long long)old_cap,
                         (unsigned long long)cap_);
    }
    // Allocates the table of old_cap * f slots and enqueues the rehash of `from` into it (error bits
    // in aux_[0]): range by range without a clear (rehash_ranges + rehash_spill) when the new homes
    // of a range of old homes are a range (quotient mode, f = 2^(from.qbits - to.qbits)) and no meta
    // moves along (FAST order), else a clear plus one CAS insertion per entry (rehash).
    // SR_REHASH_RANGES=0 (measurement knob) always takes the latter.
    void launch_rehash(const TableView& from, u64 old_cap, u64 f) {
        const u64 cap = old_cap * f;
        sr::launch_rehash(
            from, old_cap, make_table_view(m_, nullptr, nullptr, cap), cap, rehash_ranges_,
            [&](bool ranges) {
                alloc_table(cap, !ranges);
                table_unzeroed_ = ranges;
                SR_HIP(hipMemsetAsync(aux_.p, 0, sizeof(u32), stream_));
                return view();
            },
            spill_, o_.device, aux_.p, stream_);
        // SR_REHASH_FAIL=k (tests): the k-th growth of this check reports a full table, by a store
        // to its error word enqueued behind the rehash; the new table itself is complete
        if (++growths_ == rehash_fail_) SR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(aux_.p), (int)ERR_TABLE_FULL, 1, stream_));
    }
    u32 table0_log2_ = std::getenv("SR_TABLE_LOG2") ? (u32)std::min(22, std::max(10, std::atoi(std::getenv("SR_TABLE_LOG2")))) : 22u;
    u64 growths_ = 0;  // rehashes launched by this check, restarts included
    u32 restarts_ = 0;  // capacity restarts of this check (sr_stats.restarts)
    u64 rehash_fail_ = std::getenv("SR_REHASH_FAIL") ? (u64)std::atoll(std::getenv("SR_REHASH_FAIL")) : 0u;
    bool rehash_ranges_ = !std::getenv("SR_REHASH_RANGES") || std::atoi(std::getenv("SR_REHASH_RANGES")) != 0;
    DBuf<u64> spill_;  // rehash_ranges' spill list: [0] count, then old slot indices
    // The visited set was built by rehash_ranges (allocated without a clear): released without one
    // too, since the next unhinted check grows into its tables the same way (a hinted check clears
    // what it takes).
    bool table_unzeroed_ = false;

    // (an asynchronous growth is enqueued only while none is pending)
    void check_async_growth_pending_first() {
        if (rehash_pending_) check_async_growth();
    }
    // The outcome of an enqueued rehash (waits for the stream) and the retired buffers released.
    void check_async_growth() {
        if (!rehash_pending_ && retired_keys_.empty() && retired_arena_.empty()) return;
        SR_HIP(stream_sync(stream_));
        retired_keys_.clear();
        retired_arena_.clear();
        retired_u32_.clear();
        if (!rehash_pending_) return;
        rehash_pending_ = false;
        u32 err = 0;
        SR_HIP(hipMemcpy(&err, aux_.p, sizeof(u32), hipMemcpyDeviceToHost));
        if (err) throw Error(SR_ERR_CAPACITY, "an enqueued rehash exceeded the new table's probe limit");
    }
    bool rehash_pending_ = false;
    std::vector<DBuf<u64>> retired_keys_, retired_arena_;
    std::vector<DBuf<u32>> retired_u32_;

    // Growth during a check (no capacity hint, or one too small: the path a user of the reference
    // gets, whose DashMap grows as it goes, src/checker/bfs.rs:26) takes a few large steps rather
    // than doublings: every growth stops the level pipeline, and a table growth rehashes every
    // entry. A step multiplies the size by SR_GROW_STEP (default 8), within a share of the free
    // device memory (never below what the level needs).
    u64 growth_slots(u64 need_slots) const {
        // the first growth of a check that started without a hint (the model has outgrown the
        // default table) takes a larger step, SR_GROW_FIRST (measurement knob; 0: grow_step_)
        const u64 step = !o_.capacity_hint && stats.rehashes == 0 && grow_first_ ? grow_first_ : grow_step_;
        u64 target = std::max<u64>(need_slots, cap_ * step);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) target = std::min<u64>(target, std::max<u64>(need_slots, free_b / 4 / 8));
        return target;
    }
    u64 grow_step_ = std::getenv("SR_GROW_STEP") && std::atoi(std::getenv("SR_GROW_STEP")) >= 2
                         ? (u64)std::atoi(std::getenv("SR_GROW_STEP")) : 8u;
    u64 grow_first_ = std::getenv("SR_GROW_FIRST") ? (u64)std::atoi(std::getenv("SR_GROW_FIRST")) : 0u;

    // The growth threshold of the visited set: 0.8 load, or lower for a quotient-mode table whose
    // probe limit (set by its displacement bits) would otherwise be reached by the longest
    // linear-probe run to be expected at that load (kernels.hpp max_load_for).
    double max_load(u64 cap) const {
        const TableView v = make_table_view(m_, nullptr, nullptr, cap, true);
        return max_load_for(v.plimit, (double)cap, 0.8);
    }

    // sr_stats.max_displacement / displacement_limit of the final table (the scan runs only in a
    // measurement pass, sr_opts.counters: it reads the whole table).
    void displacement_stats() {
        const TableView v = view();
        stats.displacement_limit = v.plimit;
        stats.table_encoding = table_encoding_word(v, filt_log2_, filt_compact_);
        if (!o_.counters || !cap_) return;
        if (!aux_.p) aux_.alloc(o_.device, 2);
        SR_HIP(hipMemsetAsync(aux_.p + 1, 0, sizeof(u32), stream_));
        const u32 grid = (u32)std::min<u64>(blocks_for(cap_, 256), 8192);
        table_max_disp<<<grid, 256, 0, stream_>>>(v, cap_, aux_.p + 1);
        SR_HIP(hipGetLastError());
        u32 d = 0;
        SR_HIP(hipMemcpyAsync(&d, aux_.p + 1, sizeof(u32), hipMemcpyDeviceToHost, stream_));
        SR_HIP(stream_sync(stream_));
        stats.max_displacement = d;
    }

    // The visited-set audit (kernels_audit.hpp) of the final table against the arena's
    // lstart_.back() states; a measurement pass like the scan above (sr_opts.counters).
    void table_audit() {
        if (!o_.counters || !cap_ || !keys_.p) return;
        const u64 n = lstart_.back();
        DBuf<u64> acc, ls;
        DBuf<u32> marks;
        acc.alloc(o_.device, sizeof(AuditCounters) / 8);
        ls.alloc(o_.device, lstart_.size());
        marks.alloc(o_.device, (size_t)((cap_ + 31) / 32));
        SR_HIP(hipMemsetAsync(acc.p, 0, sizeof(AuditCounters), stream_));
        SR_HIP(hipMemcpyAsync(ls.p, lstart_.data(), lstart_.size() * sizeof(u64), hipMemcpyHostToDevice, stream_));
        AuditCounters* a = reinterpret_cast<AuditCounters*>(acc.p);
        launch_audit_table(view(), cap_, marks.p, a, stream_);
        launch_audit_arena(m_, view(), arena_.p, fifo_ ? apar_.p : nullptr, n, ls.p, (u32)lstart_.size() - 1, A_, marks.p, a,
                           stream_);
        AuditCounters h{};
        SR_HIP(hipMemcpyAsync(&h, acc.p, sizeof(h), hipMemcpyDeviceToHost, stream_));
        SR_HIP(stream_sync(stream_));
        audit = sr_table_audit{1u, fifo_ ? 1u : 0u, cap_, h.occupied, h.misplaced, h.duplicates, h.arena_states,
                               h.arena_missing, h.arena_shared, h.meta_wrong};
    }

    // The BFS-tree arena holds every level's states (visit order) and their parent ranks; grows
    // by copying the used prefix.
    // async: the copy is enqueued behind the work in flight and the old buffers retired until the
    // stream has passed it (check_async_growth), instead of waiting here.
    // The arena's growth step (SR_ARENA_STEP; default 8 for states of <= 2 words, 4 for wider ones, as
    // every model until round 6): unhinted 2pc N=10 8.17-8.24 -> 7.93-8.00 ms, increment_lock N=11
    // 33.9-35.0 -> 32.5-33.3; paxos C=6 (W = 12) 3.02-3.04 -> 3.20-3.21 with 8, so it keeps 4
    // (profiles/r06_arena_step.txt).
    u64 arena_step_ = std::getenv("SR_ARENA_STEP") && std::atoi(std::getenv("SR_ARENA_STEP")) >= 2
                          ? (u64)std::atoi(std::getenv("SR_ARENA_STEP")) : W <= 2 ? 8u : 4u;
    void ensure_arena(u64 states, u64 used, bool async = false) {
        if (arena_cap_ >= states) return;
        const auto ta = Clock::now();
        // (each growth step copies the arena so far and stops the level pipeline; a step never takes
        // more than half the device's free memory, nor less than `states`)
        u64 cap = std::max<u64>(states, arena_cap_ * (arena_cap_ ? arena_step_ : 1));
        if (cap > states) {
            size_t fr = 0, tot = 0;
            const u64 per = W * sizeof(u64) + sizeof(u32) + (emask_ ? sizeof(u32) : 0);
            if (hipMemGetInfo(&fr, &tot) == hipSuccess) cap = std::max<u64>(states, std::min<u64>(cap, fr / 2 / per));
            else (void)hipGetLastError();
        }
        DBuf<u64> na;
        DBuf<u32> np, ne;
        na.alloc(o_.device, cap * W);
        np.alloc(o_.device, cap);
        if (emask_) ne.alloc(o_.device, cap);
        const double alloc_ms = secs(ta, Clock::now()) * 1e3;
        if (used) {
            SR_HIP(hipMemcpyAsync(na.p, arena_.p, used * W * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
            SR_HIP(hipMemcpyAsync(np.p, apar_.p, used * sizeof(u32), hipMemcpyDeviceToDevice, stream_));
            if (emask_) SR_HIP(hipMemcpyAsync(ne.p, aeb_.p, used * sizeof(u32), hipMemcpyDeviceToDevice, stream_));
        }
        const bool had = arena_.p != nullptr;
        arena_.swap(na);
        apar_.swap(np);
        if (emask_) aeb_.swap(ne);
        arena_cap_ = cap;
        // the old buffers go back to the pool when na/np/ne leave scope: wait until no enqueued work
        // reads them (a first allocation has none, and the start of a check does not wait here)
        if (had && async) {
            retired_arena_.emplace_back();
            retired_arena_.back().swap(na);
            retired_u32_.emplace_back();
            retired_u32_.back().swap(np);
            retired_u32_.emplace_back();
            retired_u32_.back().swap(ne);
        } else if (had) {
            SR_HIP(stream_sync(stream_));
        }
        if (o_.verbose && had)
            std::fprintf(stderr, "[sr] arena -> %llu states (%llu copied) in %.3f ms (allocation %.3f ms)\n",
                         (unsigned long long)cap, (unsigned long long)used, secs(ta, Clock::now()) * 1e3, alloc_ms);
    }

    void bind(Ctx* c) {
        ctx_ = c;
        stream_ = c ? c->stream : nullptr;
        lc_d_ = c ? c->lc : nullptr;
    }

    // Device counters to their level-start values (once per run; afterwards the publishing
    // workgroup of each level resets them).
    void init_counters() {
        if (!slots_.p) slots_.alloc(o_.device, (SLOTS * sizeof(LevelCounters) + 7) / 8);
        init_level_counters<<<1, 256, 0, stream_>>>(lc_d_, reinterpret_cast<LevelCounters*>(slots_.p), SLOTS);
        SR_HIP(hipGetLastError());
        slot_k_ = 0;
        slot_published_ = true;
    }

    // Per-level counter slots of the pipelined loop (SlotWork, kernels.hpp).
    LevelCounters* slot(u32 k) const { return reinterpret_cast<LevelCounters*>(slots_.p) + (k % SLOTS); }
    // The slot duties of the next slotted launch: its frontier size from the previous slot (dev_n),
    // the previous slot's publish unless it is already done, and the reset of slot K-2.
    SlotWork slot_work(bool dev_n) {
        SlotWork sw{};
        if (dev_n) sw.prev_n = slot_k_ ? &slot(slot_k_ - 1)->claims : &lc_d_->prev_claims;
        if (slot_k_ && !slot_published_) {
            sw.pub = slot(slot_k_ - 1);
            sw.hc = hcd(slot_seq_);
            sw.seq = slot_seq_;
            slot_published_ = true;
        }
        if (slot_k_ >= 2) sw.zero = slot(slot_k_ - 2);
        return sw;
    }
    // The last slotted level's publish, when no launch that would carry it is enqueued before the
    // host waits for it.
    void publish_pending_slot() {
        if (slot_published_) return;
        SlotWork sw{};
        sw.pub = slot(slot_k_ - 1);
        sw.hc = hcd(slot_seq_);
        sw.seq = slot_seq_;
        slot_publish_kernel<M::NPROPS><<<1, 64, 0, stream_>>>(sw);
        SR_HIP(hipGetLastError());
        slot_published_ = true;
    }
    u32 next_seq() { return ++ctx_->seq; }
    HostCounters* hcd(u32 seq) const { return ctx_->hc_dev + (seq & 1); }  // device view of seq's mirror

    // Waits until the launch tagged `seq` has published its counters to pinned host memory: a
    // spin on one host word (no stream synchronisation, no copy), with a periodic stream query
    // so that a failed launch cannot hang the host.
    // recoverable: a level that overflowed the visited set's probe limit (and nothing else) returns
    // false instead of throwing; the caller doubles the table and repairs the level.
    bool wait_publish(u32 seq, bool recoverable = false) {
        volatile u32* flag = &ctx_->hc[seq & 1].seq;
        for (u64 spin = 1;; ++spin) {
            if (*flag == seq) break;
            if ((spin & query_mask_) == 0) {
                hipError_t e = hipStreamQuery(stream_);
                if (e != hipSuccess && e != hipErrorNotReady) SR_HIP(e);
                if (e == hipSuccess && *flag != seq) {
                    if (*flag == seq) break;
                    throw Error(SR_ERR_HIP, "launch finished without publishing its counters");
                }
            }
            _mm_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        std::memcpy(&lc_, (const void*)&ctx_->hc[seq & 1], sizeof(lc_));
        if (lc_.err & ERR_MODEL) throw Error(SR_ERR_UNSUPPORTED, model_fault_text(m_));  // (no restart helps)
        if (recoverable && (lc_.err == ERR_TABLE_FULL || lc_.err == ERR_DEFERRED)) return false;
        if (lc_.err & ERR_TABLE_FULL) throw Error(SR_ERR_CAPACITY, "visited set probe limit exceeded");
        if (lc_.err & ERR_DEFERRED) throw Error(SR_ERR_CAPACITY, "deferred level");
        if (lc_.err & ERR_FRONTIER_OVERFLOW) throw Error(SR_ERR_CAPACITY, "frontier overflow");
        return true;
    }

    // A level (frontier of n states at arena offset fbase) whose expansion overflowed the visited
    // set's probe limit: its successors were all counted, but some were neither found nor claimed.
    // The table is doubled (quotient mode: one more displacement bit, twice the probe limit) and
    // the level is expanded again in repair mode on the larger table: every successor is probed
    // again, the states still missing are claimed and appended after the ones the first pass
    // appended, and no successor is counted twice. A launch enqueued behind the failed level saw
    // its err word and expanded nothing. lc_ holds the failed pass's counters on entry and the
    // level's complete counters on return (the slot ring starts over).
    void repair_level(u64 fbase, u64 n, u32 undiscovered) {
        const HostCounters first = lc_;
        u32 dmin[MAX_PROPS];  // discoveries among the states appended by every pass, failed ones too
        std::copy(first.disc, first.disc + MAX_PROPS, dmin);
        for (int attempt = 0;; ++attempt) {
            if (attempt >= 8) throw Error(SR_ERR_CAPACITY, "visited set probe limit exceeded after 8 doublings");
            SR_HIP(stream_sync(stream_));
            if (o_.verbose)
                std::fprintf(stderr, "[sr] level of %llu states overflowed the probe limit %u at %llu slots: doubling\n",
                             (unsigned long long)n, view().plimit, (unsigned long long)cap_);
            grow_table();
            stats.table_doublings++;
            const u32 partial = lc_.claims;
            init_counters();  // the slot ring starts over: slot 0 continues the level's frontier cursor
            SR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&slot(0)->claims), (int)partial, 1, stream_));
            const u32 sq = launch_expand(fbase, (u32)n, false, n, undiscovered, SLOT_REPAIR);
            publish_pending_slot();
            const bool ok = wait_publish(sq, true);
            for (int p = 0; p < MAX_PROPS; ++p) dmin[p] = std::min(dmin[p], lc_.disc[p]);
            if (ok) break;
        }
        // successors and enabled slots: the first pass counted them all; claims: the repair's cursor
        lc_.successors = first.successors;
        lc_.enabled = first.enabled;
        lc_.probes += first.probes;
        lc_.cas += first.cas;
        std::copy(dmin, dmin + MAX_PROPS, lc_.disc);
    }

    // Launch bracketed by pooled events (profile=1); durations are summed once at the end of the
    // run, so timing adds no synchronisation to the level loop.
    template <class F>
    void timed(F&& launch, u64 frontier = 0) {
        size_t i = 2 * stats.expand_launches;
        if (o_.profile) SR_HIP(hipEventRecord(ctx_->event(i), stream_));
        launch();
        SR_HIP(hipGetLastError());
        if (o_.profile) SR_HIP(hipEventRecord(ctx_->event(i + 1), stream_));
        stats.expand_launches++;
        launch_frontier.push_back(frontier);
        launch_probes.push_back(0);
        launch_cas.push_back(0);
    }
    void collect_timing() {
        if (!o_.profile || !stats.expand_launches) return;
        SR_HIP(hipEventSynchronize(ctx_->event(2 * stats.expand_launches - 1)));
        double ms = 0;
        launch_ms.assign(stats.expand_launches, 0.0);
        for (u64 i = 0; i < stats.expand_launches; ++i) {
            float t = 0;
            SR_HIP(hipEventElapsedTime(&t, ctx_->event(2 * i), ctx_->event(2 * i + 1)));
            ms += t;
            launch_ms[i] = t;
        }
        stats.expand_kernel_ms = ms;
    }

    // Returns true when the run stopped early inside a level in an order-dependent way.
    bool run_order(int order) {
        auto t_start = Clock::now();
        fifo_ = order == SR_ORDER_FIFO;
        state_count = 0;
        unique = 0;
        max_depth = 0;
        for (auto& d : disc) d = DiscoveryRec{};
        live.clear();
        live_weak.clear();
        live_strong.clear();
        live_leads.clear();
        live_path_.assign(M::NPROPS, {});
        step.clear();
        step_action_.assign(M::NPROPS, -1);
        cover = CoverFigures{};
        cover.c = cover_none();
        stats = sr_stats{};
        stats.words_per_state = W;
        stats.order_used = (u32)order;
        stats.restarts = restarts_;
        audit = sr_table_audit{};
        cert = cert_none();
        launch_ms.clear();
        launch_frontier.clear();
        launch_probes.clear();
        launch_cas.clear();
        seq_launch_.clear();

        // Visited set sized for <= table_load_ load at the hinted unique count.
        // (without a hint: 2^22 slots, 32 MiB, a few us to clear and recycled between checks; the
        // table then grows in steps of SR_GROW_STEP)
        // SR_TABLE_LOG2 (tests, 10..22): a smaller first table, so that a small model grows it
        u64 cap = std::max<u64>((1ull << table0_log2_) * grow_factor_, min_table_cap(m_));
        // Hints beyond 2^31 states (increment_lock N=12: 5.2e9) size the table for <= 0.75 load and
        // the arena with 30% slack, so that table + arena fit one MI355X's 288 GB.
        const bool huge = o_.capacity_hint > (1ull << 31);
        const double load = huge && !load_env_ ? 0.75 : table_load_;
        // (a quotient-mode table also stays under the load its probe limit allows, max_load)
        if (o_.capacity_hint)
            while ((double)cap * std::min(load, max_load(cap)) < (double)o_.capacity_hint * grow_factor_) cap <<= 1;
        ratio_ = (double)D_;
        nratio_ = 0;
        en_ratio_ = std::max(1.0, (double)D_ / 2.0);
        alloc_table(cap);

        // Init states (bfs.rs:43-66): all of them are counted and queued (duplicates too), the
        // visited set keeps distinct ones; `pending` pops from the back, so level 0 is visited in
        // REVERSE init order.
        const std::vector<u64> f0 = init_states_of(m_);
        const int k = (int)(f0.size() / W);
        std::vector<u64> rev(k * W);
        for (int i = 0; i < k; ++i) std::copy(&f0[i * W], &f0[i * W] + W, &rev[(k - 1 - i) * W]);
        arena_cap_ = 0;
        // hinted: room for every state plus one level's worth of planning slack (a regrowth copies
        // the whole arena mid-run)
        const u64 slack = huge ? o_.capacity_hint / 10 * 3 : o_.capacity_hint / 2;
        // (without a hint: 2^24 words, 128 MiB + its parent ranks, never cleared and pooled across
        // checks, so that the early table growth needs no arena copy behind it: 2pc N=9 fits)
        const u64 arena0 = o_.capacity_hint ? (1u << 22) / W : (1u << 24) / W;
        ensure_arena(std::max<u64>(std::max<u64>(1u << 16, arena0), (o_.capacity_hint + slack + 1024) * grow_factor_), 0);
        lstart_.assign({0, (u64)k});
        lvisited_.clear();
        const u32 und0 = ((1u << M::NPROPS) - 1) & ~emask_ & ~lmask_ & ~smask_;  // (no kernel of the search sees a leads-to or a step bit)
        u32 sq = 0;
        if ((u64)k * W <= ROOTS_INLINE_WORDS) {
            // one launch: counters reset, level 0 into the arena (no parents; `eventually` bits
            // pending, bfs.rs:52-60), roots inserted and evaluated, published
            InlineStates init{};
            std::copy(rev.begin(), rev.end(), init.w);
            if (!slots_.p) slots_.alloc(o_.device, (SLOTS * sizeof(LevelCounters) + 7) / 8);
            slot_k_ = 0;
            slot_published_ = true;
            sq = next_seq();
            stats.root_path = SR_ROOTS_INLINE;
            roots_start<M><<<1, 256, 0, stream_>>>(m_, view(), init, (u32)k, arena_.p, apar_.p, emask_ ? aeb_.p : nullptr,
                                                   emask_, lc_d_, reinterpret_cast<LevelCounters*>(slots_.p), SLOTS,
                                                   und0, hcd(sq), sq);
        } else {
            SR_HIP(hipMemcpyAsync(arena_.p, rev.data(), rev.size() * sizeof(u64), hipMemcpyHostToDevice, stream_));
            SR_HIP(hipMemsetAsync(apar_.p, 0xff, (size_t)k * sizeof(u32), stream_));
            init_counters();
            if (emask_) fill_u32<<<blocks_for(k, 64), 64, 0, stream_>>>(aeb_.p, (u32)k, emask_);  // bfs.rs:52-60
            sq = next_seq();
            stats.root_path = k <= 256 ? SR_ROOTS_FUSED : SR_ROOTS_LAUNCHES;
            if (k <= 256) {
                roots_fused<M><<<1, 256, 0, stream_>>>(m_, view(), arena_.p, (u32)k, lc_d_, und0, hcd(sq), sq);
            } else {
                insert_roots<M><<<blocks_for(k, 64), 64, 0, stream_>>>(m_, view(), arena_.p, (u32)k, lc_d_);
                eval_roots<M><<<blocks_for(k, 64), 64, 0, stream_>>>(m_, arena_.p, (u32)k, lc_d_, und0);
                publish_kernel<<<1, 64, 0, stream_>>>(lc_d_, hcd(sq), sq, 1, nullptr);
            }
        }
        SR_HIP(hipGetLastError());
        // FAST pipelined order: level 0 is enqueued before the host reads the roots' outcome (it is
        // ignored if the roots already discover every property)
        // (a model with leads-to properties takes the level loop below: its host mask differs from the kernels')
        const bool pipelined = !fifo_ && !emask_ && !lmask_ && !smask_ && !o_.target_state_count && M::NPROPS > 0 && pipeline_;
        const u32 sq_level0 = pipelined ? launch_sync((u64)k, (1u << M::NPROPS) - 1) : 0u;
        wait_publish(sq);
        state_count = (u64)k;
        unique = lc_.claims;

        // A leads-to property is decided by the liveness pass alone: with the pass on, the host keeps its bit, so
        // that the search explores everything as for an undiscovered `always`; with it off the bit is dropped and
        // the search stops as if the property were absent.
        // A step property is decided by the step pass alone (step.hpp), which needs every state of a one-GPU search
        // over concrete states: the host keeps its bit likewise, unless the check has a target_state_count or runs
        // on orbit representatives; then the property is left unchecked.
        const u32 step_on = o_.target_state_count || is_canon<M>::value ? 0u : smask_;
        u32 undiscovered = ((1u << M::NPROPS) - 1) & ~(o_.liveness ? 0u : lmask_) & ~(smask_ & ~step_on);
        // A model whose properties are all leads-to, with the pass off, has nothing for the search to await: it is
        // a model without properties (below: the first pop returns, bfs.rs:226), not an early exit inside a level.
        const bool no_props = M::NPROPS == 0 || undiscovered == 0;
        u64 n = (u64)k, popped_before = 0;
        u32 level = 0;
        bool order_dependent = false;
        bool explored_all = false;  // every level was expanded whole and the last one produced nothing
        bool cover_all = false;     // the same for the pipelined loop (which the liveness pass never follows)
        auto t_loop = Clock::now();
        if (pipelined) {
            order_dependent = pipeline_levels(n, sq_level0);
            cover_all = !order_dependent;  // (it returns true whenever it stopped with every property discovered)
        } else for (;;) {
            // 1. Discoveries among this level's states (evaluated when they were produced).
            u32 newly = 0, max_rank = 0;
            for (int p = 0; p < M::NPROPS; ++p)
                if ((undiscovered >> p & 1) && lc_.disc[p] != ~0u) {
                    newly |= 1u << p;
                    max_rank = std::max(max_rank, lc_.disc[p]);
                    disc[p].found = true;
                    disc[p].level = level;
                    disc[p].rank = lc_.disc[p];
                }
            // `eventually` properties: the first terminal candidate of each undiscovered one.
            const u32 eund = undiscovered & emask_;
            std::vector<u32> evf(M::NPROPS, ~0u);
            DBuf<u32> tsat, evd;
            if (emask_ && n) {
                tsat.alloc(o_.device, n);
                evd.alloc(o_.device, 2 * M::NPROPS);  // [first terminal candidate | last terminal + 1]
                SR_HIP(hipMemsetAsync(evd.p, 0xff, M::NPROPS * sizeof(u32), stream_));
                SR_HIP(hipMemsetAsync(evd.p + M::NPROPS, 0, M::NPROPS * sizeof(u32), stream_));
                ev_scan<M><<<blocks_for(n, 256), 256, 0, stream_>>>(m_, cur(), aeb_.p + lstart_[level], (u32)n, eund,
                                                                    emask_, tsat.p, evd.p);
                SR_HIP(hipGetLastError());
                SR_HIP(hipMemcpyAsync(evf.data(), evd.p, M::NPROPS * sizeof(u32), hipMemcpyDeviceToHost, stream_));
                SR_HIP(stream_sync(stream_));
            }
            u64 limit = n, visited = n;
            bool stop = false;
            if (no_props) {
                limit = 0;
                visited = std::min<u64>(1, n);
                stop = true;
            } else if (undiscovered == 0) {
                // Every property was discovered at a terminal state of the previous level: the next
                // pop finds nothing to await and returns (bfs.rs:226).
                limit = 0;
                visited = std::min<u64>(1, n);
                stop = true;
                order_dependent = true;
            } else {
                // The first pop at which every property is discovered: always/sometimes ones at the
                // pop of their discovering state, eventually ones right after their terminal state.
                const u32 pop_und = undiscovered & ~emask_;
                bool all = (newly & pop_und) == pop_und;
                u64 at = newly ? (u64)max_rank : 0;
                for (u32 e = eund; e; e &= e - 1) {
                    const int p = __builtin_ctz(e);
                    if (evf[p] == ~0u) all = false;
                    else at = std::max<u64>(at, (u64)evf[p] + 1);
                }
                if (all && at < n) {
                    // The pop of rank `at` finds every property discovered: check_block returns
                    // without expanding it (bfs.rs:226) and the worker shuts down (bfs.rs:121-128).
                    limit = at;
                    visited = at + 1;
                    stop = true;
                    order_dependent = true;
                }
            }
            undiscovered &= ~newly;

            // 2. target_state_count: the reference checks it after each 1500-pop block (bfs.rs:113-135).
            bool target_stop = false;
            if (o_.target_state_count && state_count + limit * D_ >= o_.target_state_count) {
                u64 lt = target_limit(n, popped_before, limit);
                if (lt != ~0ull) {
                    limit = lt;
                    visited = lt;
                    target_stop = true;
                    stop = true;
                    order_dependent = true;
                }
            }

            lvisited_.push_back(visited);

            // 3. Expand ranks [0, limit) (eventually: the bits passed on, terminal discoveries).
            u64 produced = 0;
            DBuf<u32> peb;
            std::vector<u32> evl(M::NPROPS, 0);
            if (emask_ && limit) {
                peb.alloc(o_.device, limit);
                ev_resolve<<<blocks_for(limit, 256), 256, 0, stream_>>>(tsat.p, aeb_.p + lstart_[level], (u32)limit, eund,
                                                                       evd.p, peb.p, evd.p + M::NPROPS);
                SR_HIP(hipGetLastError());
                SR_HIP(hipMemcpyAsync(evl.data(), evd.p + M::NPROPS, M::NPROPS * sizeof(u32), hipMemcpyDeviceToHost, stream_));
                SR_HIP(stream_sync(stream_));
            }
            if (limit) {
                produced = expand_level(level, n, limit, undiscovered & ~emask_ & ~lmask_ & ~smask_, peb.p);
            } else {
                std::memset(&lc_, 0, sizeof(lc_));
            }
            for (int p = 0; p < M::NPROPS; ++p) {
                if (!evl[p]) continue;  // discoveries.insert at a terminal state (bfs.rs:265-272)
                disc[p].found = true;
                disc[p].level = level;
                disc[p].rank = evl[p] - 1;
                undiscovered &= ~(1u << p);
            }
            state_count += lc_.successors;
            unique += lc_.claims;
            stats.successors += lc_.successors;
            stats.probes += lc_.probes;
            stats.cas += lc_.cas;
            stats.algorithmic_bytes += limit * 8 * W + lc_.successors * 8 + (u64)lc_.claims * (16 + 8 * W);
            stats.levels++;
            if (produced) max_depth = level + 1;
            if (o_.verbose)
                std::fprintf(stderr, "[sr] level %u: frontier %llu expanded %llu succ %llu new %llu unique %llu cap %llu\n",
                             level, (unsigned long long)n, (unsigned long long)limit,
                             (unsigned long long)lc_.successors, (unsigned long long)produced,
                             (unsigned long long)unique.load(), (unsigned long long)cap_);
            popped_before += visited;
            if (stop || produced == 0) {
                if (target_stop) reference_done = false;  // the worker returns without waiting
                else if (stop) reference_done = true;     // all properties discovered
                else  // exhausted: the last (partial) block still checks the target (bfs.rs:129-135)
                    reference_done = !(o_.target_state_count && state_count >= o_.target_state_count);
                explored_all = !stop;
                break;
            }
            lstart_.push_back(lstart_.back() + produced);
            n = produced;
            ++level;
        }
        auto t_end = Clock::now();
        collect_timing();
        displacement_stats();
        table_audit();
        if (o_.certify) certify_pass(explored_all || cover_all);  // (reads the visited set: before its release)
        stats.level_loop_sec = secs(t_loop, t_end);
        stats.total_sec = secs(t_start, t_end);
        stats.table_capacity = cap_;
        if (o_.liveness && explored_all) live_pass();  // (reads the visited set: before its release)
        if (o_.coverage && (explored_all || cover_all)) cover_pass();  // (reads the arena only)
        if (step_on && explored_all) step_pass();                     // (likewise)
        release_table();  // (the pipelined loop released it already)
        free_unzeroed_table();
        return order_dependent && !fifo_;
    }

    // FAST order without `eventually` properties or a target count: the expansion of level L+1 is
    // enqueued while level L still runs (its frontier size is read on the device: the claims of the
    // last resetting publish), so the GPU does not idle while the host digests a level. The host
    // keeps one level in flight beyond the one it waits for. A speculative launch is skipped when
    // the visited set or the arena might not hold it (that level is then launched after the wait,
    // sized exactly). A speculative level launched past the end (an exhausted frontier or an early
    // exit) is ignored. Returns whether the run stopped early inside a level.
    bool pipeline_levels(u64 n, u32 sq_level0) {
        u32 undiscovered = (1u << M::NPROPS) - 1;
        u32 level = 0;
        bool order_dependent = false;
        auto discoveries_of = [&](u32 lvl, const HostCounters& c, u32& max_rank) {
            u32 newly = 0;
            for (int p = 0; p < M::NPROPS; ++p)
                if ((undiscovered >> p & 1) && c.disc[p] != ~0u) {
                    newly |= 1u << p;
                    max_rank = std::max(max_rank, c.disc[p]);
                    disc[p].found = true;
                    disc[p].level = lvl;
                    disc[p].rank = c.disc[p];
                }
            return newly;
        };
        u32 max_rank = 0;
        u32 newly = discoveries_of(0, lc_, max_rank);  // among the init states (roots publish)
        undiscovered &= ~newly;
        if (newly && undiscovered == 0) {
            lvisited_.push_back(max_rank + 1);
            reference_done = true;
            drain();  // the level-0 launch is not counted
            return true;
        }
        // One level's outcome (counters c); false when the check is over.
        auto account = [&](const HostCounters& c, const char* how) -> bool {
            const u64 produced = c.claims;
            state_count += c.successors;
            unique += produced;
            stats.successors += c.successors;
            stats.probes += c.probes;
            stats.cas += c.cas;
            stats.algorithmic_bytes += n * 8 * W + c.successors * 8 + produced * (16 + 8 * W);
            stats.levels++;
            ratio_ = (double)produced / (double)n;
            note_ratio(ratio_);
            en_ratio_ = std::max(1.0, (double)c.enabled / (double)n);
            lvisited_.push_back(n);
            if (o_.verbose)
                std::fprintf(stderr, "[sr] level %u: frontier %llu succ %llu new %llu unique %llu cap %llu%s at %.3f ms\n", level,
                             (unsigned long long)n, (unsigned long long)c.successors, (unsigned long long)produced,
                             (unsigned long long)unique.load(), (unsigned long long)cap_, how, secs(vt0_, Clock::now()) * 1e3);
            if (produced == 0) {  // exhausted (a speculative launch saw an empty frontier)
                reference_done = true;
                return false;
            }
            max_depth = level + 1;
            lstart_.push_back(lstart_.back() + produced);
            n = produced;
            ++level;
            max_rank = 0;
            newly = discoveries_of(level, c, max_rank);
            undiscovered &= ~newly;
            if (newly && undiscovered == 0) {
                // every property discovered inside this level: the reference stops at that pop
                // (order-dependent in FAST order; AUTO re-runs FIFO). A speculative expansion of
                // this level is not counted.
                lvisited_.push_back(max_rank + 1);
                reference_done = true;
                order_dependent = true;
                return false;
            }
            return true;
        };
        u32 sq = sq_level0;  // enqueued before the roots' outcome was read
        // Launches enqueued beyond the one waited for, in level order: one (the next level, its
        // frontier size read on the device), or two while the levels are small (the second CHAINED:
        // its frontier's offset is read on the device too). A level the host has to read before the
        // next is enqueued costs the host's turnaround (its publish seen, the launch issued: ~10-15
        // us) whenever the level in flight is shorter than that, which small levels are.
        std::deque<u32> ahead;
        vt0_ = Clock::now();
        for (;;) {
            const double g = std::max(ratio_, 1.0) * 1.5;
            const u64 est1 = (u64)((double)n * g) + 1024;     // the next frontier
            const u64 est2 = (u64)((double)est1 * g) + 1024;  // the states it will claim (= the frontier after)
            const u64 est3 = (u64)((double)est2 * g) + 1024;  // ... and those that one will claim
            const u64 nb_next = lstart_.back();
            // launch shape: a tight estimate (the grid strides over any excess)
            const u64 shape = (u64)((double)n * std::max(ratio_, 0.05) * 1.1) + 64;
            // Early growth (no capacity hint): a visited set that the next three levels
            // are projected to outgrow is grown now, while the level in flight is small. The rehash
            // then moves few entries and the stop costs one small level's latency, instead of both
            // at the first level that no longer fits (2pc N=9: ~1 M entries and a pipeline stop at
            // level 9, 0.1 ms per check).
            if (ahead.empty() && !pessimistic_ && !o_.capacity_hint && n <= early_grow_max_ &&
                (double)(unique + est1 + est2 + est3) >= lmax_ * (double)cap_) {
                // (enqueued behind the level in flight: no host wait; the whole old arena is copied,
                // since the host does not know yet how much of it that level fills)
                const u64 want = unique + est1 + est2 + est3;
                grow_table_async(growth_slots((u64)((double)want / lmax_) + 1));
                // (the arena only as far as the projection needs: it starts at 2^24 words)
                if (nb_next + est1 + est2 + est3 > arena_cap_) ensure_arena(nb_next + est1 + est2 + est3, arena_cap_, true);
                if (o_.verbose) std::fprintf(stderr, "[sr] early growth at a frontier of %llu states\n", (unsigned long long)n);
            }
            // enqueue the next level before waiting for this one
            if (ahead.empty()) {
                const bool spec = !pessimistic_ && (double)(unique + est1 + est2) < lmax_ * (double)cap_ &&
                                  nb_next + est1 + est2 <= arena_cap_;
                if (spec) ahead.push_back(launch_expand(nb_next, 0, true, shape, undiscovered));
            }
            // ... and the one after it while the next is small (a launch shorter than the host's turnaround)
            if (ahead.size() == 1 && chain_max_ && est1 <= chain_max_ && !pessimistic_ &&
                (double)(unique + est1 + est2 + est3) < lmax_ * (double)cap_ && nb_next + est1 + est2 + est3 <= arena_cap_) {
                const u64 shape2 = (u64)((double)shape * std::max(ratio_, 0.05) * 1.1) + 64;
                ahead.push_back(launch_expand(0, 0, true, shape2, undiscovered, 0, true));
            }
            if (ahead.empty()) publish_pending_slot();  // otherwise the enqueued level publishes this one

            bool spec_ok = !ahead.empty();
            if (!wait_publish(sq, true)) {  // lc_ = this level's counters
                if (lc_.err == ERR_DEFERRED) {
                    // a speculative launch whose frontier outgrew the room planned for it expanded
                    // nothing: the table and the arena are grown for it and it runs again
                    SR_HIP(stream_sync(stream_));
                    init_counters();
                    if (o_.verbose)
                        std::fprintf(stderr, "[sr] level of %llu states outgrew the room planned for it: deferred\n",
                                     (unsigned long long)n);
                    const u32 s2 = launch_sync(n, undiscovered);
                    publish_pending_slot();
                    if (!wait_publish(s2, true)) repair_level(lstart_[lstart_.size() - 2], n, undiscovered);
                } else {
                    // the level overflowed the probe limit: double the table, finish the level on it
                    repair_level(lstart_[lstart_.size() - 2], n, undiscovered);
                }
                // the enqueued next level saw the error and expanded nothing
                spec_ok = false;
            }
            auto it = seq_launch_.find(sq);
            if (it != seq_launch_.end() && it->second < launch_frontier.size()) {
                launch_frontier[it->second] = n;
                launch_probes[it->second] = lc_.probes;
                launch_cas[it->second] = lc_.cas;
            }
            if (!spec_ok) ahead.clear();  // (launches behind a failed level expanded nothing)
            if (!account(lc_, ahead.size() == 2 ? " (next two enqueued)" : spec_ok ? " (next enqueued)" : "")) break;
            if (!ahead.empty()) {
                sq = ahead.front();
                ahead.pop_front();
            } else {
                sq = launch_sync(n, undiscovered);
            }
        }
        // A speculative level past the end may still be in flight: the host waits for it, but the
        // visited set's clear for the next check is enqueued behind it first (release_table), so
        // that the clear runs while this check returns and the next one is set up.
        // (the certificate pass reads the visited set after this loop: run_order releases it then)
        SR_HIP(hipEventRecord(ctx_->done, stream_));
        if (!o_.certify) release_table();
        drain(ctx_->done);
        check_async_growth();
        if (!o_.certify) free_unzeroed_table();
        return order_dependent;
    }

    // Until the stream has passed event `ev` (or every launch enqueued on it, ev = nullptr): a
    // spin on the query. (A blocking hipStreamSynchronize returned ~30 us after a check's last
    // kernel had ended.)
    void drain(hipEvent_t ev = nullptr) {
        if (!ev) {
            SR_HIP(stream_sync(stream_));
            return;
        }
        for (;;) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return clear_not_ready();
            if (e != hipErrorNotReady) SR_HIP(e);
            _mm_pause();
        }
    }

    // Nothing reads the visited set after the search (paths, replay and the Explorer use the arena
    // and the model): it goes back to the pool, zeroed on this stream behind the work enqueued so
    // far (a full table write: ~34 us for 2pc N=9's 256 MiB), and the next check takes it without
    // a clear at its start. Kept for the displacement scan of a counting run (sr_opts.counters),
    // and in FIFO order. SR_TABLE_RECYCLE=0: an ordinary free, each check clears its own table.
    void release_table() {
        if (table_recycle_ && !fifo_ && !o_.counters && !table_unzeroed_) keys_.release_zero(stream_);
    }
    // A table built by rehash_ranges goes back to the pool as it is, once the stream is idle.
    void free_unzeroed_table() {
        if (!table_recycle_ || fifo_ || o_.counters || !table_unzeroed_ || !keys_.p) return;
        SR_HIP(stream_sync(stream_));
        keys_.reset();
    }

    // Level 0 of the arena holds the init states as given, in REVERSE order: a bit mask (one bit per arena index
    // below the init count) of the indices that repeat another init state, and how many there are.
    static u64 repeated_inits(const std::vector<u64>& inits, std::vector<u32>& skip) {
        const u32 k = (u32)(inits.size() / W);
        skip.assign((k + 31) / 32, 0u);
        u64 dups = 0;
        std::set<std::vector<u64>> seen;
        for (u32 i = 0; i < k; ++i)
            if (!seen.insert(std::vector<u64>(&inits[(size_t)i * W], &inits[(size_t)i * W] + W)).second) {
                const u32 at = k - 1 - i;  // init state i is arena index k - 1 - i
                skip[at >> 5] |= 1u << (at & 31);
                ++dups;
            }
        return dups;
    }

    // The coverage pass (cover.hpp, kernels_cover.hpp) behind a search that explored everything: one launch
    // of cover_count over the arena, the persistent grid sized from the kernel's occupancy, and one read-back
    // of its 64-bit counters. Level 0 of the arena holds the init states as given, in REVERSE order: the
    // indices that repeat another init state are handed to the kernel as a bit mask and count nothing. Every
    // buffer lives for this call only. SR_COVER_GRID and SR_COVER_CHUNK (tests: several strides and several
    // flushes on a small arena) override the grid and the strides between two flushes.
    void cover_pass() {
        const auto t0 = Clock::now();
        CoverFigures f = cover_figures_for(m_);
        const u32 C = (u32)f.c.classes;
        const u64 n = lstart_.back();
        const std::vector<u64> inits = init_states_of(m_);
        const u32 k = (u32)(inits.size() / W);
        std::vector<u32> skip;
        const u64 dups = repeated_inits(inits, skip);
        DBuf<u64> g;
        DBuf<u32> skip_d;
        const size_t words = cover_words(C);
        g.alloc(o_.device, words);
        SR_HIP(hipMemsetAsync(g.p, 0, words * sizeof(u64), stream_));
        if (dups) {
            skip_d.alloc(o_.device, skip.size());
            SR_HIP(hipMemcpyAsync(skip_d.p, skip.data(), skip.size() * sizeof(u32), hipMemcpyHostToDevice, stream_));
        }
        int per_cu = 0, cus = 0;
        SR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)cover_count<M>, COVER_BLOCK, 0));
        SR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o_.device));
        u64 grid = per_cu > 0 && cus > 0 ? (u64)per_cu * (u64)cus : 1024;
        u32 chunk = std::min<u32>(cover_chunk_max<M>(), 1024);
        if (const char* e = std::getenv("SR_COVER_GRID"))
            if (std::atoi(e) > 0) grid = (u64)std::atoi(e);
        if (const char* e = std::getenv("SR_COVER_CHUNK"))
            if (std::atoi(e) > 0) chunk = std::min<u32>((u32)std::atoi(e), cover_chunk_max<M>());
        grid = std::max<u64>(1, std::min<u64>(grid, (n + COVER_BLOCK - 1) / COVER_BLOCK));
        cover_count<M><<<(u32)grid, COVER_BLOCK, 0, stream_>>>(m_, arena_.p, n, dups ? skip_d.p : nullptr, dups ? k : 0u, cover_always_mask(m_), C,
                                                              chunk, g.p);
        SR_HIP(hipGetLastError());
        std::vector<u64> h(words);
        SR_HIP(hipMemcpyAsync(h.data(), g.p, words * sizeof(u64), hipMemcpyDeviceToHost, stream_));
        SR_HIP(stream_sync(stream_));
        const u64* tail = &h[(size_t)3 * C];
        if (tail[COVER_DEGREES + 32 + 3])
            throw Error(SR_ERR_NONDETERMINISM, "coverage: cover_class named a class outside the model's " + std::to_string(C) + " for " +
                                                   std::to_string(tail[COVER_DEGREES + 32 + 3]) + " enabled slots");
        std::copy(&h[0], &h[C], f.enabled.begin());
        std::copy(&h[C], &h[(size_t)2 * C], f.taken.begin());
        std::copy(&h[(size_t)2 * C], &h[(size_t)3 * C], f.moved.begin());
        std::copy(tail, tail + COVER_DEGREES, f.c.out_degree);
        for (int p = 0; p < M::NPROPS; ++p) f.holds[(size_t)p] = tail[COVER_DEGREES + p];
        f.c.terminal = tail[COVER_DEGREES + 32];
        f.c.stutter_ends = tail[COVER_DEGREES + 32 + 1];
        f.c.max_out_degree = (u32)tail[COVER_DEGREES + 32 + 2];
        f.c.states = n - dups;
        f.c.ran = 1;
        f.c.pass_ms = secs(t0, Clock::now()) * 1e3;
        if (o_.verbose)
            std::fprintf(stderr, "[sr] coverage: %llu states, %u classes, grid %llu x %u, %u strides per flush, %.3f ms\n",
                         (unsigned long long)f.c.states, C, (unsigned long long)grid, COVER_BLOCK, chunk, f.c.pass_ms);
        cover = std::move(f);
    }

    // The certificate pass (certify.hpp, kernels_certify.hpp) behind any one-GPU search: the arena, its level
    // offsets, the parent ranks and the final visited set, re-derived by kernels that share nothing with the
    // search but the model and the table's lookup. all: the search explored everything (the closure pass runs).
    // The option changes no launch of the search; it keeps the visited set until here. SR_CERT_GRID (tests:
    // several strides on a small arena) overrides the persistent grids.
    void certify_pass(bool all) {
        if (!cap_ || !keys_.p) return;
        SR_HIP(stream_sync(stream_));
        CertInput in;
        in.lstart = lstart_;
        in.fifo = fifo_;
        in.explored_all = all;
        in.pmask = ((1u << M::NPROPS) - 1) & ~(emask_ | lmask_ | smask_);
        for (int p = 0; p < M::NPROPS && p < 32; ++p)
            if ((in.pmask >> p & 1) && disc[p].found && live_path_[p].empty() && disc[p].level + 1 < lstart_.size())
                in.disc_index[p] = lstart_[disc[p].level] + disc[p].rank;
        if (const char* e = std::getenv("SR_CERT_GRID"))
            if (std::atoi(e) > 0) in.grid = (u32)std::atoi(e);
        cert = cert_device(m_, view(), cap_, arena_.p, apar_.p, in, o_.device, stream_);
        if (o_.verbose)
            std::fprintf(stderr, "[sr] certificate: %llu states, %llu levels, %llu edges, ran %u, %.3f ms\n", (unsigned long long)cert.states,
                         (unsigned long long)cert.levels, (unsigned long long)cert.edges, cert.ran, cert.pass_ms);
    }

    // The step pass (step.hpp, kernels_step.hpp) behind a search that explored everything: one launch of
    // step_scan over the arena for all step properties of the model, the persistent grid sized from the kernel's
    // occupancy, and one read-back of its 64-bit counters. Per property with a violation then: the level of its
    // lowest violating arena index, W + 1 launches of step_min over that level, enqueued back to back, one more
    // read-back, and the witness: the tree path to the seed's source and the seed's step, accepted on the host
    // model (step_accept) before it becomes the discovery of p. Every buffer lives for this call only.
    // SR_STEP_GRID (tests: several strides on a small arena) overrides the grid.
    void step_pass() {
        if constexpr (has_smask<M>::value && !is_canon<M>::value && !is_evbits<M>::value) {
            const auto t0 = Clock::now();
            const u64 n = lstart_.back();
            const std::vector<u64> inits = init_states_of(m_);
            const u32 k = (u32)(inits.size() / W);
            std::vector<u32> skip;
            const u64 dups = repeated_inits(inits, skip);
            DBuf<u64> g;  // [the counters | the seed's W words | its slot | its arena index]
            DBuf<u32> skip_d;
            g.alloc(o_.device, STEP_WORDS + W + 2);
            SR_HIP(hipMemsetAsync(g.p, 0, STEP_LOW * sizeof(u64), stream_));
            SR_HIP(hipMemsetAsync(g.p + STEP_LOW, 0xff, (STEP_WORDS - STEP_LOW) * sizeof(u64), stream_));
            if (dups) {
                skip_d.alloc(o_.device, skip.size());
                SR_HIP(hipMemcpyAsync(skip_d.p, skip.data(), skip.size() * sizeof(u32), hipMemcpyHostToDevice, stream_));
            }
            int per_cu = 0, cus = 0;
            SR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)step_scan<M>, STEP_BLOCK, 0));
            SR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o_.device));
            u64 grid = per_cu > 0 && cus > 0 ? (u64)per_cu * (u64)cus : 1024;
            if (const char* e = std::getenv("SR_STEP_GRID"))
                if (std::atoi(e) > 0) grid = (u64)std::atoi(e);
            grid = std::max<u64>(1, std::min<u64>(grid, (n + STEP_BLOCK - 1) / STEP_BLOCK));
            step_scan<M><<<(u32)grid, STEP_BLOCK, 0, stream_>>>(m_, arena_.p, n, dups ? skip_d.p : nullptr, dups ? k : 0u, smask_, g.p);
            SR_HIP(hipGetLastError());
            std::vector<u64> h(STEP_WORDS);
            SR_HIP(hipMemcpyAsync(h.data(), g.p, STEP_WORDS * sizeof(u64), hipMemcpyDeviceToHost, stream_));
            SR_HIP(stream_sync(stream_));
            const double scan_ms = secs(t0, Clock::now()) * 1e3;
            step.assign(M::NPROPS, step_none());
            for (int p = 0; p < M::NPROPS; ++p) {
                if (!(smask_ >> p & 1)) continue;
                const auto t1 = Clock::now();
                sr_step_result& r = step[p];
                r.ran = 1;
                r.edges = h[0];
                r.violations = h[STEP_VIOL + p];
                r.sources = h[STEP_SRC + p];
                r.scan_ms = scan_ms;
                if (r.violations && !disc[p].found) {
                    const u64 low = h[STEP_LOW + p];
                    if (low >= n) throw Error(SR_ERR_HIP, "step pass: the scan counts violating edges and names no source");
                    // the level of the lowest violating arena index is the lowest depth of a violating source
                    const size_t level = (size_t)(std::upper_bound(lstart_.begin(), lstart_.end(), low) - lstart_.begin()) - 1;
                    const u64 lo = lstart_[level], hi = lstart_[level + 1];
                    u64* const seed_d = g.p + STEP_WORDS;
                    SR_HIP(hipMemsetAsync(seed_d, 0xff, (W + 2) * sizeof(u64), stream_));
                    for (int j = 0; j <= W; ++j)
                        step_min<M><<<blocks_for(hi - lo, STEP_BLOCK), STEP_BLOCK, 0, stream_>>>(m_, arena_.p, lo, hi, p, j, seed_d);
                    SR_HIP(hipGetLastError());
                    u64 seed[W + 2];
                    SR_HIP(hipMemcpyAsync(seed, seed_d, sizeof(seed), hipMemcpyDeviceToHost, stream_));
                    SR_HIP(stream_sync(stream_));
                    const u64 slot = seed[W], at = seed[W + 1];
                    if (at < lo || at >= hi || slot >= (u64)64 * M::MW)
                        throw Error(SR_ERR_HIP, "step pass: the tie-break found no seed in the level of the lowest violating source");
                    std::vector<u64> path;
                    tree_path((u32)level, (u32)(at - lo), path);
                    if (path.size() != (level + 1) * W || !std::equal(seed, seed + W, path.end() - W))
                        throw Error(SR_ERR_HIP, "step pass: the seed's tree path does not end at the seed's source");
                    u64 out[W];
                    if (!m_.apply(seed, (int)slot, out)) throw Error(SR_ERR_NONDETERMINISM, "step pass: the seed's slot yields no state on the host model");
                    path.insert(path.end(), out, out + W);
                    const std::vector<i64> acts = step_accept(m_, p, path, (int)slot);
                    r.step_index = (int64_t)level;
                    r.step_action = acts.back();
                    r.witness_len = (int64_t)acts.size();
                    r.init_index = step_init_index<M>(inits, path.data());
                    if (r.init_index < 0) throw Error(SR_ERR_NONDETERMINISM, "step pass: the witness starts at no init state");
                    live_path_[p] = path;
                    step_action_[p] = r.step_action;
                    disc[p].found = true;
                    disc[p].level = disc[p].rank = 0;
                }
                r.min_ms = secs(t1, Clock::now()) * 1e3;
                if (o_.verbose)
                    std::fprintf(stderr, "[sr] step pass \"%s\": %llu edges, %llu violations, %llu sources, scan %.3f ms, seed %.3f ms\n",
                                 m_.prop_name(p), (unsigned long long)r.edges, (unsigned long long)r.violations,
                                 (unsigned long long)r.sources, r.scan_ms, r.min_ms);
            }
        }
    }

    // The complete `eventually` check (live.hpp, kernels_live.hpp) behind a search that explored
    // everything: per `eventually` property still without a discovery, live_mark, then live_trim
    // until a round removes nothing (one counter read-back per round, as for a level; the worklist
    // shrinks, so later rounds are cheap), and if an init state survived, the witness by live_walk.
    // The arena is R, the final visited set names its states. Every buffer lives for this call only.
    // sr_opts.liveness = SR_LIVENESS_PROGRESS launches the FAIR instantiations of live_trim and
    // live_walk (progress fairness, live.hpp); SR_LIVENESS_WEAK launches the FAIR live_trim and then
    // live_weak_pass below in place of the walk, SR_LIVENESS_STRONG likewise live_strong_pass (both through
    // live_fair_pass, over the stages of LiveFair); every other value launches the plain ones.
    void live_pass() {
        live.assign(M::NPROPS, live_result_none());
        live_weak.assign(M::NPROPS, live_fair_none<sr_live_weak>());
        live_strong.assign(M::NPROPS, live_fair_none<sr_live_strong>());
        live_leads.assign(M::NPROPS, live_leads_none());
        if constexpr ((has_emask<M>::value || has_lmask<M>::value) && !is_canon<M>::value && !is_evbits<M>::value) {
            u32 todo = 0;  // the `eventually` properties without a discovery, and the leads-to properties
            for (int p = 0; p < M::NPROPS; ++p)
                if (((emask_ | lmask_) >> p & 1) && !disc[p].found) todo |= 1u << p;
            if (!todo) return;
            if (lstart_.back() > 0xffffffffull)
                throw Error(SR_ERR_UNSUPPORTED, "liveness with more than 2^32 - 1 unique states: the pass indexes the arena with 32 bits");
            const u32 n = (u32)lstart_.back();
            const bool weak = o_.liveness == SR_LIVENESS_WEAK;  // (refused at spawn unless fair_slots_model<M>)
            const bool strong = o_.liveness == SR_LIVENESS_STRONG;  // (likewise)
            const bool fair = o_.liveness == SR_LIVENESS_PROGRESS || weak || strong;
            const TableView t = view();
            const size_t bwords = (size_t)((cap_ + 31) / 32);
            DBuf<u64> slot_of, lcb, out;
            DBuf<u32> alive, onpath, wl[2], np_list;
            slot_of.alloc(o_.device, n);
            alive.alloc(o_.device, bwords);
            wl[0].alloc(o_.device, n);
            wl[1].alloc(o_.device, n);
            lcb.alloc(o_.device, (sizeof(LiveCounters) + 7) / 8);
            LiveCounters* lc = reinterpret_cast<LiveCounters*>(lcb.p);
            LiveCounters h{};
            auto read_back = [&] {  // the launch's counters (waits for it)
                SR_HIP(hipGetLastError());
                SR_HIP(hipMemcpyAsync(&h, lc, sizeof(h), hipMemcpyDeviceToHost, stream_));
                SR_HIP(stream_sync(stream_));
                if (h.err & LIVE_ERR_LOOKUP)
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: find_slot did not find a reachable state, or a successor of one, in the "
                                                       "visited set (an engine error: such a state is never taken as \"not alive\")");
                if (h.err & LIVE_ERR_STUCK)
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: a state of the fixpoint has successors, none of them in the fixpoint");
            };
            const std::vector<u64> inits = init_states_of(m_);
            const u32 k = (u32)(inits.size() / W);  // level 0 of the arena: the init states in REVERSE order
            u32 walk_steps = LIVE_WALK_STEPS;
            if (const char* e = std::getenv("SR_LIVE_WALK_STEPS"))  // (tests: several launches on a short witness)
                if (std::atoi(e) > 0) walk_steps = std::min<u32>((u32)std::atoi(e), LIVE_WALK_STEPS);
            for (; todo; todo &= todo - 1) {
                const int p = __builtin_ctz(todo);
                const auto t0 = Clock::now();
                sr_live_result& r = live[p];
                r.ran = 1;
                sr_live_leads* const leads = lmask_ >> p & 1 ? &live_leads[p] : nullptr;  // (a leads-to property: live.hpp LEADS-TO)
                SR_HIP(hipMemsetAsync(alive.p, 0, bwords * sizeof(u32), stream_));
                SR_HIP(hipMemsetAsync(lc, 0, sizeof(LiveCounters), stream_));
                live_mark<M><<<blocks_for(n, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, n, t, p, slot_of.p, alive.p, wl[0].p, lc);
                read_back();
                u32 cnt = h.next_n;
                r.not_p_states = r.surviving = cnt;
                const u32 np_cnt = cnt;
                int last = 0;  // the worklist the last round wrote: the states of the fixpoint that are no sinks
                if (weak || strong) {  // the weak and the strong mode keep live_mark's list
                    if (!np_list.p) np_list.alloc(o_.device, n);
                    SR_HIP(hipMemcpyAsync(np_list.p, wl[0].p, (size_t)np_cnt * sizeof(u32), hipMemcpyDeviceToDevice, stream_));
                }
                for (int cur = 0;; cur ^= 1) {  // (every round but the last removes a state)
                    last = cur ^ 1;
                    r.rounds += 1;
                    r.examined += cnt;
                    h.next_n = h.removed = 0;
                    if (cnt) {
                        SR_HIP(hipMemsetAsync(lc, 0, sizeof(LiveCounters), stream_));
                        if (fair)
                            live_trim<M, true><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, t, slot_of.p, alive.p,
                                                                                                       wl[cur].p, cnt, wl[cur ^ 1].p, lc);
                        else
                            live_trim<M><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, t, slot_of.p, alive.p, wl[cur].p,
                                                                                                 cnt, wl[cur ^ 1].p, lc);
                        read_back();
                    }
                    r.surviving -= h.removed;
                    cnt = h.next_n;
                    if (o_.verbose)
                        std::fprintf(stderr, "[sr] liveness \"%s\" round %u: removed %u, worklist %u, surviving %llu\n", m_.prop_name(p),
                                     r.rounds, h.removed, cnt, (unsigned long long)r.surviving);
                    if (!h.removed) break;
                }
                if (weak || strong) {
                    live_fair_pass(strong, LivePassArgs{p, r, n, t, bwords, slot_of.p, alive.p, np_list.p, np_cnt, wl[last].p, cnt, wl[last ^ 1].p,
                                                        inits, k, walk_steps, leads});
                    r.pass_ms = secs(t0, Clock::now()) * 1e3;
                    continue;
                }
                std::vector<u64> path;  // the witness' states: the walk's first state, behind a leads-to prefix
                u32 seed = ~0u;         // a leads-to property: the seed's arena index
                if (leads) {
                    seed = live_leads_seed<false>(p, n, k, slot_of.p, alive.p, nullptr, nullptr, *leads);
                    if (seed != ~0u) live_leads_prefix(seed, inits, r, path);
                } else {
                    // the init state of lowest index whose bit survived (one launch, one read-back)
                    SR_HIP(hipMemsetAsync(&lc->first_init, 0xff, sizeof(u32), stream_));
                    live_first_init<><<<1, LIVE_BLOCK, 0, stream_>>>(slot_of.p, alive.p, k, lc);
                    read_back();
                    if (h.first_init < k) r.init_index = (int32_t)h.first_init;
                    if (r.init_index >= 0) path.assign(&inits[(size_t)r.init_index * W], &inits[(size_t)r.init_index * W] + W);
                }
                if (!path.empty()) {
                    const size_t off = path.size() / W - 1;  // the walk starts at this index of the path
                    if (!onpath.p) onpath.alloc(o_.device, bwords);
                    if (!out.p) out.alloc(o_.device, ((size_t)walk_steps + 1) * W);
                    SR_HIP(hipMemsetAsync(onpath.p, 0, bwords * sizeof(u32), stream_));
                    if (leads) SR_HIP(hipMemcpyAsync(out.p, arena_.p + (size_t)seed * W, W * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
                    else SR_HIP(hipMemcpyAsync(out.p, path.data(), W * sizeof(u64), hipMemcpyHostToDevice, stream_));
                    for (u32 resume = 0;; resume = 1) {  // (each launch but the last takes walk_steps steps; |F_p| in all)
                        SR_HIP(hipMemsetAsync(lc, 0, sizeof(LiveCounters), stream_));
                        if (fair) live_walk<M, true><<<1, 64, 0, stream_>>>(m_, t, alive.p, onpath.p, out.p, walk_steps, resume, lc);
                        else live_walk<M><<<1, 64, 0, stream_>>>(m_, t, alive.p, onpath.p, out.p, walk_steps, resume, lc);
                        read_back();
                        if (h.steps > walk_steps) throw Error(SR_ERR_HIP, "liveness: a witness launch reports more steps than its bound");
                        const size_t o = path.size();
                        path.resize(o + (size_t)h.steps * W);
                        if (h.steps)
                            SR_HIP(hipMemcpy(&path[o], out.p + W, (size_t)h.steps * W * sizeof(u64), hipMemcpyDeviceToHost));
                        if (path.size() / W - 1 - off > r.surviving)
                            throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness is longer than the fixpoint has states");
                        if (h.end != LIVE_WALK_MORE) break;
                        if (!h.steps) throw Error(SR_ERR_HIP, "liveness: a witness launch made no step");
                        SR_HIP(hipMemcpyAsync(out.p, out.p + (size_t)h.steps * W, W * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
                    }
                    if (h.end == LIVE_WALK_STUTTER && !fair) throw Error(SR_ERR_HIP, "liveness: a witness ends at a stutter end with the mode off");
                    live_accept(p, r, path, h.end, fair, off);
                }
                r.pass_ms = secs(t0, Clock::now()) * 1e3;
            }
        }
    }

    // The device's witness is replayed on the host model before it becomes the discovery of p: every
    // step is a successor in `actions()` order (concrete_path), the condition of p holds on no state,
    // and the path ends at a terminal state or (lasso) at a state EQUAL, word for word, to an earlier
    // one; the device ended the walk on equal visited-set slots, which in fingerprint mode are equal
    // 64-bit fingerprints. Under progress fairness (fair) also: no step returns its own state, and a
    // path that is no lasso ends at a terminal state or at a stutter end, which has at least one
    // successor and whose successors all are the state itself.
    // off: the index of the witness' own first state on the path (a leads-to property: behind its prefix, live.hpp
    // LEADS-TO; 0 otherwise). The loop closes on a state from there on: one that closes on a prefix state only is
    // an engine error, reported as the collision below.
    void live_accept(int p, sr_live_result& r, const std::vector<u64>& path, u32 end, bool fair, size_t off = 0) {
        const size_t len = path.size() / W - 1;
        const std::string name = live_replay(p, path, fair, off);
        const u64* last = &path[len * W];
        if (end == LIVE_WALK_LOOP) {
            size_t j = off;
            while (j < len && !std::equal(last, last + W, &path[j * W])) ++j;
            if (j == len)
                throw Error(SR_ERR_NONDETERMINISM, "liveness: fingerprint collision: the witness of \"" + name + "\" ended as a loop at step " +
                                                       std::to_string(len) + ", but its state there equals no earlier state of the path");
            r.loop_start = (int64_t)j;
            r.end_kind = SR_LIVE_END_LOOP;
        } else {
            u64 all = 0, other = 0;
            for_each_successor(m_, last, [&](int, const u64* ns) { ++all, other += !std::equal(last, last + W, ns); });
            if (end == LIVE_WALK_STUTTER) {
                if (!all || other)
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness of \"" + name + "\" ends at a state that is no stutter end (" +
                                                           std::to_string(all) + " successors, " + std::to_string(other) + " of them other states)");
                r.end_kind = SR_LIVE_END_STUTTER;
            } else {
                if (all) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness of \"" + name + "\" ends at a state that is not terminal");
                r.end_kind = SR_LIVE_END_TERMINAL;
            }
        }
        live_found(p, r, path);
    }

    // A fair mode's lasso, replayed on the host model before it becomes the discovery of p: live_replay's checks
    // with fair = true, the last state equals the state at loop_start word for word, and the loop is weakly fair
    // on its own states and steps (live.hpp live_loop_fair); strong: strongly fair (live_loop_strong_fair). A
    // path that fails is an engine error, never a discovery.
    void live_accept_loop(int p, sr_live_result& r, const std::vector<u64>& path, size_t loop_start, bool strong, size_t off = 0) {
        const size_t len = path.size() / W - 1;
        const std::string name = live_replay(p, path, true, off);
        if (loop_start < off) throw Error(SR_ERR_NONDETERMINISM, "liveness: the closed walk of the witness of \"" + name + "\" starts on its prefix");
        if (loop_start >= len || !std::equal(&path[len * W], &path[len * W] + W, &path[loop_start * W]))
            throw Error(SR_ERR_NONDETERMINISM, "liveness: the closed walk of the witness of \"" + name + "\" does not end where it starts");
        if (strong ? !live_loop_strong_fair(m_, &path[loop_start * W], len - loop_start)
                   : !live_loop_fair(m_, &path[loop_start * W], len - loop_start))
            throw Error(SR_ERR_NONDETERMINISM, "liveness: the closed walk of the witness of \"" + name + "\" is not " +
                                                   (strong ? "strongly" : "weakly") + " fair");
        r.loop_start = (int64_t)loop_start;
        r.end_kind = SR_LIVE_END_LOOP;
        live_found(p, r, path);
    }

    // What every acceptance checks first: every step is a successor in `actions()` order (concrete_path), the
    // condition of p holds on no state, and (fair) no step returns its own state. The property's name.
    // A leads-to property (off: its trigger_index): the steps are checked over the whole path, the trigger holds at
    // off, and the condition and the self-loop checks apply from off on (the condition may hold on the prefix).
    std::string live_replay(int p, const std::vector<u64>& path, bool fair, size_t off = 0) {
        const size_t len = path.size() / W - 1;
        const std::string name = m_.prop_name(p);
        std::vector<i64> acts, described;
        concrete_path(m_, path, acts, described);
        if (off > len) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness of \"" + name + "\" is shorter than its prefix");
        if ((lmask_ >> p & 1) && !live_leads_from(m_, p, &path[off * W]))
            throw Error(SR_ERR_NONDETERMINISM, "liveness: the trigger of \"" + name + "\" does not hold at step " + std::to_string(off) + " of its witness");
        for (size_t i = off; i <= len; ++i)
            if (!live_not_p(m_, p, &path[i * W]))
                throw Error(SR_ERR_NONDETERMINISM, "liveness: \"" + name + "\" holds at step " + std::to_string(i) + " of its witness");
        if (fair)
            for (size_t i = off; i < len; ++i)
                if (std::equal(&path[i * W], &path[i * W] + W, &path[(i + 1) * W]))
                    throw Error(SR_ERR_NONDETERMINISM, "liveness: step " + std::to_string(i) + " of the witness of \"" + name +
                                                           "\" returns its own state (a fair mode steps over no self-loop)");
        return name;
    }
    // An accepted witness becomes the discovery of p.
    void live_found(int p, sr_live_result& r, const std::vector<u64>& path) {
        r.witness_len = (int64_t)(path.size() / W - 1);
        live_path_[p] = path;
        disc[p].found = true;
        disc[p].level = disc[p].rank = 0;
    }

    // What live_pass hands a fair pass, behind live_mark and the progress trim of property p: np the list
    // live_mark wrote, u0 the trim's last worklist (F_p' minus its sinks), spare the other worklist buffer.
    struct LivePassArgs {
        int p;
        sr_live_result& r;
        u32 n;
        const TableView& t;
        size_t bwords;
        const u64* slot_of;
        const u32* alive;
        const u32* np;
        u32 np_cnt;
        u32* u0;
        u32 u0_cnt;
        u32* spare;
        const std::vector<u64>& inits;
        u32 k, walk_steps;
        sr_live_leads* leads;  // a leads-to property's figures (nullptr: an `eventually` property)
    };

    // LEADS-TO (live.hpp; kernels_live.hpp live_leads_scan, live_leads_min): the three counts and the seed of
    // property p over the arena's n states, behind the mode's stages for its condition. RANKED: X_Q is FairF (idx,
    // rank); otherwise the alive bitmap. Returns the seed's arena index (~0: no violating state). One read-back for
    // the counts; then W + 1 launches over the seed's level, enqueued back to back, and one more read-back.
    template <bool RANKED>
    u32 live_leads_seed(int p, u32 n, u32 k, const u64* slot_of, const u32* alive, const u32* idx, const u32* rank, sr_live_leads& L) {
        if constexpr (has_lmask<M>::value) {
            const auto t0 = Clock::now();
            DBuf<u64> buf;  // [LiveLeadsCounters | the seed's W words | its arena index]
            constexpr size_t CW = sizeof(LiveLeadsCounters) / 8;
            static_assert(sizeof(LiveLeadsCounters) == 16, "LiveLeadsCounters: four u32");
            buf.alloc(o_.device, CW + W + 1);
            LiveLeadsCounters* lc = reinterpret_cast<LiveLeadsCounters*>(buf.p);
            u64* seed_w = buf.p + CW;
            u32* seed_i = reinterpret_cast<u32*>(buf.p + CW + W);
            SR_HIP(hipMemsetAsync(buf.p, 0xff, (CW + W + 1) * sizeof(u64), stream_));
            SR_HIP(hipMemsetAsync(lc, 0, 3 * sizeof(u32), stream_));
            live_leads_scan<M, RANKED><<<std::min(blocks_for(n, LIVE_BLOCK), LIVE_LEADS_GRID), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, n, k, p, slot_of, alive, idx, rank, lc);
            SR_HIP(hipGetLastError());
            LiveLeadsCounters h{};
            SR_HIP(hipMemcpyAsync(&h, lc, sizeof(h), hipMemcpyDeviceToHost, stream_));
            SR_HIP(stream_sync(stream_));
            L.ran = 1;
            L.triggered = h.triggered;
            L.pending = h.pending;
            L.violating = h.violating;
            u32 seed = ~0u;
            if (h.violating) {
                if (h.min_idx >= n) throw Error(SR_ERR_HIP, "liveness: the seed scan counts violating states and names none");
                // the level of the lowest violating arena index is the lowest depth of a violating state
                const size_t level = (size_t)(std::upper_bound(lstart_.begin(), lstart_.end(), (u64)h.min_idx) - lstart_.begin()) - 1;
                const u32 lo = (u32)lstart_[level], hi = (u32)lstart_[level + 1];
                for (int j = 0; j <= W; ++j)
                    live_leads_min<M, RANKED><<<blocks_for(hi - lo, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, lo, hi, p, slot_of, alive, idx,
                                                                                                        rank, j, seed_w, seed_i);
                SR_HIP(hipGetLastError());
                SR_HIP(hipMemcpyAsync(&seed, seed_i, sizeof(u32), hipMemcpyDeviceToHost, stream_));
                SR_HIP(stream_sync(stream_));
                if (seed < lo || seed >= hi) throw Error(SR_ERR_HIP, "liveness: the tie-break found no seed in the level of the lowest violating state");
                L.trigger_index = L.trigger_depth = (int64_t)level;
            }
            L.seed_ms = secs(t0, Clock::now()) * 1e3;
            return seed;
        } else {
            (void)p, (void)n, (void)k, (void)slot_of, (void)alive, (void)idx, (void)rank, (void)L;
            return ~0u;
        }
    }

    // The prefix of a leads-to witness: the search's own tree path from an init state to the seed (its states into
    // path, the seed last), and the lowest index of an init state equal to its first state into r.init_index.
    void live_leads_prefix(u32 seed, const std::vector<u64>& inits, sr_live_result& r, std::vector<u64>& path) {
        const size_t level = (size_t)(std::upper_bound(lstart_.begin(), lstart_.end(), (u64)seed) - lstart_.begin()) - 1;
        tree_path((u32)level, (u32)(seed - lstart_[level]), path);
        for (size_t i = 0; i < inits.size() / W && r.init_index < 0; ++i)
            if (std::equal(&inits[i * W], &inits[i * W] + W, path.begin())) r.init_index = (int32_t)i;
        if (r.init_index < 0) throw Error(SR_ERR_NONDETERMINISM, "liveness: the prefix of a leads-to witness starts at no init state");
    }

    // WEAK and STRONG FAIRNESS (live.hpp; the kernels' headers in kernels_live.hpp): what the two passes share,
    // each stage written once. `bits` is the bitmap of the set the component search runs on (the weak mode's U,
    // the strong mode's W), L its list, X and Y the two other list buffers, cnt its size. One counter read-back
    // per round, as in the progress trim. Every buffer lives for the pass only: 4 bytes per table slot (slot ->
    // arena index), 8 bytes per arena state (rank, component), three worklists of 4 bytes per state of N_p; only
    // if F_p' has a cycle (alloc_search) 12 bytes more per arena state (colour, stamp, component size) and
    // 16 MW bytes of accumulators; only for a lasso 4 bytes more (ranks inside the component).
    template <class Stats>  // sr_live_weak or sr_live_strong
    struct LiveFair {
        static constexpr int MW = M::MW;
        static constexpr size_t HEAD = offsetof(LiveWeakCounters, notme);  // (the masks behind it live across launches)
        Engine& e;
        const LivePassArgs& a;
        Stats& s;
        const Clock::time_point t0 = Clock::now();
        DBuf<u32> bits, idx, rank, lrank, colour, stamp, comp, size, third;
        DBuf<u64> acc_me, or_took, wcb, lcb, out;  // acc_me: the weak mode's and_me, the strong mode's or_me
        LiveWeakCounters* wc = nullptr;
        LiveCounters* lc = nullptr;
        LiveWeakCounters hw{};
        u32 *L = nullptr, *X = nullptr, *Y = nullptr;
        u32 cnt = 0, round = 0;
        std::vector<u64> path;  // the witness' states
        u64 bound = 0;          // and how many steps it may have
        size_t off = 0;         // a leads-to property: the length of the prefix the path starts with (first_seed)
        u32 seed = ~0u;         //                      and the seed's arena index
        u32 g = 0, root = ~0u;  // the stem's last state and its component (by arena index)
        u64 c_mask[MW];         // acc_me of that component

        LiveFair(Engine& e_, const LivePassArgs& a_, Stats& s_) : e(e_), a(a_), s(s_) {}

        void fail(u32 err) const {
            if (err & LIVE_ERR_LOOKUP)
                throw Error(SR_ERR_NONDETERMINISM, "liveness: find_slot did not find a reachable state, or a successor of one, in the "
                                                   "visited set (an engine error: such a state is never taken as \"not alive\")");
            if (err & LIVE_ERR_STUCK)
                throw Error(SR_ERR_NONDETERMINISM, "liveness: a ranked state of the witness has no successor of a lower rank, or a "
                                                   "member of a level has no component");
        }
        void clear_head() { SR_HIP(hipMemsetAsync(wc, 0, HEAD, e.stream_)); }
        void read_w() {  // the launch's counters (waits for it)
            SR_HIP(hipGetLastError());
            SR_HIP(hipMemcpyAsync(&hw, wc, sizeof(hw), hipMemcpyDeviceToHost, e.stream_));
            SR_HIP(stream_sync(e.stream_));
            fail(hw.err);
        }

        // The buffers every run needs; the bitmap from u0, the slot -> arena index map and rank 0 for the sinks.
        void setup() {
            const int dev = e.o_.device;
            s.ran = 1;
            bits.alloc(dev, a.bwords);
            idx.alloc(dev, (size_t)e.cap_);
            rank.alloc(dev, a.n);
            comp.alloc(dev, a.n);
            third.alloc(dev, a.np_cnt);
            wcb.alloc(dev, (sizeof(LiveWeakCounters) + 7) / 8);
            lcb.alloc(dev, (sizeof(LiveCounters) + 7) / 8);
            wc = reinterpret_cast<LiveWeakCounters*>(wcb.p);
            lc = reinterpret_cast<LiveCounters*>(lcb.p);
            SR_HIP(hipMemsetAsync(bits.p, 0, a.bwords * sizeof(u32), e.stream_));
            SR_HIP(hipMemsetAsync(idx.p, 0xff, (size_t)e.cap_ * sizeof(u32), e.stream_));
            SR_HIP(hipMemsetAsync(rank.p, 0xff, (size_t)a.n * sizeof(u32), e.stream_));
            SR_HIP(hipMemsetAsync(comp.p, 0xff, (size_t)a.n * sizeof(u32), e.stream_));
            SR_HIP(hipMemsetAsync(wc, 0, sizeof(LiveWeakCounters), e.stream_));
            if (a.u0_cnt)
                live_set_bits<><<<blocks_for(a.u0_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(a.u0, a.u0_cnt, a.slot_of, bits.p);
            if (a.np_cnt)
                live_index<><<<blocks_for(a.np_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(a.np, a.np_cnt, a.slot_of, a.alive, bits.p,
                                                                                             idx.p, rank.p);
            L = a.u0, X = a.spare, Y = third.p;
            cnt = a.u0_cnt;
        }

        // The set trimmed to the states with a successor in it (the progress trim's kernel on `bits`).
        void trim() {
            while (cnt) {
                LiveCounters h{};
                SR_HIP(hipMemsetAsync(lc, 0, sizeof(LiveCounters), e.stream_));
                live_trim<M, true><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(e.m_, e.arena_.p, a.t, a.slot_of, bits.p, L, cnt, X,
                                                                                              lc);
                SR_HIP(hipGetLastError());
                SR_HIP(hipMemcpyAsync(&h, lc, sizeof(h), hipMemcpyDeviceToHost, e.stream_));
                SR_HIP(stream_sync(e.stream_));
                fail(h.err & LIVE_ERR_LOOKUP);
                if (h.next_n > cnt) throw Error(SR_ERR_HIP, "liveness: a trim round lists more states than its set has");
                std::swap(L, X);
                cnt = h.next_n;
                s.scc_rounds += 1;
                if (!h.removed) break;
            }
        }

        // What only the component search and the components' accumulators need. The mode initialises size, acc_me
        // and or_took: the weak mode once (and_me starts as all ones), the strong mode per level (live_level_open).
        void alloc_search() {
            const int dev = e.o_.device;
            colour.alloc(dev, a.n);
            stamp.alloc(dev, a.n);
            size.alloc(dev, a.n);
            acc_me.alloc(dev, (size_t)a.n * MW);
            or_took.alloc(dev, (size_t)a.n * MW);
            SR_HIP(hipMemsetAsync(stamp.p, 0, (size_t)a.n * sizeof(u32), e.stream_));
        }

        // The components of the set: colour, find the roots' components, take them out, until it is empty.
        void components() {
            while (cnt) {
                live_colour_init<><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(L, cnt, colour.p);
                u32 *src = L, *dst = X, sn = cnt;
                while (sn) {
                    clear_head();
                    live_colour_push<M><<<blocks_for(sn, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(e.m_, e.arena_.p, a.t, idx.p, bits.p, colour.p,
                                                                                                  stamp.p, ++round, src, sn, dst, wc);
                    read_w();
                    s.scc_rounds += 1;
                    if (hw.next_n > cnt) throw Error(SR_ERR_HIP, "liveness: a colouring round lists more states than its set has");
                    sn = hw.next_n;
                    src = dst;
                    dst = src == X ? Y : X;
                }
                live_scc_seed<><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(L, cnt, colour.p, comp.p);
                src = L, dst = X, sn = cnt;
                for (;;) {
                    clear_head();
                    live_scc_join<M><<<blocks_for(sn, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(e.m_, e.arena_.p, a.t, idx.p, bits.p, colour.p, comp.p,
                                                                                               src, sn, dst, wc);
                    read_w();
                    s.scc_rounds += 1;
                    if (hw.next_n > sn) throw Error(SR_ERR_HIP, "liveness: a join round lists more states than it was given");
                    sn = hw.next_n;
                    src = dst;
                    dst = src == X ? Y : X;
                    if (!hw.joined || !sn) break;
                }
                if (sn >= cnt) throw Error(SR_ERR_HIP, "liveness: a round of the component search took no state out of its set");
                live_scc_leave<><<<blocks_for(cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(L, cnt, a.slot_of, comp.p, bits.p);
                std::swap(L, src == X ? X : Y);  // (what has not joined is the next set)
                cnt = sn;
            }
        }

        // Ranks towards rank 0 in rk over the `todo` states listed in src: levels until one ranks nothing.
        void reach(u32* rk, u32* src, u32* dst, u32 todo) {
            for (u32 level = 1; todo; ++level) {
                clear_head();
                live_reach<M><<<blocks_for(todo, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(e.m_, e.arena_.p, a.t, idx.p, rk, level, src, todo, dst,
                                                                                          wc);
                read_w();
                s.reach_rounds += 1;
                if (rk == rank.p) s.fair_states += hw.joined;
                if (!hw.joined) break;
                todo = hw.next_n;
                std::swap(src, dst);
            }
        }

        // The init state of lowest index with a rank, into r.init_index; whether there is one.
        bool first_ranked() {
            clear_head();
            SR_HIP(hipMemsetAsync(&wc->first_init, 0xff, sizeof(u32), e.stream_));
            live_first_ranked<><<<1, LIVE_BLOCK, 0, e.stream_>>>(a.slot_of, idx.p, rank.p, a.k, wc);
            read_w();
            if (hw.first_init < a.k) a.r.init_index = (int32_t)hw.first_init;
            return a.r.init_index >= 0;
        }

        // A leads-to property, in place of first_ranked(): the counts, the seed among the states with a rank, and the
        // prefix into `path`; whether there is a seed.
        bool first_seed() {
            seed = e.template live_leads_seed<true>(a.p, a.n, a.k, a.slot_of, a.alive, idx.p, rank.p, *a.leads);
            if (seed == ~0u) return false;
            e.live_leads_prefix(seed, a.inits, a.r, path);
            off = path.size() / W - 1;
            return true;
        }
        bool first() { return a.leads ? first_seed() : first_ranked(); }

        // From the path's last state down the ranks rk to rank 0, then slot `then` (each launch but the last
        // takes walk_steps steps).
        void descend(const u32* rk, int then, u32 all) {
            const u32 walk_steps = a.walk_steps;
            for (;;) {
                clear_head();
                live_descend<M><<<1, 64, 0, e.stream_>>>(e.m_, a.t, idx.p, rk, out.p, walk_steps, then, all, wc);
                read_w();
                if (hw.steps > walk_steps + 1) throw Error(SR_ERR_HIP, "liveness: a witness launch reports more steps than its bound");
                const size_t o = path.size();
                path.resize(o + (size_t)hw.steps * W);
                if (hw.steps) {
                    SR_HIP(hipMemcpy(&path[o], out.p + W, (size_t)hw.steps * W * sizeof(u64), hipMemcpyDeviceToHost));
                    SR_HIP(hipMemcpyAsync(out.p, out.p + (size_t)hw.steps * W, W * sizeof(u64), hipMemcpyDeviceToDevice, e.stream_));
                }
                if (path.size() / W - 1 > bound) throw Error(SR_ERR_NONDETERMINISM, "liveness: the witness is longer than its bound");
                if (hw.end == LIVE_DESCEND_DONE) break;
                if (!hw.steps) throw Error(SR_ERR_HIP, "liveness: a witness launch made no step");
            }
        }

        // The stem from the init state first_ranked() found to rank 0 at g. A sink of F_p' ends the witness there
        // (terminal, or a stutter end: live_accept checks which) and stem() returns false; otherwise g lies in
        // the component `root`, whose acc_me mask is read into c_mask, and a closed walk has to follow.
        bool stem() {
            const std::vector<u64>& inits = a.inits;
            out.alloc(e.o_.device, ((size_t)a.walk_steps + 2) * W);
            if (a.leads) {  // (first_seed: the path holds the prefix, the seed last)
                SR_HIP(hipMemcpyAsync(out.p, e.arena_.p + (size_t)seed * W, W * sizeof(u64), hipMemcpyDeviceToDevice, e.stream_));
            } else {
                path.assign(&inits[(size_t)a.r.init_index * W], &inits[(size_t)a.r.init_index * W] + W);
                SR_HIP(hipMemcpyAsync(out.p, path.data(), W * sizeof(u64), hipMemcpyHostToDevice, e.stream_));
            }
            bound = off + ((u64)e.A_ + 2) * (a.r.surviving + 1);  // the stem and A + 1 segments, each a simple path
            descend(rank.p, -1, 0);
            s.stem_len = (int64_t)(path.size() / W - 1 - off);
            g = hw.last_idx;
            if (g >= a.n) throw Error(SR_ERR_HIP, "liveness: the stem's last state has no arena index");
            SR_HIP(hipMemcpy(&root, comp.p + g, sizeof(u32), hipMemcpyDeviceToHost));
            if (root == ~0u) {
                u64 all = 0;
                for_each_successor(e.m_, &path[path.size() - W], [&](int, const u64*) { ++all; });
                s.loop_len = 0;
                e.live_accept(a.p, a.r, path, all ? LIVE_WALK_STUTTER : LIVE_WALK_TERMINAL, true, off);
                return false;
            }
            if (root >= a.n) throw Error(SR_ERR_HIP, "liveness: the stem ends in a component without a root");
            SR_HIP(hipMemcpy(c_mask, acc_me.p + (size_t)root * MW, sizeof(c_mask), hipMemcpyDeviceToHost));
            return true;
        }

        // The closed walk inside g's component: for the slots in order the segment plan(slot) asks for (it reads
        // hw.notme, hw.taken and c_mask; LIVE_PLAN_SKIP: none), then home to g. A segment is the target set
        // (live_targets), ranks towards it inside the component, and the descent. keep_stem_masks: the weak
        // mode's notme keeps what the stem recorded at g; the strong mode's masks are the loop's alone.
        template <class Plan>
        void closed_walk(Plan&& plan, bool keep_stem_masks, bool strong) {
            lrank.alloc(e.o_.device, a.n);
            SR_HIP(hipMemsetAsync(lrank.p, 0xff, (size_t)a.n * sizeof(u32), e.stream_));
            if (keep_stem_masks) clear_head();
            else SR_HIP(hipMemsetAsync(wc, 0, sizeof(LiveWeakCounters), e.stream_));
            live_members<><<<blocks_for(a.np_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(a.np, a.np_cnt, comp.p, root, Y, wc);
            read_w();
            const u32 mcnt = hw.next_n;
            auto segment = [&](int pl, int slot) {
                clear_head();
                live_targets<M><<<blocks_for(mcnt, LIVE_BLOCK), LIVE_BLOCK, 0, e.stream_>>>(e.m_, e.arena_.p, a.t, idx.p, comp.p, root, pl, slot, g,
                                                                                            Y, mcnt, lrank.p, L, wc);
                read_w();
                if (!hw.joined) throw Error(SR_ERR_NONDETERMINISM, "liveness: a segment of the closed walk has no target in its component");
                reach(lrank.p, L, X, hw.next_n);
                s.segments += 1;
                descend(lrank.p, pl == LIVE_PLAN_TAKE ? slot : -1, 1);
            };
            for (int slot = 0; slot < (int)e.A_; ++slot) {
                const int pl = plan(slot);
                if (pl != LIVE_PLAN_SKIP) segment(pl, slot);
            }
            segment(LIVE_PLAN_HOME, 0);
            s.loop_len = (int64_t)(path.size() / W - 1 - off) - s.stem_len;
            e.live_accept_loop(a.p, a.r, path, off + (size_t)s.stem_len, strong, off);
        }
    };

    // The pass of the mode: only a FAIR_SLOTS model whose masks fit the kernels' counters has one.
    void live_fair_pass(bool strong, const LivePassArgs& a) {
        if constexpr (fair_slots_model<M> && M::MW <= LIVE_MW_MAX) {
            if (strong) live_strong_pass(a, live_strong[a.p]);
            else live_weak_pass(a, live_weak[a.p]);
        } else {
            (void)a;
            throw Error(SR_ERR_UNSUPPORTED, std::string(strong ? "strong" : "weak") + " fairness: this model's slots are not fairness classes");
        }
    }

    // WEAK FAIRNESS: U trimmed, its components, per component the fairness accumulators (live_comp_acc), the
    // goal set (live_goal), ranks towards it over F_p', and the witness.
    void live_weak_pass(const LivePassArgs& a, sr_live_weak& wk) {
        constexpr int MW = M::MW;
        LiveFair<sr_live_weak> f(*this, a, wk);
        f.setup();
        f.trim();
        wk.cyclic_states = f.cnt;
        const bool cyclic = f.cnt != 0;  // (U is not empty iff F_p' has a cycle, iff there is a component)
        if (cyclic) {
            f.alloc_search();
            SR_HIP(hipMemsetAsync(f.size.p, 0, (size_t)a.n * sizeof(u32), stream_));
            SR_HIP(hipMemsetAsync(f.acc_me.p, 0xff, (size_t)a.n * MW * sizeof(u64), stream_));
            SR_HIP(hipMemsetAsync(f.or_took.p, 0, (size_t)a.n * MW * sizeof(u64), stream_));
        }
        f.components();
        f.clear_head();
        u32 sn = 0;
        if (a.np_cnt) {
            if (cyclic)  // (without a component live_goal reads none of size, and_me, or_took: comp is ~0 everywhere)
                live_comp_acc<M><<<blocks_for(a.np_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, a.t, f.idx.p, f.comp.p, a.np, a.np_cnt,
                                                                                              f.size.p, f.acc_me.p, f.or_took.p, f.wc);
            live_goal<M><<<blocks_for(a.np_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(a.np, a.np_cnt, a.slot_of, a.alive, f.comp.p, f.size.p,
                                                                                      f.acc_me.p, f.or_took.p, f.rank.p, f.L, f.wc);
            f.read_w();
            wk.components = f.hw.comps;
            wk.fair_components = f.hw.fair_comps;
            wk.goal_states = wk.fair_states = f.hw.goal;
            sn = f.hw.next_n;
        }
        if (wk.goal_states) f.reach(f.rank.p, f.L, f.X, sn);
        if (f.first() && f.stem())
            f.closed_walk([&](int s) { return live_loop_plan(s, f.hw.notme, f.hw.taken, f.c_mask); }, true, false);
        wk.pass_ms = secs(f.t0, Clock::now()) * 1e3;
    }

    // STRONG FAIRNESS. The host form's recursive tree becomes level-synchronous rounds over all open components
    // at once: W starts as the weak mode's U; a level takes the components of G'[W], accumulates or_me and
    // or_took per component (live_comp_acc_or), lets live_refine freeze the fair nodes, drop the states that
    // enable a bad slot and hand the rest back to W, and trims W again; until W is empty. Memory is the weak
    // pass' plus one list of 4 bytes per state of N_p (the level's members); no level stamp is kept per state,
    // because live_refine clears the component number of every state that is not frozen.
    void live_strong_pass(const LivePassArgs& a, sr_live_strong& sg) {
        constexpr int MW = M::MW;
        LiveFair<sr_live_strong> f(*this, a, sg);
        DBuf<u32> lvl;
        f.setup();
        f.trim();
        sg.cyclic_states = f.cnt;
        if (f.cnt) {
            f.alloc_search();
            lvl.alloc(o_.device, f.cnt);
        }
        u64 frozen = 0;
        while (f.cnt) {  // one level of the tree
            const u32 members = f.cnt;
            SR_HIP(hipMemcpyAsync(lvl.p, f.L, (size_t)members * sizeof(u32), hipMemcpyDeviceToDevice, stream_));
            live_level_open<MW><<<blocks_for(members, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(lvl.p, members, f.size.p, f.acc_me.p, f.or_took.p);
            f.components();
            // the level's components: accumulate, then freeze, drop or hand back every member
            f.clear_head();
            live_comp_acc_or<M><<<blocks_for(members, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, a.t, f.idx.p, f.comp.p, lvl.p, members,
                                                                                            f.size.p, f.acc_me.p, f.or_took.p, f.wc);
            live_refine<M><<<blocks_for(members, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(m_, arena_.p, a.slot_of, lvl.p, members, f.comp.p, f.size.p,
                                                                                       f.acc_me.p, f.or_took.p, f.bits.p, f.L, f.wc);
            f.read_w();
            if (f.hw.next_n >= members) throw Error(SR_ERR_HIP, "liveness: a level of the decomposition removed no state from W");
            if (f.hw.comps) sg.levels += 1;
            sg.components += f.hw.comps;
            sg.fair_components += f.hw.fair_comps;
            frozen += f.hw.joined;
            f.cnt = f.hw.next_n;
            if (o_.verbose)
                std::fprintf(stderr, "[sr] liveness \"%s\" level %u: %u members, %u components (%u fair), %u back in W\n", m_.prop_name(a.p),
                             sg.levels, members, f.hw.comps, f.hw.fair_comps, f.cnt);
            f.trim();
        }
        // the goal set, ranks towards it over F_p'
        f.clear_head();
        u32 sn = 0;
        if (a.np_cnt) {
            live_goal_strong<><<<blocks_for(a.np_cnt, LIVE_BLOCK), LIVE_BLOCK, 0, stream_>>>(a.np, a.np_cnt, a.slot_of, a.alive, f.comp.p, f.rank.p,
                                                                                            f.L, f.wc);
            f.read_w();
            sg.goal_states = sg.fair_states = f.hw.goal;
            sn = f.hw.next_n;
            if (f.hw.goal < frozen) throw Error(SR_ERR_HIP, "liveness: the goal set lost a frozen state");
        }
        if (sg.goal_states) f.reach(f.rank.p, f.L, f.X, sn);
        if (f.first() && f.stem())
            f.closed_walk([&](int s) { return live_strong_plan(s, f.hw.taken, f.c_mask); }, false, true);
        sg.pass_ms = secs(f.t0, Clock::now()) * 1e3;
    }

    std::vector<std::vector<u64>> live_path_;  // per property: the states of a discovery made by the liveness pass (or the step pass)
    std::vector<i64> step_action_;             // per property: the last action of a step property's witness (-1: none)

    // Launch of the level whose frontier (n states) ends the arena, after the previous one is done:
    // the visited set and the arena are grown first if the level might not fit.
    u32 launch_sync(u64 n, u32 undiscovered) {
        const u64 d_eff = pessimistic_ ? D_ : std::min<u64>(D_, (u64)std::ceil(2.0 * recent_ratio() + 1.0));
        const double need = (double)(unique + n * d_eff);
        const u64 fbase = lstart_[lstart_.size() - 2];
        if (need > lmax_ * (double)cap_) {
            grow_table(nullptr, 0, growth_slots((u64)(need / lmax_) + 1));
            // The arena takes its next step (x8 / x4) with the table: a table that had to grow holds nearly
            // as many states as the arena (both start at 2^22), and the arena's own step, a copy and
            // a second stop of the level pipeline, would follow a level later (2pc N=9 without a
            // hint: levels 9 and 10).
            if ((double)arena_cap_ < lmax_ * (double)cap_) ensure_arena(arena_cap_ + 1, fbase + n);
        }
        ensure_arena(fbase + n + n * d_eff, fbase + n);
        return launch_expand(fbase, (u32)n, false, n, undiscovered);
    }

    // expand_fast's grid is capped at whole residencies of the device (resident blocks per CU at
    // its LDS footprint x CUs, grid_res_ of them); the kernel strides over any further parents.
    // Whole residencies avoid a partial last wave of workgroups. For 2pc one residency (every block
    // starting at once and striding with its prefetch) beats two: N=9 1.556 -> 1.520 ms, N=10 7.93
    // -> 7.76, N=11 50.7 -> 50.5 (1.17 / 0.83 residencies were slower); increment_lock (36.8 ms with
    // one against 33.3) and paxos stay at two (round 6, `profiles/r06_grid_cap.txt`). The cap is
    // printed with verbose=1. SR_GRID_MAX > 0 overrides it (<= 0 or unparsable: the default).
    // The cap is cached per kernel form (the probe loop switches to the queue form once
    // the table grows past 2^27 slots, whose occupancy differs from the rounds form's).
    // The dynamic-chunk instantiations (deep levels) have a cap of their own, from their own occupancy
    // (their registers need not match the static form's).
    u32 expand_grid_cap(bool nopf = false, bool deep = false) {
        const int form = (nopf ? 2 : probe_loop() < 0 ? 1 : 0) + (deep && !nopf ? 3 : 0);
        u32& cap = grid_max_[form];
        if (cap) return cap;
        if (grid_env_) return cap = grid_env_;
        int per_cu = 0, cus = 0;
        const size_t dyn = filt_bytes();
        const void* k = form == 1 ? (const void*)expand_fast<M, -4, 0> : (const void*)expand_fast<M, 1, 0>;
        if (form == 3) k = (const void*)expand_fast<M, 1, 0, false, false, true>;
        if (form == 4) k = (const void*)expand_fast<M, -4, 0, false, false, true>;
        if constexpr (W >= 4)
            if (nopf) k = (const void*)expand_fast<M, 1, 0, false, true>;
        SR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 64 * WPB, dyn));
        SR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o_.device));
        cap = per_cu > 0 && cus > 0 ? (u32)(grid_res_ * per_cu * cus) : ~0u;
        if (o_.verbose)
            std::fprintf(stderr, "[sr] expand grid cap %u blocks (%d per CU x %d CUs x %u)%s\n", cap, per_cu, cus, grid_res_,
                         nopf ? " [no prefetch]" : form >= 3 ? " [dynamic chunks]" : "");
        return cap;
    }
    // expand_fast's balanced level geometry (kernels.hpp LevelGeom, the BAL instantiations): for a
    // pipelined launch (dev_n) whose estimated frontier is at least balance_min_ parents (a smaller
    // level keeps the fixed geometry and with it the speculative load of its first parents), for a
    // launch with an exact n at any size; never for the dynamic-chunk form. Counted in
    // stats.balanced_levels. By default only for one-word states (balance_min_ below).
    // (The threshold: 2pc N=9's levels 6 and 22, shapes of 37 K and 49 K parents, were 1-2 us slower
    // balanced, levels of 84 K and more equal or faster: profiles/r07_level_geometry.txt.)
    bool balance_level(u64 shape, bool dev_n, bool deep) {
        if (!balance_ || deep || (dev_n ? shape < balance_min_ : balance_min_ == ~0ull)) return false;
        stats.balanced_levels++;
        return true;
    }
    // The expand_fast instantiation of a launch: counting, wide without prefetch, dynamic chunks (deep)
    // or static; all but the dynamic chunks with the fixed or the balanced level geometry (bal).
    template <class L>
    void launch_form(L& launch, bool nopf, bool deep, bool bal) {
        if (o_.counters) bal ? launch(expand_fast<M, 1, 0, true, false, false, true>) : launch(expand_fast<M, 1, 0, true>);
        else if (nopf) launch_nopf(launch, bal);
        else if (deep) probe_loop() < 0 ? launch(expand_fast<M, -4, 0, false, false, true>) : launch(expand_fast<M, 1, 0, false, false, true>);
        else if (probe_loop() < 0) bal ? launch(expand_fast<M, -4, 0, false, false, false, true>) : launch(expand_fast<M, -4, 0>);
        else bal ? launch(expand_fast<M, 1, 0, false, false, false, true>) : launch(expand_fast<M, 1, 0>);
    }
    bool action_table_ = false;      // SLOT_ACTION_TABLE on this engine's expand_fast launches (set in the constructor)
    bool balance_ = true;            // SR_BALANCE=0: the fixed geometry everywhere (A/B runs, tests)
    // SR_BALANCE_MIN. Wider states: no balanced launch unless it is set. The case for equal shares is a
    // grid of one residency, every workgroup running at once, which only one-word states have (grid_res_).
    // Wide states take 4-8 parents per wave, so a narrower chunk rounds up to the same parents per wave,
    // and the lost overlap of the first load cost their latency-bound levels (paxos C=3 0.61-0.63 ->
    // 0.64-0.65 ms); one of increment_lock N=10's levels of 151 200 parents went from 25 to 39 us.
    u64 balance_min_ = W == 1 ? (u64)1 << 16 : ~0ull;
    // A level of more than DYN_MIN_RATIO chunks per workgroup takes the kernel with dynamic chunks
    // (kernels.hpp SR_DYN_CHUNKS; the kernel checks the real frontier again). Narrow states only: the
    // wide kernels' registers set their residency.
    bool deep_level(u64 chunks, u32 grid) const {
        return SR_DYN_CHUNKS && W < 4 && dyn_env_ && grid >= DYN_SHARDS && chunks > (u64)DYN_MIN_RATIO * grid;
    }
    bool dyn_env_ = !std::getenv("SR_DYN") || std::atoi(std::getenv("SR_DYN")) != 0;  // SR_DYN=0: measurement knob
    // Wide states: the kernel without the register prefetch of the next chunk's parents when every
    // chunk of the level has its own workgroup within that kernel's grid cap (DESIGN.md §3 "Wide
    // states"); the prefetching kernel when workgroups stride over chunks. SR_WIDE_NOPF=0/1 forces.
    bool use_nopf(u64 chunks) {
        if constexpr (W < 4) return false;
        if (o_.counters || wide_nopf_ == 0) return false;
        if (wide_nopf_ == 1) return true;
        return chunks <= expand_grid_cap(true);
    }

    // One expand_fast launch over a whole level whose frontier starts at arena offset `fbase`:
    // n states (dev_n = 0), or the previous level's claims read on the device (dev_n = 1, `shape`
    // is then an estimate used only for the launch shape; the grid strides over any excess).
    // chained (dev_n only): enqueued two levels ahead, the frontier's arena offset is not known to
    // the host either: the launch reads it, and the unique count, from the previous slot (SlotWork.chain).
    u32 launch_expand(u64 fbase, u32 n, bool dev_n, u64 shape, u32 undiscovered, u32 flags = 0, bool chained = false) {
        const u32 sq = next_seq();
        if (chained) fbase = 0;  // (read on the device)
        const u64 nbase = fbase + (dev_n ? 0 : n);  // start of the next level (dev_n: + n on the device)
        const u32 ncap = (u32)std::min<u64>(arena_cap_ - nbase, 0xffffffffu);
        const u32 ppw_log2 = ppw_env_ >= 0 ? (u32)ppw_env_ : ppw_for(shape);
        const u32 chunks = std::max<u32>(1, blocks_for((shape + (1u << ppw_log2) - 1) >> ppw_log2, WPB));
        const bool nopf = use_nopf(chunks);
        u32 grid = std::min(expand_grid_cap(nopf), chunks);
        const bool deep = !o_.counters && !nopf && deep_level(chunks, grid);
        if (deep) grid = std::min(expand_grid_cap(false, true), chunks);
        const bool bal = balance_level(shape, dev_n, deep);
        seq_launch_[sq] = launch_frontier.size();
        // a slotted launch: it counts into its own slot and is published by its successor
        SlotWork sw = slot_work(dev_n);
        sw.flags = flags | (action_table_ ? (u32)SLOT_ACTION_TABLE : 0u);
        sw.arena = arena_.p;
        sw.apar = apar_.p;
        sw.arena_cap = arena_cap_;
        sw.fbase = fbase;
        // unique states before the frontier (level 0 is launched before the roots' claims are read: 0)
        const u64 u = unique.load();
        sw.ubase = dev_n ? u : u >= n ? u - n : 0ull;
        if (chained) sw.chain = slot(slot_k_ - 1);
        if (dev_n) {  // speculative: the device checks its frontier against the room left (ERR_DEFERRED)
            sw.room = (u64)(lmax_ * (double)cap_);  // (the device adds the unique states before the level)
            sw.gmul = (u32)std::min(64.0 * 256.0, std::ceil(std::max(recent_ratio(), 1.0) * 1.5 * 256.0));
        }
        LevelCounters* lc = slot(slot_k_);
        const u32 svc = sw.pub || sw.zero ? 1u : 0u;  // the extra service workgroup (SlotWork)
        timed([&] {
            auto launch = [&](auto kern) {
                kern<<<grid + svc, 64 * WPB, filt_bytes(), stream_>>>(
                    m_, arena_.p + fbase * W, 0u, n, view(), arena_.p + nbase * W, apar_.p + nbase, ncap, lc,
                    undiscovered, nullptr, sq, 0u, ppw_log2, filt_arg(), sw);
            };
            launch_form(launch, nopf, deep, bal);
        }, n);
        slot_seq_ = sq;
        slot_published_ = false;
        ++slot_k_;
        return sq;
    }

    // Smallest 1500-pop block boundary inside this level at which state_count >= target.
    u64 target_limit(u64 n, u64 popped_before, u64 limit) {
        DBuf<u32> counts;
        counts.alloc(o_.device, n);
        count_successors<M><<<blocks_for(n, 256), 256, 0, stream_>>>(m_, cur(), (u32)n, counts.p);
        SR_HIP(hipGetLastError());
        std::vector<u32> h(n);
        SR_HIP(hipMemcpyAsync(h.data(), counts.p, n * sizeof(u32), hipMemcpyDeviceToHost, stream_));
        SR_HIP(stream_sync(stream_));
        u64 sc = state_count;
        u64 r = 0;
        for (u64 k = popped_before / 1500 + 1;; ++k) {
            u64 b = k * 1500 - popped_before;  // pops of this level at the block boundary
            if (b > n || b > limit) return ~0ull;
            for (; r < b; ++r) sc += h[r];
            if (sc >= o_.target_state_count) return b;
        }
    }

    // Expands frontier ranks [0, limit) of `level` into next_; returns the next frontier size.
    u64 expand_level(u32 level, u64 n, u64 limit, u32 undiscovered, const u32* peb = nullptr) {
        const u32 A = A_;  // action slots (FIFO candidate layout)
        u64 claims = 0;
        DBuf<u32> cand;
        if (fifo_) {
            cand.alloc(o_.device, limit * A);
            SR_HIP(hipMemsetAsync(cand.p, 0xff, limit * A * sizeof(u32), stream_));
        }
        const u64 nbase = lstart_.back();  // arena offset of the next level
        // New states per parent assumed when sizing a chunk: twice the last level's growth (the
        // model's max out-degree D in pessimistic mode); see run_with_restart.
        const u64 d_eff = pessimistic_ ? D_ : std::min<u64>(D_, (u64)std::ceil(2.0 * ratio_ + 1.0));
        for (u64 lo = 0; lo < limit;) {
            // Chunk so the visited set stays under 80% load.
            u64 head = (u64)(lmax_ * (double)cap_) - std::min<u64>((u64)(lmax_ * (double)cap_), unique + claims);
            u64 c = std::min<u64>(limit - lo, head / std::max<u64>(d_eff, 1));
            if (c < std::min<u64>(limit - lo, 1u << 16)) {
                grow_table(fifo_ ? cand.p : nullptr, fifo_ ? limit * A : 0);
                continue;
            }
            if (!fifo_) ensure_arena(nbase + claims + c * d_eff, nbase + claims);
            const u32 ulo = (u32)lo, uhi = (u32)(lo + c);
            const bool last = lo + c == limit;
            // repair: the chunk's first pass overflowed the probe limit (see repair_level)
            auto launch_chunk = [&](bool repair) {
                const u32 sq = next_seq();
                if (fifo_) {
                    timed([&] {
                        expand_fifo<M><<<blocks_for(c, 256), 256, 0, stream_>>>(m_, cur(), ulo, uhi, (u32)limit, view(), cand.p,
                                                                                A, level, lc_d_, hcd(sq), sq, repair ? 0u : 1u);
                    });
                } else {
                    const u32 ncap = (u32)std::min<u64>(arena_cap_ - nbase, 0xffffffffu);
                    u64* next = arena_.p + nbase * W;
                    u32* npar = apar_.p + nbase;
                    const u32 ppw_log2 = ppw_env_ >= 0 ? (u32)ppw_env_ : ppw_for(c);
                    const u32 chunks = std::max<u32>(1, blocks_for((c + (1u << ppw_log2) - 1) >> ppw_log2, WPB));
                    const bool nopf = use_nopf(chunks);
                    u32 grid = std::min(expand_grid_cap(nopf), chunks);
                    const bool deep = !o_.counters && !nopf && deep_level(chunks, grid);
                    if (deep) grid = std::min(expand_grid_cap(false, true), chunks);
                    const bool bal = balance_level(c, false, deep);
                    SlotWork sw{};
                    sw.flags = (repair ? (u32)SLOT_REPAIR : 0u) | (action_table_ ? (u32)SLOT_ACTION_TABLE : 0u);
                    if (emask_ && peb) {
                        sw.peb = peb;
                        sw.naeb = aeb_.p + nbase;
                    }
                    timed([&] {
                        auto launch = [&](auto kern) {
                            kern<<<grid, 64 * WPB, filt_bytes(), stream_>>>(
                                m_, cur(), ulo, uhi, view(), next, npar, ncap, lc_d_, undiscovered, hcd(sq), sq,
                                last ? 1u : 0u, ppw_log2, filt_arg(), sw);
                        };
                        launch_form(launch, nopf, deep, bal);
                    });
                }
                return sq;
            };
            if (!wait_publish(launch_chunk(false), true)) {
                // Double the table (FIFO: the level's candidate slots move with it) and probe the
                // chunk again: the missing states are claimed, nothing is counted twice. The
                // counters continue from the failed pass (a last FAST chunk's publish reset them).
                const HostCounters first = lc_;
                u32 dmin[MAX_PROPS];
                std::copy(first.disc, first.disc + MAX_PROPS, dmin);
                for (int attempt = 0;; ++attempt) {
                    if (attempt >= 8) throw Error(SR_ERR_CAPACITY, "visited set probe limit exceeded after 8 doublings");
                    grow_table(fifo_ ? cand.p : nullptr, fifo_ ? limit * A : 0);
                    stats.table_doublings++;
                    SR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&lc_d_->claims), (int)lc_.claims, 1, stream_));
                    SR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&lc_d_->err), 0, 1, stream_));
                    const bool ok = wait_publish(launch_chunk(true), true);
                    for (int p = 0; p < MAX_PROPS; ++p) dmin[p] = std::min(dmin[p], lc_.disc[p]);
                    if (ok) break;
                }
                lc_.successors = std::max(lc_.successors, first.successors);
                lc_.enabled = std::max(lc_.enabled, first.enabled);
                std::copy(dmin, dmin + MAX_PROPS, lc_.disc);
            }
            claims = lc_.claims;
            lo += c;
        }
        ratio_ = (double)claims / (double)limit;
        if (!fifo_) {
            en_ratio_ = std::max(1.0, (double)lc_.enabled / (double)limit);
            return claims;
        }

        // FIFO passes 2-3: owners per parent, exclusive scan, ordered scatter.
        ensure_arena(nbase + claims, nbase);
        DBuf<u32> counts, offs, sums, total;
        counts.alloc(o_.device, limit);
        offs.alloc(o_.device, limit);
        u32 tiles = blocks_for(limit, SCAN_TILE);
        sums.alloc(o_.device, tiles);
        total.alloc(o_.device, 1);
        timed([&] { own_count<M><<<blocks_for(limit, 256), 256, 0, stream_>>>(cand.p, (u32)limit, A, level, view(), counts.p); });
        scan_tile_sums<<<tiles, SCAN_BLOCK, 0, stream_>>>(counts.p, (u32)limit, sums.p);
        scan_sums<<<1, SCAN_BLOCK, 0, stream_>>>(sums.p, tiles, total.p);
        scan_tiles<<<tiles, SCAN_BLOCK, 0, stream_>>>(counts.p, (u32)limit, sums.p, offs.p);
        SR_HIP(hipGetLastError());
        const u32 sq = next_seq();
        timed([&] {
            scatter_fifo<M><<<blocks_for(limit, 256), 256, 0, stream_>>>(m_, cur(), cand.p, offs.p, (u32)limit, A, level,
                                                                         view(), arena_.p + nbase * W, apar_.p + nbase, lc_d_,
                                                                         undiscovered, hcd(sq), sq, total.p, peb,
                                                                         emask_ ? aeb_.p + nbase : nullptr);
        });
        wait_publish(sq);
        const u32 owners = lc_.aux;
        if (owners != claims) throw Error(SR_ERR_CAPACITY, "FIFO ownership mismatch: owners " + std::to_string(owners) + " claims " + std::to_string(claims));
        return owners;
    }

    // Parents per wave (log2) of the FAST kernel for a chunk of c parents. A wave walks the
    // enabled action slots of its parents 64 at a time. Light models (a few ALU ops per successor)
    // amortise the wave's setup over ~16 such rounds; heavy ones (paxos: ~1.3K VALU ops per
    // successor) want ~4 rounds per wave and more waves to hide the probe latency. Small levels
    // use fewer parents per wave until ~2K waves are in flight (minimum 4 parents per wave).
    // Measured per level with SR_PPW_LOG2 sweeps (profiles/r01_ppw_levels.txt).
    u32 ppw_for(u64 c) const {
        const double rounds = W >= 4 ? 4.0 : 16.0;
        const double ppw = 64.0 * rounds / en_ratio_;
        const u32 lmax = expand_ppw_log2_max<M>();  // expand_fast's PPW_LOG2_MAX
        u32 l = 2;
        while (l < lmax && (double)(2u << l) <= ppw) ++l;
        while (l > 2 && ((c + (1u << l) - 1) >> l) < ppw_waves_) --l;
        return l;
    }
    u64 ppw_waves_ = std::getenv("SR_PPW_WAVES") && std::atoll(std::getenv("SR_PPW_WAVES")) > 0
                         ? (u64)std::atoll(std::getenv("SR_PPW_WAVES")) : 2048;

    // The frontier being expanded: the arena's second-to-last level.
    const u64* cur() const { return arena_.p + lstart_[lstart_.size() - 2] * W; }

    M m_;
    sr_opts o_;
    u32 A_;  // action slots
    u32 D_;  // max successors of one state (bounds the new states a chunk can create)
    u32 emask_;  // the model's `eventually` properties
    u32 lmask_;  // the model's leads-to properties (live.hpp LEADS-TO): never in a kernel's `undiscovered`
    u32 smask_;  // the model's step properties (step.hpp): likewise
    bool fifo_ = false;
    int probe_batch_ = 0;  // SR_PROBE_BATCH: 1 forces the probe rounds, -4 the per-lane probe queues (0: probe_loop)
    // expand_fast's probe loop (DESIGN.md §3 "Probe loops"): rounds of one successor per lane, or
    // per-lane queues over 4 rounds (-4) once the visited set is far beyond the 256 MB Infinity
    // Cache (>= 2^27 slots), where each probe is a longer round trip: 2pc N=10 -7 %, N=11 -6 %,
    // N=9 (2^25 slots) +6 % (profiles/r05_probe_loops.txt). Fingerprint-mode narrow states only.
    int probe_loop() const {
        if (probe_batch_) return probe_batch_ < 0 ? -4 : 1;
        constexpr bool queue_ok = W == 1 || !has_qkey<M>::value;  // not multi-word quotient tables
        if (queue_ok && W < 4 && queue_ratio_ > 0 && ratio_ >= queue_ratio_) return -4;  // (measurement knob)
        return queue_ok && W < 4 && cap_ >= (1ull << 27) ? -4 : 1;
    }
    // SR_QUEUE_RATIO: the per-lane queues also for levels after one that made at least this many new
    // states per parent (the claim-heavy ascending levels; 0: off)
    double queue_ratio_ = std::getenv("SR_QUEUE_RATIO") ? std::atof(std::getenv("SR_QUEUE_RATIO")) : 0.0;
    int ppw_env_ = -1;
    bool table_recycle_ = true;  // the visited set is returned zeroed (~Engine)
    u32 grid_res_ = 2;  // residencies per expand grid (set in the constructor)
    u32 grid_max_[5] = {0, 0, 0, 0, 0};  // cap on expand_fast's grid per form (rounds, queue, wide no-prefetch,
                                   // rounds and queue with dynamic chunks);
                                   // 0 = not computed yet (two device residencies, or SR_GRID_MAX)
    u32 grid_env_ = 0;       // SR_GRID_MAX
    int wide_nopf_ = -1;     // SR_WIDE_NOPF: -1 chosen per level (use_nopf), 0 never, 1 always
    // The pipelined loop enqueues a second level ahead (chained) while the next frontier is
    // estimated at <= this many states (SR_CHAIN_MAX; 0: never).
    u64 chain_max_ = 16384;
    // Early growth of an unhinted visited set happens while the frontier is at most this large
    // (SR_EARLY_GROW_MAX; 0: never).
    u64 early_grow_max_ = std::getenv("SR_EARLY_GROW_MAX") ? std::strtoull(std::getenv("SR_EARLY_GROW_MAX"), nullptr, 10)
                                                           : (u64)1 << 17;
    int table_kind_ = 0;  // DevicePool memory kind of the visited set (SR_TABLE_KIND, measurement knob)
    // the no-prefetch form exists for wide states only (it is the prefetching kernel otherwise)
    template <class L>
    void launch_nopf(L& launch, bool bal) {
        if constexpr (W >= 4) bal ? launch(expand_fast<M, 1, 0, false, true, false, true>) : launch(expand_fast<M, 1, 0, false, true>);
    }
    u64 query_mask_ = 4095;  // spins between hipStreamQuery calls in wait_publish (SR_QUERY_LOG2)
    bool pipeline_ = true;  // FAST-order level pipelining (SR_PIPELINE=0 disables, for A/B runs)
    DBuf<u64> slots_;                 // SLOTS per-level counter slots (the pipelined loop)
    u32 slot_k_ = 0;                  // slotted launches in this run
    u32 slot_seq_ = 0;                // sequence number of the last one
    bool slot_published_ = true;      // its publish is done or enqueued
    std::map<u32, size_t> seq_launch_;  // launch sequence number -> index in launch_frontier
    u32 filt_log2_ = default_filter_log2<W>();  // block-local duplicate filter
    bool filt_compact_ = false;         // ... in 4-byte entries (kernels.hpp FILT_COMPACT)
    size_t filt_bytes() const { return filt_log2_ ? (size_t)(filt_compact_ ? 4u : 8u) << filt_log2_ : 0u; }
    u32 filt_arg() const { return filt_log2_ | (filt_compact_ ? FILT_COMPACT : 0u); }
    bool pessimistic_ = false;  // size chunks for max out-degree new states per parent
    u64 grow_factor_ = 1;       // initial-capacity multiplier after a capacity restart
    double ratio_ = 1.0;        // new states per expanded parent in the last level
    double ratios_[4] = {};     // ... in the last four levels (a model's growth can be periodic:
    u32 nratio_ = 0;            // increment_lock grows x5 every fourth level)
    void note_ratio(double r) { ratios_[nratio_++ & 3] = r; }
    double recent_ratio() const {
        double m = ratio_;
        for (u32 i = 0; i < std::min<u32>(nratio_, 4); ++i) m = std::max(m, ratios_[i]);
        return m;
    }
    double en_ratio_ = 8.0;     // enabled action slots per expanded parent in the last level
    // planned load of the visited set at the capacity hint (SR_TABLE_LOAD): 0.3 with 4-byte slots (2pc
    // N=9: 2^26 slots, 256 MiB, 1.615 -> 1.565 ms; N=10 8.64 -> 7.89 ms; profiles/r06_table_load.txt)
    double table_load_ = 0.3;
    bool load_env_ = false;
    Ctx* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
    HostCounters lc_{};  // host copy of the last published counters
    LevelCounters* lc_d_ = nullptr;
    u64 cap_ = 0;
    DBuf<u64> keys_, meta_;      // visited set
    double lmax_ = 0.8;          // growth threshold of the current table (max_load)
    Clock::time_point vt0_{};    // verbose log: start of the level loop
    DBuf<u32> aux_;              // [0] rehash error bits, [1] max displacement (displacement_stats)
    DBuf<u64> arena_;            // BFS tree: every level's states in visit order
    DBuf<u32> apar_;             // parent rank (in the previous level) of each arena state
    DBuf<u32> aeb_;              // EventuallyBits of each arena state (models with eventually properties)
    u64 arena_cap_ = 0;          // states
    std::vector<u64> lstart_;    // arena offset of each level (+ one past the newest)
    std::vector<u64> lvisited_;  // states of each level that the reference would pop
};

}  // namespace sr

#include "dist.hpp"

namespace sr {

// The fingerprint of a state given by its canonical description (the integers of
// sr_gpu_bfs_discovery_path / `describe`): what a host that holds the state compares with a
// discovery's fingerprint chain (`Path::from_fingerprints`, src/checker/path.rs:20-86).
// The description must be canonical: undescribe masks its fields, so a malformed or contradictory
// description (a paxos Get return value for a client still in phase 1, a field out of range) would
// otherwise map to some state and a plausible fingerprint. It is described again and compared.
template <class M>
int described_fingerprint(const M& m, const i64* d, int width, u64* fp, std::string* why = nullptr) {
    if constexpr (has_undescribe<M>::value) {
        if (!d || !fp || width != m.describe_width()) {
            if (why) *why = "bad description width";
            return SR_ERR_ARG;
        }
        u64 s[M::W];
        m.undescribe(d, s);
        std::vector<i64> back((size_t)width);
        m.describe(s, back.data());
        for (int i = 0; i < width; ++i)
            if (back[i] != d[i]) {
                if (why)
                    *why = "not a canonical state description (element " + std::to_string(i) + ": " + std::to_string(d[i]) +
                           " describes back as " + std::to_string(back[i]) + ")";
                return SR_ERR_ARG;
            }
        *fp = state_fp<M>(s);
        return SR_OK;
    } else {
        (void)m, (void)d, (void)width, (void)fp;
        if (why) *why = "model has no state description inverse";
        return SR_ERR_UNSUPPORTED;
    }
}

// ---- plugins: a GpuModel compiled into its own shared library (include/stateright_gpu_model.hpp) ----
// MAKE(params, nparams, device) builds the model (device < 0: host-only use); it may throw Error.
inline sr_opts normalized_opts(const sr_opts* opts) {
    sr_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(sr_opts);
    if (opts) std::memcpy(&o, opts, std::min<size_t>(sizeof(o), opts->struct_size ? opts->struct_size : sizeof(o)));
    return o;
}

template <class M, class Make>
void* plugin_create(Make make, const int64_t* p, int32_t np, const sr_opts* opts, void* comm, int32_t vparts, char* err,
                    int32_t errcap) {
    try {
        const sr_opts o = normalized_opts(opts);
        M m = make(p, np, o.device);
        EngineBase* e = nullptr;
        if (o.symmetry) {
            if constexpr (has_canonical<M>::value) {
                if (comm || vparts > 1) e = new DistEngine<Canon<M>>(Canon<M>(m), o, static_cast<Comm*>(comm), (int)vparts);
                else e = new Engine<Canon<M>>(Canon<M>(m), o);
            } else {
                throw Error(SR_ERR_UNSUPPORTED, "symmetry reduction: the plugin model has no `canonical`");
            }
        } else if (comm || vparts > 1) {
            if constexpr (has_emask<M>::value) {
                if (model_emask(m)) e = new DistEngine<EvBits<M>>(EvBits<M>(m), o, static_cast<Comm*>(comm), (int)vparts);
            }
            if (!e) e = new DistEngine<M>(m, o, static_cast<Comm*>(comm), (int)vparts);
        } else {
            e = new Engine<M>(m, o);
        }
        return e;
    } catch (const std::exception& x) {
        if (err && errcap > 0) std::snprintf(err, (size_t)errcap, "%s", x.what());
        return nullptr;
    }
}

template <class M, class Make>
int32_t plugin_fingerprint(Make make, const int64_t* p, int32_t np, const int64_t* d, int32_t width, uint64_t* fp) {
    try {
        return described_fingerprint(make(p, np, -1), d, width, fp);
    } catch (const Error& x) {
        return x.code;
    } catch (const std::exception&) {
        return SR_ERR_ARG;
    }
}

}  // namespace sr
