// The compiled-in GpuModel registry, split into families that compile as separate translation units
// (reg_*.hip, built in parallel by stateright_amd/build.py and linked into libstateright_gpu.so).
// Each family instantiates the single-GPU Engine<M>, the partitioned DistEngine<M> and the simulation
// checker SimEngine<M> (sim.hpp) for its models; engine.hip maps a model id (SR_MODEL_*) to its family.
#pragma once
#include <memory>

#include "engine.hpp"
#include "dist.hpp"
#include "sim.hpp"

namespace sr {

// What a spawn asks for: the model's integer parameters and options, and for the partitioned
// search its communicator (or none) and virtual partitions; for a simulation (sim != nullptr) the
// walk options, with `o` carrying the device only.
struct EngineArgs {
    int model;
    const i64* p;
    int np;
    const sr_opts* o;
    bool dist;
    Comm* comm;
    int vparts;
    const sr_sim_opts* sim = nullptr;
    void need(int k) const {
        if (np < k) throw Error(SR_ERR_ARG, "model " + std::to_string(model) + " needs " + std::to_string(k) + " params");
    }
};

// Engine<M>, DistEngine<M> or SimEngine<M> (plain models only: no Canon<M>, no EvBits<M>). EV: a model with `eventually` properties runs partitioned as
// EvBits<M> (models.hpp).
template <class M, bool EV = false>
std::unique_ptr<EngineBase> make_for(const M& m, const EngineArgs& a) {
    if (a.sim) {
        if constexpr (is_canon<M>::value || is_evbits<M>::value) throw Error(SR_ERR_UNSUPPORTED, "simulation: symmetry reduction has no counterpart");
        else return std::make_unique<SimEngine<M>>(m, *a.sim);
    }
    if (!a.dist) return std::make_unique<Engine<M>>(m, *a.o);
    if constexpr (EV && has_emask<M>::value) {
        if (model_emask(m)) return std::make_unique<DistEngine<EvBits<M>>>(EvBits<M>(m), *a.o, a.comm, a.vparts);
    }
    return std::make_unique<DistEngine<M>>(m, *a.o, a.comm, a.vparts);
}

// One function per family (reg_<family>.hip): the engine of a.model.
std::unique_ptr<EngineBase> reg_basic(const EngineArgs& a);           // LinearEquation, BinaryClock, DGraph, actor fixtures
std::unique_ptr<EngineBase> reg_two_phase(const EngineArgs& a);       // 2pc (and its canonical reduction)
std::unique_ptr<EngineBase> reg_increment(const EngineArgs& a);       // increment
std::unique_ptr<EngineBase> reg_increment_lock(const EngineArgs& a);  // increment_lock
std::unique_ptr<EngineBase> reg_paxos(const EngineArgs& a);           // paxos, 1-4 clients (W = 11)
std::unique_ptr<EngineBase> reg_paxos_wide(const EngineArgs& a);      // paxos, 5-6 clients (W = 12)
std::unique_ptr<EngineBase> reg_ping_pong(const EngineArgs& a);       // ping-pong
std::unique_ptr<EngineBase> reg_registers(const EngineArgs& a);       // ABD (8 slots) and the single-copy register
std::unique_ptr<EngineBase> reg_registers_wide(const EngineArgs& a);  // ABD, 16 and 32 network slots (W = 14, 22)
std::unique_ptr<EngineBase> reg_spread(const EngineArgs& a);          // the Spread fixture (W = 1, 2, 4), LiveGraph
std::unique_ptr<EngineBase> reg_two_phase_live(const EngineArgs& a);  // 2pc with `eventually` properties (TwoPhaseLive)
std::unique_ptr<EngineBase> reg_spin_lock(const EngineArgs& a);       // SpinLock
std::unique_ptr<EngineBase> reg_fair_rings(const EngineArgs& a);      // FairRings
std::unique_ptr<EngineBase> reg_leads(const EngineArgs& a);           // LeadsGraph (W = 1, 2, 4), LeadsDGraph
std::unique_ptr<EngineBase> reg_req_lock(const EngineArgs& a);        // ReqLock, 1..4 threads
std::unique_ptr<EngineBase> reg_req_lock_wide(const EngineArgs& a);   // ReqLock, 5..8 threads
std::unique_ptr<EngineBase> reg_step(const EngineArgs& a);            // StepGraph (W = 1, 2, 4), StepDGraph, TwoPhaseStep

// SpinLock (models.hpp) of (threads), handed to f: the engine (reg_spin_lock.hip) and the host-only entry
// points (engine.hip) validate alike.
template <class F>
auto with_spin_lock(const i64* p, int np, F&& f) {
    if (np < 1) throw Error(SR_ERR_ARG, "spin-lock needs 1 param (threads)");
    if (p[0] < 1 || p[0] > 20) throw Error(SR_ERR_UNSUPPORTED, "spin-lock: threads must be in 1..=20");
    return f(SpinLock{(int)p[0]});
}

// FairRings (models.hpp) of (d, w, core, lanes), handed to f: the engine (reg_fair_rings.hip) and the
// host-only entry points (engine.hip) validate alike.
template <class F>
auto with_fair_rings(const i64* p, int np, F&& f) {
    if (np < 4) throw Error(SR_ERR_ARG, "fair-rings needs 4 params (d, w, core, lanes)");
    if (p[0] < 1 || p[0] > 28) throw Error(SR_ERR_UNSUPPORTED, "fair-rings: d must be in 1..=28");
    if (p[1] < 4 || p[1] > 64) throw Error(SR_ERR_UNSUPPORTED, "fair-rings: w must be in 4..=64");
    if (p[2] < 0 || p[2] > 2) throw Error(SR_ERR_ARG, "fair-rings: core must be 0, 1 or 2");
    if (p[3] < 1 || p[3] > 512) throw Error(SR_ERR_UNSUPPORTED, "fair-rings: lanes must be in 1..=512");
    return f(FairRings{(int)p[0], (int)p[1], (int)p[2], (int)p[3]});
}

// TwoPhaseLive (models.hpp) of (rm_count), handed to f: the engines (reg_two_phase_live.hip) and the
// host-only entry points (engine.hip) validate alike.
template <class F>
auto with_two_phase_live(const i64* p, int np, F&& f) {
    if (np < 1) throw Error(SR_ERR_ARG, "2pc-live needs 1 param (rm_count)");
    if (p[0] < 1 || p[0] > 14) throw Error(SR_ERR_UNSUPPORTED, "2pc-live: rm_count must be in 1..=14 (4n+4 <= 63 bits)");
    return f(TwoPhaseLive{{(int)p[0], 0}});
}

// The LiveGraph fixture (models.hpp) of (n_bits, degree, seed, p_mod, t_mod, roots) and optionally words
// (default 1) and dup (default 0), handed to f: the engines (reg_spread.hip) and the host-only entry points (engine.hip)
// validate alike.
template <class F>
auto with_live_graph(const i64* p, int np, F&& f) {
    if (np < 6 || np > 8) throw Error(SR_ERR_ARG, "live graph needs 6 params (n_bits, degree, seed, p_mod, t_mod, roots) and optionally words, dup");
    if (p[0] < 1 || p[0] > 24) throw Error(SR_ERR_UNSUPPORTED, "live graph: n_bits must be in 1..=24");
    if (p[1] < 1 || p[1] > 4) throw Error(SR_ERR_UNSUPPORTED, "live graph: degree must be in 1..=4");
    if (p[3] < 0 || p[3] > 0xffffffffll || p[4] < 0 || p[4] > 0xffffffffll)
        throw Error(SR_ERR_ARG, "live graph: p_mod and t_mod must be in 0..2^32-1");
    if (p[5] < 1 || p[5] > 512 || p[5] > (i64)1 << p[0]) throw Error(SR_ERR_ARG, "live graph: roots must be in 1..=min(512, 2^n_bits)");
    const i64 w = np > 6 ? p[6] : 1;
    if (w != 1 && w != 2 && w != 4) throw Error(SR_ERR_UNSUPPORTED, "live graph: words must be 1, 2 or 4");
    const i64 dup = np > 7 ? p[7] : 0;
    if (dup < 0 || dup > p[5] || p[5] + dup > 512) throw Error(SR_ERR_ARG, "live graph: dup must be in 0..=roots, roots + dup at most 512");
    if (w == 1) return f(LiveGraphT<1>{(int)p[0], (int)p[1], (u64)p[2], (u32)p[3], (u32)p[4], (int)p[5], (int)dup});
    if (w == 2) return f(LiveGraphT<2>{(int)p[0], (int)p[1], (u64)p[2], (u32)p[3], (u32)p[4], (int)p[5], (int)dup});
    return f(LiveGraphT<4>{(int)p[0], (int)p[1], (u64)p[2], (u32)p[3], (u32)p[4], (int)p[5], (int)dup});
}

// The LeadsGraph fixture (models.hpp) of (n_bits, degree, seed, p_mod, t_mod, roots, q_mod) and optionally words
// and dup: LiveGraph's parameters with q_mod behind roots, handed to f.
template <class F>
auto with_leads_graph(const i64* p, int np, F&& f) {
    if (np < 7 || np > 9)
        throw Error(SR_ERR_ARG, "leads graph needs 7 params (n_bits, degree, seed, p_mod, t_mod, roots, q_mod) and optionally words, dup");
    if (p[6] < 0 || p[6] > 0xffffffffll) throw Error(SR_ERR_ARG, "leads graph: q_mod must be in 0..2^32-1");
    i64 lp[8] = {p[0], p[1], p[2], p[3], p[4], p[5], np > 7 ? p[7] : 1, np > 8 ? p[8] : 0};
    return with_live_graph(lp, 8, [&](const auto& g) {
        constexpr int GW = std::decay_t<decltype(g)>::W;
        LeadsGraphT<GW> m;
        static_cast<LiveGraphT<GW>&>(m) = g;
        m.q_mod = (u32)p[6];
        return f(m);
    });
}

// The StepGraph fixture (models.hpp) of (n_bits, degree, seed, f_mod, t_mod, roots) and optionally words and
// dup: LiveGraph's parameters with f_mod (any non-negative int64) in p_mod's place, handed to f.
template <class F>
auto with_step_graph(const i64* p, int np, F&& f) {
    if (np < 6 || np > 8) throw Error(SR_ERR_ARG, "step graph needs 6 params (n_bits, degree, seed, f_mod, t_mod, roots) and optionally words, dup");
    if (p[3] < 0) throw Error(SR_ERR_ARG, "step graph: f_mod must not be negative");
    i64 lp[8] = {p[0], p[1], p[2], 0, p[4], p[5], np > 6 ? p[6] : 1, np > 7 ? p[7] : 0};
    return with_live_graph(lp, 8, [&](const auto& g) {
        constexpr int GW = std::decay_t<decltype(g)>::W;
        StepGraphT<GW> m;
        static_cast<LiveGraphT<GW>&>(m) = g;
        m.f_mod = (u64)p[3];
        return f(m);
    });
}

// TwoPhaseStep (models.hpp) of (rm_count), handed to f.
template <class F>
auto with_two_phase_step(const i64* p, int np, F&& f) {
    if (np < 1) throw Error(SR_ERR_ARG, "2pc-step needs 1 param (rm_count)");
    if (p[0] < 1 || p[0] > 14) throw Error(SR_ERR_UNSUPPORTED, "2pc-step: rm_count must be in 1..=14 (4n+4 <= 63 bits)");
    return f(TwoPhaseStep{{(int)p[0], 0}});
}

// ReqLock (models.hpp) of (threads), handed to f as ReqLockT<threads>: the engines (reg_req_lock.hip for LO = 1,
// threads 1..4; reg_req_lock_wide.hip for LO = 5, threads 5..8: two units, since every thread count is a model
// of its own) and the host-only entry points (engine.hip, both ranges) validate alike.
inline void req_lock_threads(const i64* p, int np) {
    if (np < 1) throw Error(SR_ERR_ARG, "req-lock needs 1 param (threads)");
    if (p[0] < 1 || p[0] > 8) throw Error(SR_ERR_UNSUPPORTED, "req-lock: threads must be in 1..=8");
}
template <int LO, class F>
auto with_req_lock_range(const i64* p, int np, F&& f) {
    req_lock_threads(p, np);
    switch (p[0] - LO) {
        case 0: return f(ReqLockT<LO>{});
        case 1: return f(ReqLockT<LO + 1>{});
        case 2: return f(ReqLockT<LO + 2>{});
        case 3: return f(ReqLockT<LO + 3>{});
    }
    throw Error(SR_ERR_ARG, "req-lock: threads outside this unit's range");
}
template <class F>
auto with_req_lock(const i64* p, int np, F&& f) {
    req_lock_threads(p, np);
    return p[0] <= 4 ? with_req_lock_range<1>(p, np, f) : with_req_lock_range<5>(p, np, f);
}

// The Spread fixture (models.hpp) of the parameters (words, key_bits, free_bits, loops, mark) and
// optionally (roots, dup), its init states (default 1, 0), handed to f: the engines (reg_spread.hip) and the host-only entry points (engine.hip) validate alike.
template <class F>
auto with_spread_model(const i64* p, int np, F&& f) {
    if (np < 5) throw Error(SR_ERR_ARG, "spread needs 5 params (words, key_bits, free_bits, loops, mark)");
    const i64 w = p[0], b = p[1], fb = p[2], loops = p[3], mark = p[4];
    if (w != 1 && w != 2 && w != 4) throw Error(SR_ERR_UNSUPPORTED, "spread: words must be 1, 2 or 4");
    if (fb < 1 || fb > 24) throw Error(SR_ERR_UNSUPPORTED, "spread: free_bits must be in 1..=24");
    if (b <= fb || b > std::min<i64>(64 * w, 128))
        throw Error(SR_ERR_UNSUPPORTED, "spread: free_bits < key_bits <= min(64 words, 128)");
    if (loops < 0 || loops > 4) throw Error(SR_ERR_UNSUPPORTED, "spread: loops must be in 0..=4");
    if (mark < 0 || mark >> fb) throw Error(SR_ERR_ARG, "spread: mark must be below 2^free_bits");
    const i64 roots = np > 5 ? p[5] : 1, dup = np > 6 ? p[6] : 0;
    if (np > 7) throw Error(SR_ERR_ARG, "spread takes at most 7 params (.., roots, dup)");
    if (roots < 1 || roots > (i64)1 << fb) throw Error(SR_ERR_ARG, "spread: roots must be in 1..=2^free_bits");
    if (dup < 0 || dup > roots) throw Error(SR_ERR_ARG, "spread: dup must be in 0..=roots");
    if (roots + dup > 512) throw Error(SR_ERR_UNSUPPORTED, "spread: roots + dup must be at most 512");
    if (w == 1) return f(Spread<1>{(int)b, (int)fb, (int)loops, (u64)mark, (int)roots, (int)dup});
    if (w == 2) return f(Spread<2>{(int)b, (int)fb, (int)loops, (u64)mark, (int)roots, (int)dup});
    return f(Spread<4>{(int)b, (int)fb, (int)loops, (u64)mark, (int)roots, (int)dup});
}

}  // namespace sr
