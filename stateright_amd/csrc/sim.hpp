// Random-walk simulation checker: the counterpart of the simulation checker Stateright gained after
// the 0.28 this engine mirrors. Many independent random traces ("walks") run from the init states,
// the properties are evaluated on every state of a walk, and NO visited set is kept: a check whose
// reachable set fits no card still gets discoveries. A run without a discovery proves nothing.
//
// The walk is defined ONCE here, as SR_HD templates over a GpuModel M (models.hpp): the kernel
// (kernels_sim.hpp simulate_walks) and the host re-walk (sim_host_walk: discovery paths, the
// host-only sr_sim_walk entry point) instantiate the same code, so a walk is a pure function of
// (model, seed, walk index w, max_depth, loops), on either side (loops: the opt-in loop detection
// below; off by default).
//
// Randomness (part of the definition). A counter-based generator, no per-lane state:
//   sim_walk_key(seed, w) = fmix64(seed + 0x9E3779B97F4A7C15 * (w + 1))
//   r(seed, w, t, k)      = fmix64((sim_walk_key(seed, w) ^ (t << 32 | k)) + 0x632BE59BD9B4E019)
// t is the step (0 .. max_depth <= 2^20), k the attempt of that step; the init state is drawn with
// t = 0, k = SIM_K_INIT (no attempt count reaches it: max_actions is an int). fmix64 is a bijection,
// so for one walk distinct (t, k) give distinct draws' inputs. To choose one of n:
//   sim_choose(r, n) = ((r >> 32) * n) >> 32          (n < 2^32; no modulo)
//
// The walk of index w:
//   s_0 = init state number sim_choose(r(seed, w, 0, SIM_K_INIT), init_count) of init_states_of(m).
//   Visiting s_t: one state is counted; then for every property p, in order:
//     always / sometimes with discovers(p, s_t): a hit (p, t, w) (the first of the walk per property);
//     eventually with discovers(p, s_t): bit p of the walk's `sat` mask is set.
//   If the model has `faulted` and it holds at s_t, the walk ends with SIM_FAULT.
//   If t == max_depth the walk ends with SIM_DEPTH (a non-terminal end records nothing for
//   `eventually`: `assert_discovery` demands a terminal last state, src/checker.rs:306-323).
//   Stepping: mask = enabled(s_t), attempt k = 0. While mask is non-empty: a = its
//   sim_choose(r(seed, w, t, k), popcount(mask))-th set bit (ascending slot order); if
//   apply(s_t, a, out) then s_{t+1} = out; else bit a is cleared and k += 1 (`next_state` is None
//   or outside the boundary, src/checker/bfs.rs:231-234). If the mask runs empty, s_t is terminal:
//   every `eventually` property not in `sat` is a hit (p, t, w) and the walk ends with SIM_TERMINAL
//   (bfs.rs:265-272).
// The walk uses the model's plain `enabled` and `apply` (2pc's self-loop actions are steps like any
// other); `enabled_moves` and `self_loops` would change which slots are candidates. Canon<M> and
// EvBits<M> are not simulated. Every loop is bounded: steps by max_depth (<= 2^20), redraws by the
// number of enabled slots (<= max_actions).
//
// Loop detection (opt-in: sr_sim_opts.loops, `spawn_simulation(detect_loops=True)`). A trace is a
// path, so a trace that returns to a state it has visited is a lasso: a finite prefix and a cycle that
// can repeat forever. If an `eventually` property held nowhere on it, that infinite execution refutes
// the property (as the reference defines `eventually`: no fairness assumption), which neither the
// plain walk nor BFS can report (src/checker.rs:400-413, the FIXME's [0, 2, 4, 2]). With loops on a
// walk also keeps a loop memory of fingerprints f_i = state_fp<M>(s_i):
//   window:     the fingerprints of the last min(t, R) states before s_t, R = SIM_LOOP_WINDOW = 8;
//   checkpoint: a pair (f_c, t_c), initially (f_0, 0).
// Visiting s_t gains one step, after the property visit and the `faulted` test and BEFORE the
// t == max_depth test. For t >= 1: let j be the largest index in the window with f_j == f_t; failing
// that, j = t_c if f_c == f_t. If there is such a j the walk ends at s_t with SIM_LOOP and
// loop_start = j, and every `eventually` property not in `sat` is a hit (p, t, w), exactly as at a
// terminal state. Otherwise f_t enters the window, and if t is a power of two the checkpoint
// becomes (f_t, t). So:
//   a cycle of length <= 8, self-loops included, is reported at its first closure, with the
//     shortest lasso;
//   a longer cycle is reported once the walk returns to a checkpoint: a checkpoint taken at 2^k is
//     held for 2^k steps, so in a finite recurrent component that happens with probability 1 as the
//     depth grows (a deterministic lasso of prefix mu and cycle length L > 8 ends at the first
//     t = 2^k + L with 2^k >= max(mu, L), j = 2^k: L = 12, mu <= 16 gives (t, j) = (28, 16));
//   the generator is counter-based and the loop memory feeds nothing back into the walk, so the
//     loop-mode walk w is exactly the plain walk w cut at its first detection;
//   a walk that closed a loop has nothing new to show on it, and its lane is free for another walk.
// Fingerprints are compared, not states: the device and sim_host_walk may end a walk on a
// collision of two 64-bit fingerprints, but a discovery path is only returned after s_j and s_t
// were compared word for word (SimEngine::discovery_walk fails the call otherwise).
//
// A check (SimEngine) runs the walks 0 .. walks-1 in batches of consecutive indices, one launch per
// batch, and stops after the first WHOLE batch at whose end every property has a hit, state_count
// reached target_state_count, or the walks are exhausted; so a check is a deterministic function of
// (model, seed, walks, max_depth, batch size). Per property the hit with the smallest (t, w) is
// kept: the shortest trace, ties to the lowest walk index. There is no visited set, so
// `unique` is SET EQUAL to state_count (every visited state counts, repeats included) unless the
// distinct-state count below is on, `max_depth` is the longest walk in steps, and `is_done` means
// "every property discovered".
//
// Distinct-state count (opt-in: sr_sim_opts.unique, `spawn_simulation(count_unique=True)`; with it
// off no kernel, count, record, hit or allocation changes). For a check that ran the walks 0 .. n-1:
//   U = { state_fp<M>(s_t) : 0 <= w < n, 0 <= t <= steps(w) }
// Every state a walk visits is in U, its init state and its last state included, whatever the end
// reason: exactly the states state_count counts (with loops on, the states of the cut walk). The
// mode feeds nothing back into the walk: walk w, its record, its hits and the check's stop point
// are bit-identical with the mode on or off (the stop rule `stale_batches`, which exists only with
// the mode on, aside). U is a union, so it does not depend on lane, wave, launch order or the form
// of the kernel, and |U|, the set and the number of new fingerprints per batch are deterministic
// functions of (model, seed, walks run, max_depth, loops, batch size). Fingerprints are compared,
// not states: exact for one-word states (state_fp is a bijection there), a 64-bit hash for wider
// ones, so n distinct states lose one to a collision with probability ~n^2 / 2^65.
// The host form is sim_unique_host below (sim_host_walk's fingerprints, sorted, distinct); the
// device form inserts into a table in HBM while it walks (kernels_sim.hpp "Distinct-state table").
// The table (both sides agree on it; only the device keeps one): `slots` 8-byte slots, a power of
// two >= 2, 0 = vacant as in the BFS fingerprint table (kernels.hpp: state_fp is never 0, a one-word
// fingerprint by construction, a wider one by the remap of 0 to 1 in fingerprint<W>, so no state
// is mistaken for a vacant slot; the two wide states that hash to 0 and 1 count as one, which is
// the collision above). Home slot sim_unique_home(f), linear probing, at most
// sim_unique_probe_limit(slots) = min(slots, 1024) probes; an insert that exhausts them is dropped
// and raises the overflow flag: |U| is then a lower bound (the host says so: unique_overflow).
// A slot goes vacant -> fingerprint exactly once and nothing is ever removed, so while |U| <= slots
// <= 1024 no insert is dropped (a probe sequence covers the whole table), and an overflow there
// means the table is full: the count equals slots.
#pragma once
#include "engine.hpp"

namespace sr {

enum SimEnd : u32 { SIM_RUNNING = 0, SIM_TERMINAL = 1, SIM_DEPTH = 2, SIM_FAULT = 3, SIM_LOOP = 4, SIM_ENDS = 5 };
constexpr u32 SIM_LOOP_WINDOW = 8;  // a power of two: slot t % SIM_LOOP_WINDOW holds f_t
constexpr u32 SIM_NO_LOOP = ~0u;
constexpr u32 SIM_K_INIT = 0xFFFFFFFFu;
constexpr u32 SIM_MAX_DEPTH = 1u << 20;
constexpr u64 SIM_MAX_WALKS = 1ull << 40;
constexpr u64 SIM_NO_HIT = ~0ull;
constexpr u64 SIM_UNIQUE_MAX_CAPACITY = 1ull << 28;  // the default capacity's cap: 2^29 slots, 4 GiB
constexpr u32 SIM_UNIQUE_MAX_PROBES = 1024;
constexpr u64 SIM_UNIQUE_MAX_REQUEST = 1ull << 30;  // the largest unique_capacity accepted: 2^31 slots, 16 GiB
constexpr u32 SIM_UNIQUE_TAIL = 16;  // words behind the slots: the overflow flag, the gather's cursor

// The distinct-state table's geometry ("Distinct-state count" above).
// Slots for a capacity of c fingerprints: the smallest power of two >= 2 c (load <= 0.5).
SR_HD u64 sim_unique_slots(u64 c) {
    u64 s = 2;
    while (s < 2 * c) s <<= 1;
    return s;
}
SR_HD u32 sim_unique_log2(u64 slots) { return (u32)__builtin_ctzll(slots); }
SR_HD u32 sim_unique_probe_limit(u64 slots) { return (u32)(slots < SIM_UNIQUE_MAX_PROBES ? slots : SIM_UNIQUE_MAX_PROBES); }
// Home slot: the top log2(slots) bits of the fingerprint times 2^64 / phi (a mix of all its bits; a
// one-word fingerprint is fmix64 of a small integer, whose low bits alone are as good, but nothing
// here relies on that).
SR_HD u64 sim_unique_home(u64 f, u32 log2_slots) { return (f * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots); }

SR_HD u64 sim_walk_key(u64 seed, u64 w) { return fmix64(seed + 0x9E3779B97F4A7C15ull * (w + 1)); }
SR_HD u64 sim_rand_keyed(u64 key, u32 t, u32 k) { return fmix64((key ^ ((u64)t << 32 | k)) + 0x632BE59BD9B4E019ull); }
SR_HD u64 sim_rand(u64 seed, u64 w, u32 t, u32 k) { return sim_rand_keyed(sim_walk_key(seed, w), t, k); }
SR_HD u32 sim_choose(u64 r, u32 n) { return (u32)(((r >> 32) * (u64)n) >> 32); }
// Key of a hit: the minimum over hits is the shortest trace, then the lowest walk index.
SR_HD u64 sim_hit_key(u32 t, u64 w) { return (u64)t << 40 | w; }

// A walk in progress: what a lane of the kernel keeps in registers.
template <class M>
struct SimWalk {
    u64 s[M::W];
    u64 key;        // sim_walk_key(seed, w)
    u32 t;          // steps taken so far: s is s_t
    u32 sat;        // `eventually` properties whose condition held on the way
    u32 hit;        // always / sometimes properties this walk already reported
    u32 redraws;    // slots drawn whose apply() refused (all steps)
};

template <class M>
SR_HD void sim_start(SimWalk<M>& wk, u64 seed, u64 w, const u64* inits, u32 init_count) {
    wk.key = sim_walk_key(seed, w);
    const u32 i = sim_choose(sim_rand_keyed(wk.key, 0, SIM_K_INIT), init_count);
#pragma unroll
    for (int j = 0; j < M::W; ++j) wk.s[j] = inits[(size_t)i * M::W + j];
    wk.t = 0;
    wk.sat = 0;
    wk.hit = 0;
    wk.redraws = 0;
}

// The j-th (0-based, ascending) set bit of a mask of MW words holding more than j set bits.
template <int MW>
SR_HD int sim_select(const u64* mask, u32 j) {
    int a = 0;
#pragma unroll
    for (int w = 0; w < MW; ++w) {
        const u32 c = (u32)__builtin_popcountll(mask[w]);
        if (j < c) {
            u64 bits = mask[w];
            for (u32 i = 0; i < j; ++i) bits &= bits - 1;  // (j < 64)
            a = w * 64 + __builtin_ctzll(bits);
            break;
        }
        j -= c;
    }
    return a;
}

// The loop memory of a walk (loop detection on). Ring stores the window: get(slot) / put(slot, f)
// over SIM_LOOP_WINDOW slots, an array on the host (SimRingArray), a view of the workgroup's LDS in
// the kernel (kernels_sim.hpp SimRingLds). Nothing is reset between walks: the valid slots are
// derived from the walk's own t, so a lane that takes a new walk never reads its predecessor's.
struct SimRingArray {
    u64 f[SIM_LOOP_WINDOW] = {};
    SR_HD u64 get(u32 slot) const { return f[slot]; }
    SR_HD void put(u32 slot, u64 v) { f[slot] = v; }
};
template <class Ring>
struct SimLoops {
    static constexpr bool on = true;
    Ring ring;
    u64 cf = 0;                // checkpoint: f_c
    u32 ct = 0;                //             t_c
    u32 start = SIM_NO_LOOP;   // loop_start of a walk that ended with SIM_LOOP
};
struct SimNoLoops {  // loop detection off: sim_advance compiles to the plain walk
    static constexpr bool on = false;
};

// state_fp<M>(s_t) for sim_advance's loop memory: computed there (SimFpOwn), or handed in by a caller
// that has it already (SimFpGiven: the kernel's distinct-state insert), so that it is computed once.
struct SimFpOwn {
    static constexpr bool given = false;
};
struct SimFpGiven {
    static constexpr bool given = true;
    u64 f;
};

// Visits s_t and takes one step. emask: the model's `eventually` properties (the others are reported
// where discovers() holds). on_hit(p, t) is called for every hit of the walk; on_step(s_t, a)
// before the walk moves on through slot a. lp: SimLoops<Ring> or SimNoLoops.
// Returns SIM_RUNNING (wk now holds s_{t+1}) or the reason the walk ended at s_t.
template <class M, class Hit, class Step, class Loops, class Fp = SimFpOwn>
SR_HD u32 sim_advance(const M& m, SimWalk<M>& wk, u32 max_depth, u32 emask, Hit&& on_hit, Step&& on_step, Loops& lp,
                      const Fp& fpv = Fp{}) {
    u32 skip = 0;  // leads-to properties (models.hpp has_lmask) are left unchecked: a walk decides none
    if constexpr (has_lmask<M>::value) skip = m.lmask();
#pragma unroll
    for (int p = 0; p < M::NPROPS; ++p) {
        if (emask >> p & 1) {
            if (!(wk.sat >> p & 1) && m.discovers(p, wk.s)) wk.sat |= 1u << p;
        } else if (!((wk.hit | skip) >> p & 1) && m.discovers(p, wk.s)) {
            wk.hit |= 1u << p;
            on_hit(p, wk.t);
        }
    }
    if constexpr (has_faulted<M>::value) {
        if (m.faulted(wk.s)) return SIM_FAULT;
    }
    if constexpr (Loops::on) {
        u64 f;
        if constexpr (Fp::given) f = fpv.f;
        else f = state_fp<M>(wk.s);
        const u32 t = wk.t;
        u32 j = t && lp.cf == f ? lp.ct : SIM_NO_LOOP;
        // the window, oldest first, so that the largest index wins (no early exit: every read is
        // independent of the others); t = 0 has none, and its fingerprint is the first checkpoint
#pragma unroll
        for (u32 i = SIM_LOOP_WINDOW; i; --i)
            if (i <= t && lp.ring.get((t - i) % SIM_LOOP_WINDOW) == f) j = t - i;
        if (j != SIM_NO_LOOP) {
            lp.start = j;
            for (u32 e = emask & ~wk.sat; e; e &= e - 1) on_hit(__builtin_ctz(e), t);
            return SIM_LOOP;
        }
        lp.ring.put(t % SIM_LOOP_WINDOW, f);
        if ((t & (t - 1)) == 0) {  // t = 0 and the powers of two
            lp.cf = f;
            lp.ct = t;
        }
    }
    if (wk.t >= max_depth) return SIM_DEPTH;
    u64 mask[M::MW];
    m.enabled(wk.s, mask);
    u32 left = 0;
#pragma unroll
    for (int w = 0; w < M::MW; ++w) left += (u32)__builtin_popcountll(mask[w]);
    for (u32 k = 0; left; ++k, --left) {  // (at most the enabled slots: each round clears one)
        const int a = sim_select<M::MW>(mask, sim_choose(sim_rand_keyed(wk.key, wk.t, k), left));
        u64 out[M::W];
        if (m.apply(wk.s, a, out)) {
            on_step(wk.s, a);
#pragma unroll
            for (int j = 0; j < M::W; ++j) wk.s[j] = out[j];
            wk.t += 1;
            return SIM_RUNNING;
        }
#pragma unroll
        for (int w = 0; w < M::MW; ++w)  // (no dynamic index: the mask stays in registers)
            if (w == (a >> 6)) mask[w] &= ~(1ull << (a & 63));
        wk.redraws += 1;
    }
    for (u32 e = emask & ~wk.sat; e; e &= e - 1) on_hit(__builtin_ctz(e), wk.t);
    return SIM_TERMINAL;
}

}  // namespace sr

#include "kernels_sim.hpp"

namespace sr {

// One walk on the host, as the device runs it.
struct SimHostWalk {
    u32 steps = 0, end = SIM_RUNNING, redraws = 0;
    u32 loop_start = SIM_NO_LOOP;  // end == SIM_LOOP: the index of the earlier state the walk returned to
    u64 final_fp = 0;
    std::vector<i64> actions;   // canonical action ids, one per step
    std::vector<i64> states;    // (steps + 1) descriptions (only when asked for)
    std::vector<u64> words;     // (steps + 1) states as the engine holds them, W words each (likewise)
    std::vector<u64> fps;       // (steps + 1) fingerprints (only when asked for)
    std::vector<int> first_hit; // per property: the step of its hit, -1 = none
};

// The whole walk w. describe: also the descriptions and fingerprints of its first keep + 1 states and
// the action ids of its first keep steps (a discovery path is the walk cut at its hit's step).
// loops: with loop detection.
template <class M>
SimHostWalk sim_host_walk(const M& m, u64 seed, u64 w, u32 max_depth, bool loops, bool describe = false, u32 keep = ~0u) {
    const std::vector<u64> inits = init_states_of(m);
    const u32 k = (u32)(inits.size() / M::W);
    if (!k) throw Error(SR_ERR_ARG, "simulation: the model has no init state");
    SimHostWalk r;
    r.first_hit.assign(M::NPROPS, -1);
    SimWalk<M> wk;
    sim_start<M>(wk, seed, w, inits.data(), k);
    const u32 emask = model_emask(m);
    const int wd = m.describe_width();
    auto emit = [&](const u64* s, u32 t) {
        if (!describe || t > keep) return;
        const size_t o = r.states.size();
        r.states.resize(o + wd);
        m.describe(s, &r.states[o]);
        r.words.insert(r.words.end(), s, s + M::W);
        r.fps.push_back(state_fp<M>(s));
    };
    SimLoops<SimRingArray> lp;
    SimNoLoops none;
    for (;;) {
        const u32 t = wk.t;
        auto on_hit = [&](int p, u32 th) { if (r.first_hit[p] < 0) r.first_hit[p] = (int)th; };
        auto on_step = [&](const u64* s, int a) {
            emit(s, t);
            if (t < keep) r.actions.push_back(m.action_id(s, a));
        };
        r.end = loops ? sim_advance(m, wk, max_depth, emask, on_hit, on_step, lp) : sim_advance(m, wk, max_depth, emask, on_hit, on_step, none);
        if (r.end != SIM_RUNNING) break;
    }
    if (r.end == SIM_LOOP) r.loop_start = lp.start;
    emit(wk.s, wk.t);
    r.steps = wk.t;
    r.redraws = wk.redraws;
    r.final_fp = state_fp<M>(wk.s);
    return r;
}

// What the C ABI's simulation accessors ask of a handle (a BFS handle is none).
class SimEngineBase : public EngineBase {
  public:
    virtual bool sim_hit(int p, u64* walk, u32* step) const = 0;
    virtual i64 sim_records(u32* steps, u32* end, u64* fp, i64 cap) const = 0;
    virtual i64 sim_loop_starts(u32* start, i64 cap) const = 0;
    virtual const sr_sim_unique_result& sim_unique() const = 0;
    virtual i64 sim_unique_fps(u64* out, i64 cap) = 0;  // -1: the mode was off
    virtual i64 sim_batch_new(u64* out, i64 cap) const = 0;
};

// U of the walks [w0, w0 + n) on the host ("Distinct-state count" above): sorted, distinct.
template <class M>
std::vector<u64> sim_unique_host(const M& m, u64 seed, u64 w0, u64 n, u32 max_depth, bool loops) {
    std::vector<u64> out;
    auto settle = [&] {
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
    };
    size_t settled = 0;
    for (u64 w = w0; w < w0 + n; ++w) {
        const SimHostWalk h = sim_host_walk(m, seed, w, max_depth, loops, true);
        out.insert(out.end(), h.fps.begin(), h.fps.end());
        if (out.size() > 2 * settled + (1u << 20)) {  // (memory stays within a factor of the set)
            settle();
            settled = out.size();
        }
    }
    settle();
    return out;
}

// SR_SIM_REFILL: 1 = the persistent form (a lane whose walk ended takes the next unstarted index of
// the batch), 0 = one walk per lane. Both give the same per-walk records and hits. The default is
// the static form: profiles/sim_walk_rate.txt.
inline bool sim_refill_default() {
    if (const char* e = std::getenv("SR_SIM_REFILL")) return std::atoi(e) != 0;
    return false;
}

// Steps a launch may take at most (walks of a batch x max_depth): at the ~1.5e10 steps/s of the slowest
// model measured (paxos C=3, profiles/sim_walk_rate.txt) a launch whose walks all run to max_depth
// takes ~9 ms, and a model several times slower stays in the tens of milliseconds. A batch is a whole
// launch followed by a read-back of the counters, so deep walks mean small batches: at the default
// max_depth of 4096 a batch is 32 768 walks, half a wave per SIMD of a 256-CU part, and a check
// whose walks really run that deep is launch-bound at a fraction of the profile's rates (taken at
// max_depth 256, 524 288 walks per batch); walks that end early only make the launch shorter.
// SR_SIM_BATCH (tests) sets the walks per batch directly.
constexpr u64 SIM_STEP_BUDGET = 1ull << 27;
constexpr u64 SIM_BATCH_MAX = 1ull << 24;

template <class M>
class SimEngine final : public SimEngineBase {
    static constexpr int W = M::W;
    static_assert(!is_canon<M>::value && !is_evbits<M>::value, "Canon<M> and EvBits<M> are not simulated");
    static_assert(M::NPROPS <= MAX_PROPS, "too many properties");

  public:
    SimEngine(M m, const sr_sim_opts& o) : m_(m), o_(o), emask_(model_emask(m)), refill_(sim_refill_default()) {
        disc.resize(M::NPROPS);
        hits_.assign(M::NPROPS, SIM_NO_HIT);
        inits_ = init_states_of(m_);
        if (inits_.empty()) throw Error(SR_ERR_ARG, "simulation: the model has no init state");
        batch_ = std::max<u64>(1, std::min<u64>(SIM_BATCH_MAX, SIM_STEP_BUDGET / o_.max_depth));
        if (const char* e = std::getenv("SR_SIM_BATCH"))
            if (std::atoll(e) > 0) batch_ = std::min<u64>((u64)std::atoll(e), SIM_BATCH_MAX);
        if (const char* e = std::getenv("SR_SIM_GRID"))
            if (std::atoi(e) > 0) grid_cap_ = (u32)std::atoi(e);
    }

    int nprops() const override { return M::NPROPS; }
    const char* prop_name(int p) const override { return m_.prop_name(p); }
    int expectation(int p) const override { return m_.expectation(p); }
    int width() const override { return m_.describe_width(); }
    std::string action_name(i64 id) const override { return m_.action_name(id); }
    i64 action_id_bound() const override { return m_.action_id_bound(); }
    int init_count() const override { return (int)(inits_.size() / W); }
    int replay(int init, const i64* ids, int n, std::vector<i64>& states, std::vector<int>& conds, std::vector<int>* all_conds,
               int* terminal) const override {
        return replay_model(m_, init, ids, n, states, conds, all_conds, terminal);
    }
    int explore(const u64* fps, int n, std::vector<i64>& action, std::vector<int>& has, std::vector<u64>& fp,
                std::vector<i64>& states) const override {
        return explore_model(m_, fps, n, action, has, fp, states);
    }
    std::vector<i64> visits() const override { return {}; }

    void run() override {
        const auto t_start = Clock::now();
        SR_HIP(hipSetDevice(o_.device));
        CtxLease lease(o_.device);
        hipStream_t stream = lease.c->stream;
        stats = sr_stats{};
        stats.words_per_state = W;
        const u32 k = (u32)(inits_.size() / W);
        SimArgs a{};
        a.seed = o_.seed;
        a.max_depth = o_.max_depth;
        a.init_count = k;
        a.emask = emask_;
        InlineStates inl{};
        DBuf<u64> init_d;
        if ((u64)k * W <= ROOTS_INLINE_WORDS) {
            std::copy(inits_.begin(), inits_.end(), inl.w);
            stats.root_path = SR_ROOTS_INLINE;
        } else {
            stats.root_path = SR_ROOTS_BUFFER;
            init_d.alloc(o_.device, inits_.size());
            SR_HIP(hipMemcpyAsync(init_d.p, inits_.data(), inits_.size() * sizeof(u64), hipMemcpyHostToDevice, stream));
            a.inits = init_d.p;
        }
        DBuf<u64> dev;  // SimDevice: the counter shards, the best hits, the batch cursor
        dev.alloc(o_.device, (sizeof(SimDevice) + 7) / 8);
        SimDevice* sd = reinterpret_cast<SimDevice*>(dev.p);
        SR_HIP(hipMemsetAsync(sd, 0, sizeof(SimDevice), stream));
        SR_HIP(hipMemsetAsync(sd->best, 0xff, sizeof(sd->best), stream));
        a.dev = sd;
        DBuf<SimRecord> rec;
        const u64 total = o_.walks;  // 0: until every property is discovered or the target is reached
        if (o_.record_walks) rec.alloc(o_.device, (size_t)std::min<u64>(batch_, total ? total : batch_));
        records_.clear();
        int ndev = 0;
        SR_HIP(hipDeviceGetAttribute(&ndev, hipDeviceAttributeMultiprocessorCount, o_.device));
        if (ndev <= 0) ndev = 256;

        // distinct-state table: sized here, cleared once, shared by every batch, released below
        DBuf<u64> uq;
        uq_ = sr_sim_unique_result{};
        uq_.struct_size = sizeof(uq_);
        uq_fps_.clear();
        uq_sorted_ = false;
        batch_new_.clear();
        u64 fresh = 0, stale_run = 0;
        if (o_.unique) {
            uq_.on = 1;
            uq_.capacity = o_.unique_capacity ? o_.unique_capacity
                           : total            ? std::min<u64>(total * ((u64)o_.max_depth + 1), SIM_UNIQUE_MAX_CAPACITY)
                                              : SIM_UNIQUE_MAX_CAPACITY;
            uq_.slots = sim_unique_slots(uq_.capacity);
            uq.alloc(o_.device, (size_t)uq_.slots + SIM_UNIQUE_TAIL);  // the flag and the gather's cursor ride behind the slots
            SR_HIP(hipMemsetAsync(uq.p, 0, ((size_t)uq_.slots + SIM_UNIQUE_TAIL) * sizeof(u64), stream));
            a.uq_keys = uq.p;
            a.uq_flag = reinterpret_cast<u32*>(uq.p + uq_.slots);
            a.uq_log2 = sim_unique_log2(uq_.slots);
            a.uq_limit = sim_unique_probe_limit(uq_.slots);
            stats.table_capacity = uq_.slots;
        }

        u64 states = 0, started = 0, ended[SIM_ENDS] = {};
        u32 longest = 0;
        const auto t_loop = Clock::now();
        std::vector<SimDevice> host(1);
        for (u64 b0 = 0;;) {
            const u64 left = total ? total - b0 : SIM_MAX_WALKS - b0;
            const u32 n = (u32)std::min<u64>(batch_, left);
            if (!n) break;
            a.b0 = b0;
            a.n = n;
            a.records = o_.record_walks ? rec.p : nullptr;
            // the persistent form: at most SIM_PERSIST_WAVES waves per compute unit walk the whole batch
            // (a batch beyond that many lanes is what the refill hands out; SR_SIM_GRID, for tests and
            // measurements, sets the cap in workgroups)
            u32 grid = blocks_for(n, SIM_BLOCK);
            if (refill_) grid = std::min<u32>(grid, grid_cap_ ? grid_cap_ : (u32)ndev * SIM_PERSIST_WAVES / (SIM_BLOCK / 64));
            const size_t ev = 2 * stats.expand_launches;
            if (o_.profile) SR_HIP(hipEventRecord(lease.c->event(ev), stream));
            // (the counting forms are compiled once per LOOPS: the persistent form's code, which with
            // uq_refill = 0 reserves nothing and so is the static form)
            a.uq_refill = refill_;
            if (o_.unique && o_.loops) simulate_walks<M, true, true, true><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            else if (o_.unique) simulate_walks<M, true, false, true><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            else if (o_.loops && refill_) simulate_walks<M, true, true><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            else if (o_.loops) simulate_walks<M, false, true><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            else if (refill_) simulate_walks<M, true, false><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            else simulate_walks<M, false, false><<<grid, SIM_BLOCK, 0, stream>>>(m_, a, inl);
            SR_HIP(hipGetLastError());
            if (o_.profile) SR_HIP(hipEventRecord(lease.c->event(ev + 1), stream));
            stats.expand_launches++;
            launch_frontier.push_back(n);
            launch_probes.push_back(0);
            launch_cas.push_back(0);
            SR_HIP(hipMemcpyAsync(host.data(), sd, sizeof(SimDevice), hipMemcpyDeviceToHost, stream));
            if (o_.record_walks) {
                const size_t o = records_.size();
                records_.resize(o + n);
                SR_HIP(hipMemcpyAsync(&records_[o], rec.p, (size_t)n * sizeof(SimRecord), hipMemcpyDeviceToHost, stream));
            }
            u32 uq_full = 0;
            if (o_.unique) SR_HIP(hipMemcpyAsync(&uq_full, a.uq_flag, sizeof(u32), hipMemcpyDeviceToHost, stream));
            // the next batch starts from zeroed shards and cursor (the best hits carry over)
            SR_HIP(hipMemsetAsync(sd, 0, offsetof(SimDevice, best), stream));
            SR_HIP(stream_sync(stream));
            u64 batch_fresh = 0;
            for (u32 i = 0; i < NSHARD; ++i) {
                const SimShard& s = host[0].shard[i];
                states += s.states;
                batch_fresh += s.fresh;
                for (u32 r = 1; r < SIM_ENDS; ++r) ended[r] += s.ended[r];
                longest = std::max(longest, s.longest);
            }
            started += n;
            b0 += n;
            stats.levels++;
            bool all = true;
            for (int p = 0; p < M::NPROPS; ++p) {
                hits_[p] = host[0].best[p];
                disc[p].found = hits_[p] != SIM_NO_HIT;
                all = all && disc[p].found;
            }
            state_count = states;
            if (o_.unique) {
                fresh += batch_fresh;
                batch_new_.push_back(batch_fresh);
                stale_run = batch_fresh ? 0 : stale_run + 1;
                uq_.unique = fresh;
                uq_.overflow = uq_full != 0;
                uq_.batches = stats.levels;
                unique = fresh;  // |U| (a lower bound after an overflow)
            } else {
                unique = states;  // no visited set: every visited state counts
            }
            max_depth = longest;
            if (o_.verbose)
                std::fprintf(stderr, "[sr] simulation batch %llu: walks %llu, states %llu, longest %u\n",
                             (unsigned long long)stats.levels, (unsigned long long)started, (unsigned long long)states, longest);
            if (ended[SIM_FAULT]) throw Error(SR_ERR_UNSUPPORTED, model_fault_text(m_));
            const u64 done = ended[SIM_TERMINAL] + ended[SIM_DEPTH] + ended[SIM_FAULT] + ended[SIM_LOOP];
            if (done != started)
                throw Error(SR_ERR_HIP, "simulation: a batch ended " + std::to_string(done) + " of " + std::to_string(started) + " walks");
            if (o_.stale_batches && uq_.overflow)
                throw Error(SR_ERR_CAPACITY, "simulation: the distinct-state table of " + std::to_string(uq_.slots) +
                                                 " slots overflowed under stale_batches (a full table takes no new fingerprint and would "
                                                 "look stale forever); raise unique_capacity");
            if (all) {
                reference_done = true;
                break;
            }
            if (o_.target_state_count && states >= o_.target_state_count) break;
            if (o_.stale_batches && stale_run >= o_.stale_batches) {
                uq_.stopped_stale = 1;
                break;
            }
            if (b0 >= SIM_MAX_WALKS) break;
        }
        stats.successors = states - started;
        stats.level_loop_sec = secs(t_loop, Clock::now());
        if (o_.unique && fresh) {  // the set leaves the device compacted; the table is released with this scope
            DBuf<u64> out;
            out.alloc(o_.device, (size_t)fresh);
            unsigned long long* cursor = reinterpret_cast<unsigned long long*>(uq.p + uq_.slots + 1);
            const u32 grid = (u32)std::min<u64>(blocks_for(uq_.slots, SIM_BLOCK), (u64)ndev * 8);
            sim_unique_gather<<<grid, SIM_BLOCK, 0, stream>>>(uq.p, uq_.slots, out.p, fresh, cursor);
            SR_HIP(hipGetLastError());
            uq_fps_.resize((size_t)fresh);
            u64 gathered = 0;
            SR_HIP(hipMemcpyAsync(uq_fps_.data(), out.p, (size_t)fresh * sizeof(u64), hipMemcpyDeviceToHost, stream));
            SR_HIP(hipMemcpyAsync(&gathered, cursor, sizeof(u64), hipMemcpyDeviceToHost, stream));
            SR_HIP(stream_sync(stream));
            if (gathered != fresh)
                throw Error(SR_ERR_HIP, "simulation: the distinct-state table holds " + std::to_string(gathered) + " fingerprints, but " +
                                            std::to_string(fresh) + " were counted");
        }
        if (o_.profile && stats.expand_launches) {
            double ms = 0;
            launch_ms.assign(stats.expand_launches, 0.0);
            for (u64 i = 0; i < stats.expand_launches; ++i) {
                float t = 0;
                SR_HIP(hipEventElapsedTime(&t, lease.c->event(2 * i), lease.c->event(2 * i + 1)));
                ms += t;
                launch_ms[i] = t;
            }
            stats.expand_kernel_ms = ms;
        }
        stats.total_sec = secs(t_start, Clock::now());
    }

    // The discovery of property p: walk w of its hit (t, w), cut at step t, re-walked on the host. With
    // loop detection the hit of an `eventually` property may be a lasso (the walk ended with SIM_LOOP
    // at t): the walk was ended on equal FINGERPRINTS, so the path is returned only after its last
    // state and the state at loop_start were compared word for word.
    SimHostWalk discovery_walk(int p) const {
        const u64 key = hits_[p];
        const u32 t = (u32)(key >> 40);
        const u64 w = key & (SIM_MAX_WALKS - 1);
        SimHostWalk r = sim_host_walk(m_, o_.seed, w, o_.max_depth, o_.loops != 0, true, t);
        if (r.steps < t || r.first_hit[p] != (int)t)
            throw Error(SR_ERR_NONDETERMINISM, "simulation: the host walk " + std::to_string(w) + " does not reproduce the device's hit of \"" +
                                                   std::string(m_.prop_name(p)) + "\" at step " + std::to_string(t));
        if ((emask_ >> p & 1) && r.end == SIM_LOOP && r.steps == t) {
            const u32 j = r.loop_start;
            if (j >= t || r.words.size() != (size_t)(t + 1) * W ||
                !std::equal(r.words.begin() + (size_t)j * W, r.words.begin() + (size_t)(j + 1) * W, r.words.begin() + (size_t)t * W))
                throw Error(SR_ERR_NONDETERMINISM, "simulation: fingerprint collision: walk " + std::to_string(w) + " ended as a loop at step " +
                                                       std::to_string(t) + ", but its state there differs from the state at step " +
                                                       std::to_string(j) + "; no lasso is reported for \"" + std::string(m_.prop_name(p)) + "\"");
        }
        return r;
    }
    int chain(int p, std::vector<u64>& out) override {
        out.clear();
        if (p < 0 || p >= M::NPROPS || hits_[p] == SIM_NO_HIT) return 0;
        out = discovery_walk(p).fps;
        return (int)out.size();
    }
    int path(int p, std::vector<i64>& actions, std::vector<i64>& states) override {
        if (p < 0 || p >= M::NPROPS || hits_[p] == SIM_NO_HIT) return -1;
        SimHostWalk r = discovery_walk(p);
        actions = std::move(r.actions);
        states = std::move(r.states);
        return (int)actions.size();
    }

    bool sim_hit(int p, u64* walk, u32* step) const override {
        if (p < 0 || p >= M::NPROPS || hits_[p] == SIM_NO_HIT) return false;
        if (walk) *walk = hits_[p] & (SIM_MAX_WALKS - 1);
        if (step) *step = (u32)(hits_[p] >> 40);
        return true;
    }
    i64 sim_records(u32* steps, u32* end, u64* fp, i64 cap) const override {
        for (i64 i = 0; i < std::min<i64>(cap, (i64)records_.size()); ++i) {
            if (steps) steps[i] = records_[i].steps;
            if (end) end[i] = records_[i].end & 0xff;
            if (fp) fp[i] = records_[i].fp;
        }
        return (i64)records_.size();
    }
    i64 sim_loop_starts(u32* start, i64 cap) const override {
        for (i64 i = 0; start && i < std::min<i64>(cap, (i64)records_.size()); ++i)
            start[i] = (records_[i].end & 0xff) == SIM_LOOP ? records_[i].end >> 8 : SIM_NO_LOOP;
        return (i64)records_.size();
    }
    const sr_sim_unique_result& sim_unique() const override { return uq_; }
    i64 sim_unique_fps(u64* out, i64 cap) override {
        if (!uq_.on) return -1;
        if (!uq_sorted_) {  // once, on demand
            std::sort(uq_fps_.begin(), uq_fps_.end());
            uq_sorted_ = true;
        }
        for (i64 i = 0; out && i < std::min<i64>(cap, (i64)uq_fps_.size()); ++i) out[i] = uq_fps_[i];
        return (i64)uq_fps_.size();
    }
    i64 sim_batch_new(u64* out, i64 cap) const override {
        for (i64 i = 0; out && i < std::min<i64>(cap, (i64)batch_new_.size()); ++i) out[i] = batch_new_[i];
        return (i64)batch_new_.size();
    }

  private:
    M m_;
    sr_sim_opts o_;
    u32 emask_;
    bool refill_;
    u32 grid_cap_ = 0;  // SR_SIM_GRID: the persistent form's grid cap in workgroups (0: by compute units)
    u64 batch_ = 1;
    std::vector<u64> inits_;
    std::vector<u64> hits_;          // per property: sim_hit_key of the best hit, SIM_NO_HIT = none
    std::vector<SimRecord> records_; // record_walks: one per walk started, by walk index
    sr_sim_unique_result uq_{};      // distinct-state count: what sr_gpu_sim_unique reports
    std::vector<u64> uq_fps_;        //   U as gathered from the table (sorted at the first request)
    bool uq_sorted_ = false;
    std::vector<u64> batch_new_;     //   per batch: the fingerprints it added
};

// Validated copy of a caller's sr_sim_opts (a shorter mirror is zero-extended, then defaulted).
inline sr_sim_opts normalized_sim_opts(const sr_sim_opts* opts) {
    sr_sim_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) std::memcpy(&o, opts, std::min<size_t>(sizeof(o), opts->struct_size ? opts->struct_size : sizeof(o)));
    o.struct_size = sizeof(sr_sim_opts);
    if (!o.max_depth) o.max_depth = 4096;
    if (o.max_depth > SIM_MAX_DEPTH) throw Error(SR_ERR_ARG, "simulation: max_depth must be in 1..=2^20");
    if (o.walks >= SIM_MAX_WALKS) throw Error(SR_ERR_ARG, "simulation: walks must be below 2^40");
    o.reserved0 = 0;  // (a 56-byte caller's tail padding: never read)
    if (o.stale_batches && !o.unique)
        throw Error(SR_ERR_ARG, "simulation: stale_batches needs unique = 1 (it counts batches without a new distinct state)");
    if (o.unique_capacity > SIM_UNIQUE_MAX_REQUEST) throw Error(SR_ERR_ARG, "simulation: unique_capacity must be at most 2^30");
    if (!o.walks && !o.target_state_count && !o.stale_batches)
        throw Error(SR_ERR_ARG, "simulation: walks or target_state_count must be set (a property may never be discovered)");
    return o;
}

}  // namespace sr
