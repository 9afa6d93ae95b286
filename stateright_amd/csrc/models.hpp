// GpuModel encodings: the device-side counterpart of `impl Model for X` (src/lib.rs:155-237).
//
// A GpuModel packs one state into W 64-bit words (equal states <=> equal words) and exposes the
// reference's `actions()` list as ACTION SLOTS 0..max_actions-1 in the reference's own order:
//   enabled(s, mask)   bit a of mask = slot a appears in `actions(s)`
//   apply(s, a, out)   `next_state(s, action)` is Some AND `within_boundary` holds -> out
//   discovers(p, s)    property p yields a discovery at s (always: !cond, sometimes: cond)
// Host-only helpers give init states, property names/expectations, the canonical description of a
// state (shared with the CPU oracle for set/order/path comparison) and canonical action ids.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace sr {

using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;

#define SR_HD __host__ __device__ __forceinline__

enum Expect { ALWAYS = 0, EVENTUALLY = 1, SOMETIMES = 2, LEADS_TO = 3, ALWAYS_STEP = 4 };

// Mask of a model's `eventually` properties (0 for models without an `emask()` member).
template <class M, class = void>
struct has_emask : std::false_type {};
template <class M>
struct has_emask<M, std::void_t<decltype(std::declval<const M&>().emask())>> : std::true_type {};
template <class M>
inline u32 model_emask(const M& m) {
    if constexpr (has_emask<M>::value) return m.emask();
    else return 0;
}

// Mask of a model's leads-to properties (0 for models without an `lmask()` member). Such a property p
// (`expectation(p) == LEADS_TO`) has `discovers(p, s)` as its TARGET condition Q, the role it has for
// `eventually`, and `leads_from(p, s)` as its TRIGGER P: "whenever P, eventually Q" (live.hpp, LEADS-TO).
// The search never evaluates it: its bit is in no `undiscovered` mask handed to a kernel and not in
// emask(); only the complete liveness check decides it.
template <class M, class = void>
struct has_lmask : std::false_type {};
template <class M>
struct has_lmask<M, std::void_t<decltype(std::declval<const M&>().lmask())>> : std::true_type {};
template <class M>
inline u32 model_lmask(const M& m) {
    if constexpr (has_lmask<M>::value) return m.lmask();
    else return 0;
}

// Mask of a model's STEP properties (0 for models without an `smask()` member). Such a property p
// (`expectation(p) == ALWAYS_STEP`) is an invariant over steps, TLA+'s [][A]_v: `step_holds(p, s, a, t)` says
// whether the step from s through slot a to t is allowed. `discovers(p, .)` is false everywhere, and its bit is
// in no `undiscovered` mask handed to a kernel of the search: only the step pass decides it (step.hpp).
template <class M, class = void>
struct has_smask : std::false_type {};
template <class M>
struct has_smask<M, std::void_t<decltype(std::declval<const M&>().smask())>> : std::true_type {};
template <class M>
inline u32 model_smask(const M& m) {
    if constexpr (has_smask<M>::value) return m.smask();
    else return 0;
}

// Models whose states pack into a key (`qkey_bits()` and `qkey(s)`: an injective packing of the
// state into an integer below 2^qkey_bits) use the exact quotient visited set (kernels.hpp
// TableView) when the key has at most 62 bits on one word or 96 on more (kernels.hpp
// quotient_model), and a fingerprint otherwise.
template <class M, class = void>
struct has_qkey : std::false_type {};
template <class M>
struct has_qkey<M, std::void_t<decltype(std::declval<const M&>().qkey_bits())>> : std::true_type {};

// Models that can rebuild a state from its canonical description (`undescribe`, the inverse of
// `describe`) expose their fingerprint to a host that holds the state (sr_model_fingerprint).
template <class M, class = void>
struct has_undescribe : std::false_type {};
template <class M>
struct has_undescribe<M, std::void_t<decltype(std::declval<const M&>().undescribe((const i64*)nullptr, (u64*)nullptr))>>
    : std::true_type {};

// Models with a canonical representative under their symmetry (`canonical(s, out)`).
template <class M, class = void>
struct has_canonical : std::false_type {};
template <class M>
struct has_canonical<M, std::void_t<decltype(std::declval<const M&>().canonical((const u64*)nullptr, (u64*)nullptr))>>
    : std::true_type {};

// Models that know which enabled actions return the state itself (`self_loops(s, enabled, out)`:
// out = the subset of `enabled` whose next_state is s). The FAST expansion counts those successors
// (they are state_count increments, bfs.rs:235, and never new) without generating them: on 2pc
// they are 37% of all successors. Exactness is tested against apply() over every reachable state
// (tests/test_gpu_parity.py, the oracle's state counts).
template <class M, class = void>
struct has_self_loops : std::false_type {};
template <class M>
struct has_self_loops<M, std::void_t<decltype(std::declval<const M&>().self_loops((const u64*)nullptr, (const u64*)nullptr,
                                                                                  (u64*)nullptr))>> : std::true_type {};

// One-word models (W == 1) whose actions write fields that depend on the slot alone
// (`action_masks(slot, &clr, &set)`): for every state s and every slot enabled in s, `apply(s, slot)`
// returns true with o[0] == (s[0] & ~clr) | set. The FAST expansion then keeps one (clr, set) pair
// per lane, slot = lane, and a successor lane fetches its slot's pair from that lane instead of
// running `apply` (kernels.hpp ActionTable). The hook is called for every slot below 64 MW, enabled
// anywhere or not, so it must be total there (its result for a slot that is never enabled is unused).
template <class M, class = void>
struct has_action_masks : std::false_type {};
template <class M>
struct has_action_masks<M, std::void_t<decltype(std::declval<const M&>().action_masks(0, (u64*)nullptr, (u64*)nullptr))>>
    : std::true_type {};

// Models that compute their enabled mask without their self-loops in one pass
// (`enabled_moves(s, mk)`: mk = enabled(s) & ~self_loops(s), returns the number of self-loops
// removed). The FAST expansion calls it in place of the `enabled` + `self_loops` pair.
template <class M, class = void>
struct has_enabled_moves : std::false_type {};
template <class M>
struct has_enabled_moves<M, std::void_t<decltype(std::declval<const M&>().enabled_moves((const u64*)nullptr, (u64*)nullptr))>>
    : std::true_type {};

// Models whose self-loop hook is exact (`static constexpr bool SELF_LOOPS_EXACT = true`): every
// slot that `enabled_moves` (or `enabled & ~self_loops`) leaves changes the state, so the FAST
// expansion does not compare a successor with its parent again.
template <class M, class = void>
struct self_loops_exact : std::false_type {};
template <class M>
struct self_loops_exact<M, std::void_t<decltype(M::SELF_LOOPS_EXACT)>> : std::integral_constant<bool, M::SELF_LOOPS_EXACT> {};

// Wide models whose enabled mask is a per-slot test (`enabled_slot(s, k)` = bit k of `enabled(s)`,
// `ESLOTS` = max_actions, a power of two <= 64, MW = 1). Small levels of such a model are chains of
// dependent instructions on a few lanes; the FAST expansion then evaluates the mask with one lane
// per (parent, slot) instead of one lane per parent walking all the slots (paxos: 16 slots, each a
// switch over the destination server's word), reading the parent from the wave's LDS copy.
template <class M, class = void>
struct has_enabled_slot : std::false_type {};
template <class M>
struct has_enabled_slot<M, std::void_t<decltype(std::declval<const M&>().enabled_slot((const u64*)nullptr, 0)),
                                       decltype(M::ESLOTS)>> : std::true_type {};

// Models with an OWNER KEY (`owner_key(s, &key)`: a projection of the state that most actions
// leave unchanged; returns false when this instance has none). The partitioned search then owns a
// state by its key instead of its fingerprint, so most successors stay in their parent's
// partition and are inserted there instead of crossing to another GPU. Any
// deterministic function of the state keeps the search exact (every state has exactly one
// owner); the projection only sets the share of successors that cross and the load balance.
template <class M, class = void>
struct has_owner_key : std::false_type {};
template <class M>
struct has_owner_key<M, std::void_t<decltype(std::declval<const M&>().owner_key((const u64*)nullptr, (u64*)nullptr))>>
    : std::true_type {};

// Models whose encoding can be exceeded by a reachable state (`faulted(s)`: the state s lost
// information when it was built, e.g. an actor network past its slots). Every kernel that evaluates
// a new state's properties asks the hook and ORs ERR_MODEL into the level's err word (kernels.hpp
// eval_props); the engines end the check with SR_ERR_UNSUPPORTED (`model_fault`), with no capacity
// restart. `model_name()` (optional, host) names the model in that error.
template <class M, class = void>
struct has_faulted : std::false_type {};
template <class M>
struct has_faulted<M, std::void_t<decltype(std::declval<const M&>().faulted((const u64*)nullptr))>> : std::true_type {};
template <class M, class = void>
struct has_model_name : std::false_type {};
template <class M>
struct has_model_name<M, std::void_t<decltype(std::declval<const M&>().model_name())>> : std::true_type {};
template <class M>
inline std::string model_fault_text(const M& m) {
    std::string name = "model";
    if constexpr (has_model_name<M>::value) name = m.model_name();
    return name + ": a state exceeded its encoding (network slots)";
}

// Init states (`Model::init_states`, src/lib.rs:163). A model writes its init states into a host
// buffer of W words each; the engine sizes that buffer from the model's optional `init_count()`,
// or for MAX_INIT_STATES states when the model has none (the documented bound of the GpuModel
// concept, include/stateright_gpu_model.hpp). Every host-side caller goes through init_states_of.
constexpr int MAX_INIT_STATES = 256;
template <class M, class = void>
struct has_init_count : std::false_type {};
template <class M>
struct has_init_count<M, std::void_t<decltype(std::declval<const M&>().init_count())>> : std::true_type {};
template <class M>
inline int init_capacity(const M& m) {
    if constexpr (has_init_count<M>::value) return m.init_count() > 0 ? m.init_count() : 1;
    else return MAX_INIT_STATES;
}

// The symmetry-reduced view of a model (the engine's opt-in canonical reduction): init states and
// successors are replaced by their canonical representatives, so the visited set, the frontier and
// the BFS tree hold one state per orbit. Everything else is the model's own.
template <class M>
struct Canon : M {
    Canon() = default;
    explicit Canon(const M& m) : M(m) {}
    const M& base() const { return *this; }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        u64 t[M::W];
        if (!M::apply(s, a, t)) return false;
        M::canonical(t, o);
        return true;
    }
    int init_states(u64* out) const {
        const int k = M::init_states(out);
        for (int i = 0; i < k; ++i) {
            u64 t[M::W];
            M::canonical(out + i * M::W, t);
            for (int w = 0; w < M::W; ++w) out[i * M::W + w] = t[w];
        }
        return k;
    }
};
template <class M>
struct is_canon : std::false_type {};
template <class M>
struct is_canon<Canon<M>> : std::true_type {};

// murmur3 fmix64: a bijection on u64 with fmix64(0) == 0.
SR_HD u64 fmix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// 64-bit state fingerprint (`fingerprint`, src/lib.rs:306-311). For W == 1 the packed state
// uses at most 63 bits, so XOR-ing bit 63 and mixing is a BIJECTION that is never zero: the
// visited set is then exact (no fingerprint collisions at all). For W > 1 it is a 64-bit hash
// like the reference's (collisions possible at ~n^2/2^65); zero is remapped to 1 where the
// reference would panic (src/lib.rs:310).
template <int W>
SR_HD u64 fingerprint(const u64* s) {
    if constexpr (W == 1) {
        return fmix64(s[0] ^ 0x8000000000000000ull);
    } else {
        // every word mixed on its own (position-keyed), then one mix of their sum: two mixes deep
        // instead of a chain of W (a lone wave of a small paxos level waits on that chain: C=3
        // 0.62 -> 0.61 ms, profiles/r05_paxos_lin.txt; round 4 had measured no gain, before the
        // linearizability test's chain was cut)
        u64 acc = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) acc += fmix64(s[i] ^ (0x632BE59BD9B4E019ull * (u64)(i + 1)));
        const u64 h = fmix64(acc ^ 0x9E3779B97F4A7C15ull);
        return h ? h : 1;
    }
}

// Words of a state that its fingerprint covers: M::FPW when the model declares it (EvBits<M>: the
// last word is bookkeeping that rides with the state but is not part of it), else all W. Every
// fingerprint the engines compute (visited set, partition owner, discovery chains) goes through
// state_fp, so an EvBits<M> state has the fingerprint of the M state it wraps.
template <class M, class = void>
struct fp_words_of : std::integral_constant<int, M::W> {};
template <class M>
struct fp_words_of<M, std::void_t<decltype(M::FPW)>> : std::integral_constant<int, M::FPW> {};
template <class M>
SR_HD u64 state_fp(const u64* s) {
    return fingerprint<fp_words_of<M>::value>(s);
}

// `eventually` properties for the PARTITIONED search (src/checker/bfs.rs:52-60,212-222,265-272):
// the EventuallyBits of a pending state ride in one extra word of it, so the records the ranks
// exchange carry them and the owner's claim keeps the claiming generator's bits (the FAST order's
// rule of the one-GPU engine, kernels.hpp expand_fast naeb). A successor gets its parent's bits
// minus the eventually properties whose condition holds at the parent (the parent's pop), and an
// eventually property is discovered at a state that still carries its bit, where its condition
// does not hold and that has no successor within boundary (a terminal state, bfs.rs:265-272).
// The engine sees no `eventually` property (emask() == 0): such a discovery is an ordinary
// discovery of the new state, with its path.  The visited set and every fingerprint cover the
// wrapped state only (FPW), so a state reached with two different bit words is ONE state, as in
// the reference (bfs.rs:235-246: the first generator's bits win).
template <class M>
struct EvBits : M {
    static constexpr int W = M::W + 1, FPW = M::W;
    u32 ev_props_ = 0;  // the wrapped model's eventually properties
    EvBits() = default;
    explicit EvBits(const M& m) : M(m), ev_props_(model_emask(m)) {}
    const M& base() const { return *this; }
    u32 emask() const { return 0; }
    SR_HD u32 holds(const u64* s) const {
        u32 h = 0;
        for (u32 e = ev_props_; e; e &= e - 1)
            if (M::discovers(__builtin_ctz(e), s)) h |= 1u << __builtin_ctz(e);
        return h;
    }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        if (!M::apply(s, a, o)) return false;
        o[M::W] = s[M::W] & ~(u64)holds(s);
        return true;
    }
    SR_HD bool discovers(int p, const u64* s) const {
        if (!(ev_props_ >> p & 1)) return M::discovers(p, s);
        if (!(s[M::W] >> p & 1) || M::discovers(p, s)) return false;
        u64 mask[M::MW];
        M::enabled(s, mask);
        for (int w = 0; w < M::MW; ++w)
            for (u64 bits = mask[w]; bits; bits &= bits - 1) {
                u64 t[M::W];
                if (M::apply(s, w * 64 + __builtin_ctzll(bits), t)) return false;
            }
        return true;
    }
    int init_states(u64* out) const {
        const int k = M::init_states(out);
        for (int i = k - 1; i >= 0; --i) {
            for (int w = M::W - 1; w >= 0; --w) out[i * W + w] = out[i * M::W + w];
            out[i * W + M::W] = ev_props_;
        }
        return k;
    }
};
template <class M>
struct is_evbits : std::false_type {};
template <class M>
struct is_evbits<EvBits<M>> : std::true_type {};

// Canon<M> and EvBits<M> inherit their model's hooks but replace its `apply` (the canonical
// representative, the extra word), so what `action_masks` and SELF_LOOPS_EXACT say about the
// model's own successors does not hold for theirs: those two are taken from unwrapped models only.
template <class M>
constexpr bool action_table_model = M::W == 1 && has_action_masks<M>::value && !is_canon<M>::value && !is_evbits<M>::value;
template <class M>
constexpr bool exact_moves_model = self_loops_exact<M>::value && !is_canon<M>::value && !is_evbits<M>::value;

SR_HD u64 getb(const u64* s, int off, int width) {
    // bit field [off, off+width) of a little-endian multi-word state; width <= 8, no word crossing
    return (s[off >> 6] >> (off & 63)) & ((1ull << width) - 1);
}
SR_HD void setb(u64* s, int off, int width, u64 v) {
    u64 m = ((1ull << width) - 1) << (off & 63);
    s[off >> 6] = (s[off >> 6] & ~m) | ((v << (off & 63)) & m);
}

// -----------------------------------------------------------------------------------------------
// LinearEquation (src/test_util.rs:140-188): state (x: u8, y: u8); actions IncreaseX, IncreaseY.
// -----------------------------------------------------------------------------------------------
struct LinearEquation {
    static constexpr int W = 1, MW = 1, NPROPS = 1;
    u32 a, b, c;
    int max_actions() const { return 2; }
    int max_out_degree() const { return 2; }
    SR_HD void enabled(const u64*, u64* m) const { m[0] = 3; }
    SR_HD bool apply(const u64* s, int a_, u64* o) const {
        u64 x = s[0] & 0xff, y = (s[0] >> 8) & 0xff;
        if (a_ == 0) x = (x + 1) & 0xff; else y = (y + 1) & 0xff;
        o[0] = x | (y << 8);
        return true;
    }
    SR_HD bool discovers(int, const u64* s) const {  // sometimes "solvable": a*x + b*y == c (u8)
        u64 x = s[0] & 0xff, y = (s[0] >> 8) & 0xff;
        return ((a * x + b * y) & 0xff) == c;
    }
    int init_states(u64* out) const { out[0] = 0; return 1; }
    int expectation(int) const { return SOMETIMES; }
    const char* prop_name(int) const { return "solvable"; }
    int describe_width() const { return 2; }
    void describe(const u64* s, i64* d) const { d[0] = (i64)(s[0] & 0xff); d[1] = (i64)((s[0] >> 8) & 0xff); }
    void undescribe(const i64* d, u64* s) const { s[0] = ((u64)d[0] & 0xff) | ((u64)d[1] & 0xff) << 8; }
    i64 action_id(const u64*, int a_) const { return a_; }
    std::string action_name(i64 id) const { return id == 0 ? "IncreaseX" : "IncreaseY"; }
    i64 action_id_bound() const { return 2; }
};

// -----------------------------------------------------------------------------------------------
// BinaryClock (src/test_util.rs:4-45): i8 state in {0, 1}; one action (GoHigh at 0, GoLow at 1).
// -----------------------------------------------------------------------------------------------
struct BinaryClock {
    static constexpr int W = 1, MW = 1, NPROPS = 1;
    int max_actions() const { return 1; }
    int max_out_degree() const { return 1; }
    SR_HD void enabled(const u64*, u64* m) const { m[0] = 1; }
    SR_HD bool apply(const u64* s, int, u64* o) const { o[0] = (s[0] & 0xff) == 0 ? 1 : 0; return true; }
    SR_HD bool discovers(int, const u64* s) const {  // always "in [0, 1]"
        int8_t v = (int8_t)(s[0] & 0xff);
        return !(0 <= v && v <= 1);
    }
    int init_states(u64* out) const { out[0] = 0; out[1] = 1; return 2; }
    int expectation(int) const { return ALWAYS; }
    const char* prop_name(int) const { return "in [0, 1]"; }
    int describe_width() const { return 1; }
    void describe(const u64* s, i64* d) const { d[0] = (int8_t)(s[0] & 0xff); }
    void undescribe(const i64* d, u64* s) const { s[0] = (u64)(u8)d[0]; }
    i64 action_id(const u64* s, int) const { return (s[0] & 0xff) == 0 ? 1 : 0; }  // GoLow=0, GoHigh=1
    std::string action_name(i64 id) const { return id == 0 ? "GoLow" : "GoHigh"; }
    i64 action_id_bound() const { return 2; }
};

// -----------------------------------------------------------------------------------------------
// Two-phase commit (examples/2pc.rs:10-121), n <= 14 resource managers, 4n+4 bits:
//   [0,2n)      rm_state[rm]   (Working 0, Prepared 1, Committed 2, Aborted 3)
//   [2n,2n+2)   tm_state       (Init 0, Committed 1, Aborted 2)
//   [2n+2,3n+2) tm_prepared[rm]
//   [3n+2,4n+2) msgs ∋ Prepared{rm}
//   4n+2        msgs ∋ Commit;  4n+3  msgs ∋ Abort
// Slots follow `actions()` (examples/2pc.rs:56-81): 0 TmCommit, 1 TmAbort, then for each rm
// 2+5rm+{0 TmRcvPrepared, 1 RmPrepare, 2 RmChooseToAbort, 3 RmRcvCommitMsg, 4 RmRcvAbortMsg}.
// Every action returns Some (examples/2pc.rs:83-104), self-loops included.
// -----------------------------------------------------------------------------------------------
// NC > 0: the rm count as a compile-time constant (the engine's specialization of the bench
// configurations, reg_two_phase.hip); the device functions read it through N(), so their per-rm
// loops unroll with constant shifts. NC = 0 reads the runtime n.
template <int NC = 0>
struct TwoPhaseT {
    static constexpr int W = 1, MW = 2, NPROPS = 3;
    int n;
    SR_HD int N() const {
        if constexpr (NC > 0) return NC;
        else return n;
    }
    // Owner key of the partitioned search: the per-RM tuples (rm_state, tm_prepared,
    // Prepared{rm} in msgs) of the first okey_rms resource managers (0: no key, own by
    // fingerprint). Only the five actions of those RMs change it; TmCommit/TmAbort and the other
    // RMs' actions keep a successor in its parent's partition.
    int okey_rms = 0;
    SR_HD bool owner_key(const u64* sp, u64* key) const {
        const int n = N();
        const int k = okey_rms;
        const u64 s = sp[0], m = (1ull << k) - 1;
        *key = (s & ((1ull << (2 * k)) - 1)) | ((s >> (2 * n + 2)) & m) << (2 * k) | ((s >> (3 * n + 2)) & m) << (3 * k);
        return k > 0;
    }
    int max_actions() const { return 2 + 5 * n; }
    // Per rm at most three of its five slots (a Working rm after TmAbort: Prepare, ChooseToAbort,
    // RcvAbort); TmCommit/TmAbort only while the TM is Init (then at most two per rm).
    int max_out_degree() const { return 2 + 3 * n; }
    SR_HD u64 rmask() const { return (1ull << N()) - 1; }
    // per-rm bit vectors
    SR_HD u64 working(u64 s) const {  // rm_state == 0, one bit per rm
        const int n = N();
        const u64 ev = 0x5555555555555555ull & ((1ull << (2 * n)) - 1);
        u64 w = ~(s | (s >> 1)) & ev;  // bit 2rm: field rm == 0
        // compress the even bits to bits 0..n-1
        w = (w | (w >> 1)) & 0x3333333333333333ull;
        w = (w | (w >> 2)) & 0x0f0f0f0f0f0f0f0full;
        w = (w | (w >> 4)) & 0x00ff00ff00ff00ffull;
        w = (w | (w >> 8)) & 0x0000ffff0000ffffull;
        w = (w | (w >> 16)) & 0x00000000ffffffffull;
        return w;
    }
    // One 5-bit group per rm at slot 2 + 5rm (TmRcvPrepared, RmPrepare, RmChooseToAbort,
    // RmRcvCommitMsg, RmRcvAbortMsg), placed without per-action branches.
    SR_HD void enabled(const u64* sp, u64* m) const {
        const int n = N();
        const u64 s = sp[0];
        const u64 tm = (s >> (2 * n)) & 3;
        const u64 prepared = (s >> (2 * n + 2)) & rmask();
        const u64 msgp = (s >> (3 * n + 2)) & rmask();
        const u64 commit = (s >> (4 * n + 2)) & 1, abort = (s >> (4 * n + 3)) & 1;
        const u64 work = working(s);
        const u64 rcv = tm == 0 ? msgp : 0;
        const u64 tail = commit << 3 | abort << 4;
        u64 lo = (u64)(tm == 0 && prepared == rmask()) | (u64)(tm == 0) << 1, hi = 0;
        for (int rm = 0; rm < n; ++rm) {
            const int b = 2 + 5 * rm;
            const u64 bits = ((rcv >> rm) & 1) | ((work >> rm) & 1) * 6ull | tail;
            if (b < 64) lo |= bits << b;
            if (b + 4 >= 64) hi |= b >= 64 ? bits << (b - 64) : bits >> (64 - b);
        }
        m[0] = lo;
        m[1] = hi;
    }
    // The enabled actions that return s itself: TmRcvPrepared(rm) with tm_prepared[rm] already set,
    // RmRcvCommitMsg(rm) with rm already Committed, RmRcvAbortMsg(rm) with rm already Aborted. No
    // other action can (RmPrepare and RmChooseToAbort need a Working rm and change it, TmCommit and
    // TmAbort need tm_state Init and change it).
    SR_HD void self_loops(const u64* sp, const u64* mk, u64* sl) const {
        const int n = N();
        const u64 s = sp[0];
        const u64 tm = (s >> (2 * n)) & 3;
        const u64 prepared = (s >> (2 * n + 2)) & rmask();
        const u64 msgp = (s >> (3 * n + 2)) & rmask();
        const bool commit = (s >> (4 * n + 2)) & 1, abort = (s >> (4 * n + 3)) & 1;
        u64 lo = 0, hi = 0;
        for (int rm = 0; rm < n; ++rm) {
            const u64 r = (s >> (2 * rm)) & 3;
            const int b = 2 + 5 * rm;
            const u64 bits = (u64)(tm == 0 && ((msgp & prepared) >> rm & 1)) | (u64)(commit && r == 2) << 3 |
                             (u64)(abort && r == 3) << 4;
            if (b < 64) lo |= bits << b;
            if (b + 4 >= 64) hi |= b >= 64 ? bits << (b - 64) : bits >> (64 - b);
        }
        sl[0] = lo & mk[0];
        sl[1] = hi & mk[1];
    }
    // Branch-free: the lanes of a wave apply different actions, and a switch over them ran every
    // taken arm for the whole wave. Every action writes at most one 2-bit field (rm_state[rm] or
    // tm_state) and sets at most one bit:
    //   a = 0 TmCommit         tm_state <- 1, bit 4n+2 (Commit)
    //   a = 1 TmAbort          tm_state <- 2, bit 4n+3 (Abort)
    //   k = 0 TmRcvPrepared    bit 2n+2+rm (tm_prepared)
    //   k = 1 RmPrepare        rm_state <- 1, bit 3n+2+rm (Prepared{rm})
    //   k = 2 RmChooseToAbort  rm_state <- 3
    //   k = 3 RmRcvCommitMsg   rm_state <- 2
    //   k = 4 RmRcvAbortMsg    rm_state <- 3
    SR_HD bool apply(const u64* sp, int a, u64* o) const {
        const int n = N();
        const u64 s = sp[0];
        const bool tm = a < 2;
        const u32 b = tm ? 0u : (u32)(a - 2), rm = b / 5, k = b - 5 * rm;
        const u32 fpos = tm ? 2u * n : 2u * rm;
        const u64 fval = tm ? (u64)(a + 1) : k == 1 ? 1ull : k == 3 ? 2ull : 3ull;
        const u64 fmask = (tm || k != 0) ? 3ull << fpos : 0ull;
        const u32 epos = tm ? 4u * n + 2 + (u32)a : (k == 0 ? 2u * n + 2 : 3u * n + 2) + rm;
        const u64 ebit = (tm || k <= 1) ? 1ull << epos : 0ull;
        o[0] = ((s & ~fmask) | ((fval << fpos) & fmask)) | ebit;
        return true;
    }
    // The same table as masks of the slot alone (has_action_masks): apply(s, a) = (s & ~clr) | set.
    // Total over the slots past max_actions (their shifts wrap; nothing enables them).
    SR_HD void action_masks(int a, u64* clr, u64* set) const {
        const int n = N();
        const bool tm = a < 2;
        const u32 b = tm ? 0u : (u32)(a - 2), rm = b / 5, k = b - 5 * rm;
        const u32 fpos = (tm ? 2u * n : 2u * rm) & 63;
        const u64 fval = tm ? (u64)(a + 1) : k == 1 ? 1ull : k == 3 ? 2ull : 3ull;
        const u64 fmask = (tm || k != 0) ? 3ull << fpos : 0ull;
        const u32 epos = (tm ? 4u * n + 2 + (u32)a : (k == 0 ? 2u * n + 2 : 3u * n + 2) + rm) & 63;
        const u64 ebit = (tm || k <= 1) ? 1ull << epos : 0ull;
        *clr = fmask;
        *set = ((fval << fpos) & fmask) | ebit;
    }
    // No slot that enabled_moves (or enabled & ~self_loops) leaves returns the state itself: see
    // self_loops above (sr_selftest_action_masks checks it over reachable and random states).
    static constexpr bool SELF_LOOPS_EXACT = true;
    // A slot is an action of the protocol (TmCommit, RmPrepare(rm), ..): a fairness class (live.hpp, weak fairness).
    static constexpr bool FAIR_SLOTS = true;
    // Six fields of a word to stride 5 (field i to bit 5i), three shift-and-mask steps like
    // working()'s compression: 2-bit fields at stride 2 (bits 0..11), 1-bit fields at stride 1.
    SR_HD static u32 spread2to5(u32 x) {
        x = (x | x << 12) & 0x00F000FFu;
        x = (x | x << 6) & 0x00F03C0Fu;
        x = (x | x << 3) & 0x06318C63u;
        return x;
    }
    SR_HD static u32 spread1to5(u32 x) {
        x = (x | x << 16) & 0x0030000Fu;
        x = (x | x << 8) & 0x00300C03u;
        x = (x | x << 4) & 0x02108421u;
        return x;
    }
    // enabled(s) & ~self_loops(s) in one pass (has_enabled_moves), the self-loops counted. The fields
    // are extracted once and the 5-bit groups are built bit-parallel, six rms (30 slots) at a time:
    // per rm the group is {TmRcvPrepared not yet recorded, Working, Working, Commit sent and not
    // Committed, Abort sent and not Aborted}.
    SR_HD u32 enabled_moves(const u64* sp, u64* m) const {
        const int n = N();
        const u64 s = sp[0];
        const u32 rmk = (u32)rmask(), ev = (u32)even_mask();
        const bool tm0 = ((s >> (2 * n)) & 3) == 0;
        const u32 prepared = (u32)(s >> (2 * n + 2)) & rmk;
        const u32 msgp = (u32)(s >> (3 * n + 2)) & rmk;
        const bool commit = (s >> (4 * n + 2)) & 1, abort = (s >> (4 * n + 3)) & 1;
        const u32 lo = (u32)s & ev, hi = (u32)(s >> 1) & ev;  // rm_state bits, one rm per even bit
        const u32 work = ~(hi | lo) & ev, is2 = hi & ~lo, is3 = hi & lo;
        const u32 rcv = tm0 ? msgp : 0u;
        const u32 sl0 = rcv & prepared, sl3 = commit ? is2 : 0u, sl4 = abort ? is3 : 0u;  // the self-loops
        const u32 a0 = rcv & ~prepared;                                 // stride 1
        const u32 a13 = work | (commit ? (ev & ~is2) << 1 : 0u);        // stride 2: Working | RmRcvCommitMsg << 1
        const u32 a4 = abort ? ev & ~is3 : 0u;                          // stride 2
        u64 mlo = (u64)(tm0 && prepared == rmk) | (u64)tm0 << 1, mhi = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (6 * k >= n) break;
            const u32 w13 = spread2to5((a13 >> (12 * k)) & 0xfffu);
            const u32 g = spread1to5((a0 >> (6 * k)) & 0x3fu) | (w13 & 0x02108421u) << 1 | w13 << 2 |
                          spread2to5((a4 >> (12 * k)) & 0x555u) << 4;
            const int b = 2 + 30 * k;  // the group's first slot
            mlo |= (u64)g << b;
            if (b + 30 > 64) mhi |= (u64)(g >> (64 - b));
        }
        m[0] = mlo;
        m[1] = mhi;
        return (u32)(__builtin_popcount(sl0) + __builtin_popcount(sl3) + __builtin_popcount(sl4));
    }
    // rm_state fields, bit-parallel: bit 2rm of `ab` is set iff rm is Aborted (3), of `cm` iff
    // Committed (2) (the loop over the rms ran once per property for every new state).
    SR_HD u64 even_mask() const { return 0x5555555555555555ull & ((1ull << (2 * N())) - 1); }
    SR_HD bool discovers(int p, const u64* sp) const {
        const u64 s = sp[0], ev = even_mask();
        const u64 lo = s & ev, hi = (s >> 1) & ev;
        const u64 ab = hi & lo, cm = hi & ~lo;
        if (p == 0) return ab == ev;           // sometimes "abort agreement"
        if (p == 1) return cm == ev;           // sometimes "commit agreement"
        return ab != 0 && cm != 0;             // always "consistent" violated
    }
    int init_states(u64* out) const { out[0] = 0; return 1; }
    // Exact key (quotient visited set): the packed word itself, 4N+4 bits. At N=9 a 2^25-slot
    // table keeps a 15-bit remainder and 17 displacement bits in a 32-bit slot (kernels.hpp).
    int qkey_bits() const { return 4 * N() + 4; }
    SR_HD unsigned __int128 qkey(const u64* s) const { return s[0]; }
    int expectation(int p) const { return p == 2 ? ALWAYS : SOMETIMES; }
    const char* prop_name(int p) const {
        return p == 0 ? "abort agreement" : p == 1 ? "commit agreement" : "consistent";
    }
    int describe_width() const { return 3 * n + 3; }
    void describe(const u64* sp, i64* d) const {
        u64 s = sp[0];
        int k = 0;
        for (int rm = 0; rm < n; ++rm) d[k++] = (i64)((s >> (2 * rm)) & 3);
        d[k++] = (i64)((s >> (2 * n)) & 3);
        for (int rm = 0; rm < n; ++rm) d[k++] = (i64)((s >> (2 * n + 2 + rm)) & 1);
        for (int rm = 0; rm < n; ++rm) d[k++] = (i64)((s >> (3 * n + 2 + rm)) & 1);
        d[k++] = (i64)((s >> (4 * n + 2)) & 1);
        d[k++] = (i64)((s >> (4 * n + 3)) & 1);
    }
    void undescribe(const i64* d, u64* sp) const {
        u64 s = 0;
        int k = 0;
        for (int rm = 0; rm < n; ++rm) s |= ((u64)d[k++] & 3) << (2 * rm);
        s |= ((u64)d[k++] & 3) << (2 * n);
        for (int rm = 0; rm < n; ++rm) s |= ((u64)d[k++] & 1) << (2 * n + 2 + rm);
        for (int rm = 0; rm < n; ++rm) s |= ((u64)d[k++] & 1) << (3 * n + 2 + rm);
        s |= ((u64)d[k++] & 1) << (4 * n + 2);
        s |= ((u64)d[k++] & 1) << (4 * n + 3);
        sp[0] = s;
    }
    // Canonical representative under permutations of the resource managers (the symmetry the
    // reference's `representative` exploits, examples/2pc.rs:156-187): the per-RM tuples
    // (rm_state, tm_prepared, Prepared{rm} in msgs) sorted ascending by that 4-bit key. Unlike the
    // reference's sort by rm_state alone (ties kept in index order), equal orbits always give equal
    // words, so the reduced state count does not depend on the visit order.
    SR_HD void canonical(const u64* sp, u64* o) const {
        const int n = N();
        const u64 s = sp[0];
        u32 cnt[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) cnt[k] = 0;
        for (int rm = 0; rm < n; ++rm) {
            const u32 key = (u32)((s >> (2 * rm)) & 3) | (u32)((s >> (2 * n + 2 + rm)) & 1) << 2 |
                            (u32)((s >> (3 * n + 2 + rm)) & 1) << 3;
            ++cnt[key];
        }
        u64 r = s & (3ull << (2 * n) | 3ull << (4 * n + 2));  // tm_state, Commit, Abort
        int rm = 0;
        for (u32 key = 0; key < 16; ++key)
            for (u32 c = 0; c < cnt[key]; ++c, ++rm)
                r |= (u64)(key & 3) << (2 * rm) | (u64)(key >> 2 & 1) << (2 * n + 2 + rm) | (u64)(key >> 3 & 1) << (3 * n + 2 + rm);
        o[0] = r;
    }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return 2 + 5 * n; }
    std::string action_name(i64 id) const {
        if (id == 0) return "TmCommit";
        if (id == 1) return "TmAbort";
        const char* names[] = {"TmRcvPrepared", "RmPrepare", "RmChooseToAbort", "RmRcvCommitMsg", "RmRcvAbortMsg"};
        return std::string(names[(id - 2) % 5]) + "(" + std::to_string((id - 2) / 5) + ")";
    }
};
using TwoPhase = TwoPhaseT<0>;

// -----------------------------------------------------------------------------------------------
// TwoPhaseLive(n): two-phase commit with two `eventually` properties after its three (no reference
// counterpart; the model of the complete `eventually` check's progress mode, live.hpp). State,
// slots, `apply` and every hook are TwoPhase's, so `action_masks`, `enabled_moves` and
// SELF_LOOPS_EXACT hold for it as they do there (unlike Canon / EvBits, which replace `apply`), and
// its counts are 2pc's. 2pc has NO terminal state: once Commit or Abort is in msgs, RmRcvCommitMsg /
// RmRcvAbortMsg stay enabled for ever as self-loops, so the search's own rule never refutes these
// properties and the plain complete check refutes every one by stuttering.
//   3  eventually "every RM decides": every rm is Committed or Aborted (holds under progress fairness)
//   4  eventually "every RM commits": refuted by a path to the all-aborted stutter end
// -----------------------------------------------------------------------------------------------
struct TwoPhaseLive : TwoPhase {
    static constexpr int NPROPS = 5;
    u32 emask() const { return 3u << 3; }
    SR_HD bool discovers(int p, const u64* sp) const {
        if (p < 3) return TwoPhase::discovers(p, sp);
        const u64 ev = even_mask(), hi = (sp[0] >> 1) & ev, lo = sp[0] & ev;
        return p == 3 ? hi == ev : (hi & ~lo) == ev;  // rm_state 2 or 3 everywhere; 2 everywhere
    }
    int expectation(int p) const { return p < 3 ? TwoPhase::expectation(p) : EVENTUALLY; }
    const char* prop_name(int p) const { return p < 3 ? TwoPhase::prop_name(p) : p == 3 ? "every RM decides" : "every RM commits"; }
};

// -----------------------------------------------------------------------------------------------
// TwoPhaseStep(n): two-phase commit with two STEP properties after its three (no reference counterpart;
// the model of the step pass, step.hpp). State, slots, `apply` and every hook are TwoPhase's, so its counts
// are 2pc's; the search never evaluates the two.
//   3  step "a decided RM stays decided": an rm that is Committed or Aborted keeps its rm_state (holds: only
//      RmRcvCommitMsg / RmRcvAbortMsg write a decided rm, and Commit and Abort are never both sent)
//   4  step "the TM never aborts once an RM is prepared": refuted by RmPrepare(rm), TmAbort
// -----------------------------------------------------------------------------------------------
struct TwoPhaseStep : TwoPhase {
    static constexpr int NPROPS = 5;
    u32 smask() const { return 3u << 3; }
    SR_HD bool discovers(int p, const u64* sp) const { return p < 3 && TwoPhase::discovers(p, sp); }
    SR_HD bool step_holds(int p, const u64* sp, int a, const u64* tp) const {
        const u64 ev = even_mask(), hi = (sp[0] >> 1) & ev, lo = sp[0] & ev;
        if (p == 3) return ((sp[0] ^ tp[0]) & (hi | hi << 1)) == 0;
        return !(a == 1 && (lo & ~hi) != 0);
    }
    int expectation(int p) const { return p < 3 ? TwoPhase::expectation(p) : ALWAYS_STEP; }
    const char* prop_name(int p) const {
        return p < 3 ? TwoPhase::prop_name(p) : p == 3 ? "a decided RM stays decided" : "the TM never aborts once an RM is prepared";
    }
};

// -----------------------------------------------------------------------------------------------
// Ladder(K, F): a test fixture (no reference counterpart) for models with `action_masks` whose slot
// count passes 64, where a table held one slot per lane and a one-word mask both end. K rungs are
// climbed in order and F free bits are set in any order: (K + 1) * 2^F states, depth K + F.
//   [0,6)    rung   0..K (K <= 62)
//   [6,6+F)  free bits
// Slot k < K: enabled iff rung == k; rung <- k + 1. Slot K + j: enabled iff free bit j is clear;
// sets it. (One bit per rung, slot k setting bit k, would need K + F = 66 bits at the 66 slots of
// K = 58, F = 8; a one-word state has 63. The rung counter also makes the table clear a field.)
// -----------------------------------------------------------------------------------------------
struct Ladder {
    static constexpr int W = 1, MW = 2, NPROPS = 1;
    int k, f;  // K <= 62, F <= 57, K + F <= 128
    int max_actions() const { return k + f; }
    int max_out_degree() const { return 1 + f; }
    SR_HD void enabled(const u64* sp, u64* m) const {
        const u64 s = sp[0];
        const u32 rung = (u32)(s & 63);
        const u64 fr = ~(s >> 6) & ((1ull << f) - 1);  // the free bits still clear
        unsigned __int128 e = (unsigned __int128)fr << k;
        if (rung < (u32)k) e |= (unsigned __int128)1 << rung;
        m[0] = (u64)e;
        m[1] = (u64)(e >> 64);
    }
    SR_HD bool apply(const u64* sp, int a, u64* o) const {
        const u64 s = sp[0];
        o[0] = a < k ? (s & ~63ull) | (u64)(a + 1) : s | 1ull << (6 + a - k);
        return true;
    }
    SR_HD void action_masks(int a, u64* clr, u64* set) const {
        *clr = a < k ? 63ull : 0ull;
        *set = a < k ? (u64)(a + 1) : 1ull << ((6 + a - k) & 63);
    }
    static constexpr bool SELF_LOOPS_EXACT = true;  // every enabled slot changes the state
    SR_HD bool discovers(int, const u64* sp) const { return (sp[0] & 63) > (u64)k; }  // always "on the ladder"
    int init_states(u64* out) const { out[0] = 0; return 1; }
    int expectation(int) const { return ALWAYS; }
    const char* prop_name(int) const { return "on the ladder"; }
    int describe_width() const { return 2; }
    void describe(const u64* s, i64* d) const { d[0] = (i64)(s[0] & 63); d[1] = (i64)(s[0] >> 6); }
    void undescribe(const i64* d, u64* s) const { s[0] = ((u64)d[0] & 63) | (u64)d[1] << 6; }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return k + f; }
    std::string action_name(i64 id) const {
        return id < k ? "Climb(" + std::to_string(id) + ")" : "Set(" + std::to_string(id - k) + ")";
    }
};

// -----------------------------------------------------------------------------------------------
// Spread<W>(B, F, loops, mark[, roots, dup]): a test fixture (no reference counterpart) whose key width is a
// parameter, so that a check can be put into any slot encoding of the visited set (kernels.hpp
// make_table_view) whatever its size. A state is a subset x of F free bits, packed into a key of
// B bits, F < B <= min(64 W, 128):
//   key = (x | filler(x) << F) mod 2^B, little-endian in words 0 and 1 (word 1 only for W >= 2)
// filler(x) is 128 bits, 64-bit chunk c being fmix64(x + an odd constant of c): every key bit up
// to B - 1 is pseudo-random, and the key stays injective because x sits in its low bits. W = 4:
// words 2 and 3 hold chunks 2 and 3 of the filler, so all four words are loaded, stored and
// compared (equal x <=> equal words).
// Slot j < F: enabled iff bit j of x is clear; sets it. Slots F .. F + loops - 1 (loops <= 4) are
// always enabled and return the state itself, and are NOT reported through `self_loops`.
// 2^F states, depth F, 1 + F 2^(F-1) + loops 2^F generated; level L holds C(F, L) states, each
// generated by L parents. always "in range": the words are the packing of their own x (never
// violated). sometimes "marked": x == mark.
// Init states: the subsets 0 .. roots - 1 in that order, then 0 .. dup - 1 once more (duplicates,
// which the reference counts, queues and expands again, bfs.rs:43-66); 1 <= roots <= 2^F,
// 0 <= dup <= roots, roots + dup <= 512. The default (1, 0) is the single root x = 0. x = 0 is always
// a root, so the reachable set is all 2^F subsets; generated = (roots + dup) + F 2^(F-1) + loops 2^F
// + sum over i < dup of (F - popcount(i) + loops); depth = max over x of the fewest bits that x adds
// to a root inside it (F - j for roots = 2^j).
// -----------------------------------------------------------------------------------------------
template <int W_>
struct Spread {
    static_assert(W_ == 1 || W_ == 2 || W_ == 4, "Spread: 1, 2 or 4 words");
    static constexpr int W = W_, MW = 1, NPROPS = 2;
    int b, f, loops;
    u64 mark;
    int roots = 1, dup = 0;
    int max_actions() const { return f + loops; }
    int max_out_degree() const { return f + loops; }
    SR_HD static u64 chunk(u64 x, int c) { return fmix64(x + 0x9E3779B97F4A7C15ull * (u64)(2 * c + 1)); }
    SR_HD u64 fmask() const { return (1ull << f) - 1; }
    SR_HD void pack(u64 x, u64* o) const {
        const unsigned __int128 fill = (unsigned __int128)chunk(x, 0) | (unsigned __int128)chunk(x, 1) << 64;
        unsigned __int128 key = (unsigned __int128)x | fill << f;
        if (b < 128) key &= ((unsigned __int128)1 << b) - 1;
        o[0] = (u64)key;
        if constexpr (W_ >= 2) o[1] = (u64)(key >> 64);
        if constexpr (W_ == 4) {
            o[2] = chunk(x, 2);
            o[3] = chunk(x, 3);
        }
    }
    SR_HD void enabled(const u64* s, u64* m) const { m[0] = (~s[0] & fmask()) | ((1ull << loops) - 1) << f; }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        if (a < f) {
            pack((s[0] & fmask()) | 1ull << a, o);
        } else {
#pragma unroll
            for (int i = 0; i < W_; ++i) o[i] = s[i];
        }
        return true;
    }
    SR_HD bool discovers(int p, const u64* s) const {
        const u64 x = s[0] & fmask();
        if (p == 1) return x == mark;  // sometimes "marked"
        u64 t[W_];                     // always "in range": discovered at a state that is not pack(x)
        pack(x, t);
        bool same = true;
#pragma unroll
        for (int i = 0; i < W_; ++i) same &= t[i] == s[i];
        return !same;
    }
    int init_count() const { return roots + dup; }
    int init_states(u64* out) const {
        for (int i = 0; i < roots; ++i) pack((u64)i, out + i * W_);
        for (int i = 0; i < dup; ++i) pack((u64)i, out + (roots + i) * W_);
        return roots + dup;
    }
    int expectation(int p) const { return p == 0 ? ALWAYS : SOMETIMES; }
    const char* prop_name(int p) const { return p == 0 ? "in range" : "marked"; }
    int qkey_bits() const { return b; }
    SR_HD unsigned __int128 qkey(const u64* s) const {
        if constexpr (W_ == 1) return s[0];
        else return (unsigned __int128)s[0] | ((unsigned __int128)s[1] << 64);
    }
    // x, then the low and the high 32 bits of every word
    int describe_width() const { return 1 + 2 * W_; }
    void describe(const u64* s, i64* d) const {
        d[0] = (i64)(s[0] & fmask());
        for (int i = 0; i < W_; ++i) {
            d[1 + 2 * i] = (i64)(s[i] & 0xffffffffull);
            d[2 + 2 * i] = (i64)(s[i] >> 32);
        }
    }
    void undescribe(const i64* d, u64* s) const {
        for (int i = 0; i < W_; ++i) s[i] = ((u64)d[1 + 2 * i] & 0xffffffffull) | (u64)d[2 + 2 * i] << 32;
    }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return f + loops; }
    std::string action_name(i64 id) const {
        return id < f ? "Set(" + std::to_string(id) + ")" : "Loop(" + std::to_string(id - f) + ")";
    }
};

// -----------------------------------------------------------------------------------------------
// Increment (examples/increment.rs:109-197), n <= 15 threads: i (4 bits) then per thread
// t (4 bits) + pc (2 bits, values 1..3). 4+6n bits; W = 1 for n <= 9, else 2.
// Slot = thread id (each thread has at most one enabled action: Read at pc 1, Write at pc 2).
// -----------------------------------------------------------------------------------------------
template <int W_>
struct Increment {
    static constexpr int W = W_, MW = 1, NPROPS = 1;
    int n;
    int max_actions() const { return n; }
    int max_out_degree() const { return n; }
    SR_HD static int toff(int t) { return 4 + 6 * t; }
    SR_HD void enabled(const u64* s, u64* m) const {
        u64 r = 0;
        for (int t = 0; t < n; ++t) {
            u64 pc = getb(s, toff(t) + 4, 2);
            r |= (u64)(pc == 1 || pc == 2) << t;
        }
        m[0] = r;
    }
    SR_HD bool apply(const u64* s, int t, u64* o) const {
#pragma unroll
        for (int i = 0; i < W; ++i) o[i] = s[i];
        u64 pc = getb(s, toff(t) + 4, 2);
        if (pc == 1) {  // Read: s[t] = {t: i, pc: 2}
            setb(o, toff(t), 4, getb(s, 0, 4));
            setb(o, toff(t) + 4, 2, 2);
        } else {  // Write: pc = 3; i = t + 1
            setb(o, toff(t) + 4, 2, 3);
            setb(o, 0, 4, getb(s, toff(t), 4) + 1);
        }
        return true;
    }
    SR_HD bool discovers(int, const u64* s) const {  // always "fin": #(pc == 3) == i
        u64 c = 0;
        for (int t = 0; t < n; ++t) c += getb(s, toff(t) + 4, 2) == 3;
        return c != getb(s, 0, 4);
    }
    int init_states(u64* out) const {
        for (int i = 0; i < W; ++i) out[i] = 0;
        for (int t = 0; t < n; ++t) setb(out, toff(t) + 4, 2, 1);
        return 1;
    }
    int expectation(int) const { return ALWAYS; }
    const char* prop_name(int) const { return "fin"; }
    // Exact key (quotient visited set) of the two-word layout: word 0 is full (4 + 6*10 = 64 bits),
    // word 1 holds threads 10.. : the state is an integer below 2^(4 + 6n).
    int qkey_bits() const { return 4 + 6 * n; }
    SR_HD unsigned __int128 qkey(const u64* s) const {
        if constexpr (W_ == 1) return s[0];
        else return (unsigned __int128)s[0] | ((unsigned __int128)s[W_ - 1] << 64);
    }
    int describe_width() const { return 1 + 2 * n; }
    void describe(const u64* s, i64* d) const {
        d[0] = (i64)getb(s, 0, 4);
        for (int t = 0; t < n; ++t) {
            d[1 + 2 * t] = (i64)getb(s, toff(t), 4);
            d[2 + 2 * t] = (i64)getb(s, toff(t) + 4, 2);
        }
    }
    void undescribe(const i64* d, u64* s) const {
        for (int i = 0; i < W; ++i) s[i] = 0;
        setb(s, 0, 4, (u64)d[0]);
        for (int t = 0; t < n; ++t) {
            setb(s, toff(t), 4, (u64)d[1 + 2 * t]);
            setb(s, toff(t) + 4, 2, (u64)d[2 + 2 * t]);
        }
    }
    i64 action_id(const u64* s, int t) const { return 2 * t + (getb(s, toff(t) + 4, 2) == 2 ? 1 : 0); }
    i64 action_id_bound() const { return 2 * n; }
    std::string action_name(i64 id) const {
        return std::string(id % 2 ? "Write(" : "Read(") + std::to_string(id / 2) + ")";
    }
    // Coverage classes (cover.hpp): the canonical action ids, Read(t) and Write(t).
    SR_HD int cover_class(const u64* s, int t) const { return 2 * t + (getb(s, toff(t) + 4, 2) == 2 ? 1 : 0); }
    int cover_classes() const { return 2 * n; }
    std::string cover_class_name(int c) const { return action_name(c); }
};

// -----------------------------------------------------------------------------------------------
// IncrementLock (examples/increment_lock.rs:3-107), n <= 12 threads: i (4 bits), lock (1 bit),
// then per thread t (4 bits) + pc (3 bits, 0..4); 5+7n bits, W = 1 for n <= 8, else 2.
// Per-thread fields are placed so that none crosses a word boundary.
// -----------------------------------------------------------------------------------------------
template <int W_>
struct IncrementLock {
    static constexpr int W = W_, MW = 1, NPROPS = 2;
    int n;
    int max_actions() const { return n; }
    int max_out_degree() const { return n; }
    // threads 0..7 live in word 0 (bits 5..60), threads 8.. in word 1 (bits 0..)
    SR_HD static int toff(int t) { return t < 8 ? 5 + 7 * t : 64 + 7 * (t - 8); }
    // Bit-parallel over the threads: bit 0 of thread t's pc field sits at pc_pos(t); pc_mask(w) has
    // those bits of word w, so b0/b1/b2 of every pc are three masked shifts of the word.
    SR_HD static int pc_pos(int t) { return t < 8 ? 9 + 7 * t : 4 + 7 * (t - 8); }
    SR_HD u64 pc_mask(int w) const {
        u64 m = 0;
        for (int t = w == 0 ? 0 : 8; t < (w == 0 ? (n < 8 ? n : 8) : n); ++t) m |= 1ull << pc_pos(t);
        return m;
    }
    SR_HD void enabled(const u64* s, u64* m) const {
        const bool lock = (s[0] >> 4) & 1;
        u64 r = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 M = pc_mask(w), x = s[w];
            const u64 b0 = x & M, b1 = (x >> 1) & M, b2 = (x >> 2) & M;
            // Lock at pc 0 (lock free), Read at 1, Write at 2, Release at 3 (lock held)
            const u64 en = ~b2 & ((b1 ^ b0) | (~(b1 | b0) & (lock ? 0 : M)) | (b1 & b0 & (lock ? M : 0))) & M;
            for (int t = w == 0 ? 0 : 8; t < (w == 0 ? (n < 8 ? n : 8) : n); ++t) r |= ((en >> pc_pos(t)) & 1) << t;
        }
        m[0] = r;
    }
    // Every action advances pc by one (Lock 0->1, Read 1->2, Write 2->3, Release 3->4); the other
    // field it writes is selected without branches (the lanes of a wave run different threads).
    SR_HD bool apply(const u64* s, int t, u64* o) const {
#pragma unroll
        for (int i = 0; i < W; ++i) o[i] = s[i];
        const u64 pc = getb(s, toff(t) + 4, 3), iv = getb(s, 0, 4), tv = getb(s, toff(t), 4);
        const u64 lock = getb(s, 4, 1);
        setb(o, toff(t) + 4, 3, pc + 1);
        setb(o, 4, 1, pc == 0 ? 1 : pc == 3 ? 0 : lock);  // Lock / Release
        setb(o, toff(t), 4, pc == 1 ? iv : tv);           // Read: t = i
        setb(o, 0, 4, pc == 2 ? tv + 1 : iv);             // Write: i = t + 1
        return true;
    }
    SR_HD bool discovers(int p, const u64* s) const {
        u64 fin = 0, crit = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 M = pc_mask(w), x = s[w];
            const u64 b0 = x & M, b1 = (x >> 1) & M, b2 = (x >> 2) & M;
            fin += __builtin_popcountll(b2 | (b1 & b0));   // pc >= 3
            crit += __builtin_popcountll(~b2 & (b1 | b0) & M);  // 1 <= pc < 4
        }
        if (p == 0) return fin != getb(s, 0, 4);  // always "fin"
        return crit > 1;                          // always "mutex"
    }
    int init_states(u64* out) const {
        for (int i = 0; i < W; ++i) out[i] = 0;
        return 1;
    }
    int expectation(int) const { return ALWAYS; }
    const char* prop_name(int p) const { return p == 0 ? "fin" : "mutex"; }
    // Exact key (quotient visited set), 5 + 6n bits: i and lock, then one 6-bit code per thread for
    // its (t, pc) pair: pc while pc < 2 (t is still 0 there: it is set by Read, pc 1 -> 2), else
    // 2 + 3t + (pc - 2) <= 49. Injective on every state whose threads hold t = 0 before their Read
    // and pc <= 4, i.e. on every reachable state. Two bits per thread shorter than the packed
    // words (5 + 7n): at N = 12 the key is 77 bits, so a table of 2^33 slots keeps 20 displacement
    // bits per slot (a probe limit far beyond any run) where the packed words left 8 (254 slots).
    int qkey_bits() const { return 5 + 6 * n; }
    SR_HD unsigned __int128 qkey(const u64* s) const {
        u64 lo = s[0] & 31, hi = 0;  // threads 0..8 in lo bits 5..58, threads 9.. in hi
        for (int t = 0; t < n; ++t) {
            const u64 f = getb(s, toff(t), 7);  // t | pc << 4
            const u64 tv = f & 15, pc = f >> 4;
            const u64 code = pc < 2 ? pc : 2 + 3 * tv + (pc - 2);
            if (t < 9) lo |= code << (5 + 6 * t);
            else hi |= code << (6 * (t - 9));
        }
        return (unsigned __int128)lo | ((unsigned __int128)hi << 59);
    }
    int describe_width() const { return 2 + 2 * n; }
    void describe(const u64* s, i64* d) const {
        d[0] = (i64)getb(s, 0, 4);
        d[1] = (i64)getb(s, 4, 1);
        for (int t = 0; t < n; ++t) {
            d[2 + 2 * t] = (i64)getb(s, toff(t), 4);
            d[3 + 2 * t] = (i64)getb(s, toff(t) + 4, 3);
        }
    }
    void undescribe(const i64* d, u64* s) const {
        for (int i = 0; i < W; ++i) s[i] = 0;
        setb(s, 0, 4, (u64)d[0]);
        setb(s, 4, 1, (u64)d[1]);
        for (int t = 0; t < n; ++t) {
            setb(s, toff(t), 4, (u64)d[2 + 2 * t]);
            setb(s, toff(t) + 4, 3, (u64)d[3 + 2 * t]);
        }
    }
    i64 action_id(const u64* s, int t) const { return 4 * t + (i64)getb(s, toff(t) + 4, 3); }
    i64 action_id_bound() const { return 4 * n; }
    std::string action_name(i64 id) const {
        const char* names[] = {"Lock", "Read", "Write", "Release"};
        return std::string(names[id % 4]) + "(" + std::to_string(id / 4) + ")";
    }
    // Coverage classes (cover.hpp): the canonical action ids, Lock / Read / Write / Release(t).
    SR_HD int cover_class(const u64* s, int t) const { return 4 * t + (int)getb(s, toff(t) + 4, 3); }
    int cover_classes() const { return 4 * n; }
    std::string cover_class_name(int c) const { return action_name(c); }
};

// -----------------------------------------------------------------------------------------------
// LiveGraph(n_bits, degree, seed, p_mod, t_mod, roots): a test fixture (no reference counterpart)
// with cycles at scale, for the complete `eventually` check (live.hpp): a pseudo-random graph of
// out-degree `degree` over the states v < 2^n_bits (n_bits <= 24, degree 1..4), one word, whose
// packed key is v itself, so every quotient encoding applies. The key is DECLARED n_bits + 8 bits
// wide: most of the 2^n_bits states are reachable, and a table with at least as many slots as the
// key space has values homes every key in its first half (kernels.hpp make_table_view: a 1-bit
// remainder), where a dense key space would pile into probe runs of millions of slots; the 8 spare
// bits keep the hashed keys sparse, as Spread's filler does. With r(v, k) = fmix64((fmix64(seed ^ v) + k) mod 2^64):
//   v has no actions iff t_mod > 0 and r(v, degree) % t_mod == 0 (a terminal state);
//   otherwise slot k < degree leads to r(v, k) mod 2^n_bits; the action id is k.
// eventually "marked": p_mod > 0 and r(v, degree + 1) % p_mod == 0. Init states 0 .. roots-1
// (1 <= roots <= 512). An optional seventh parameter, words = 1 (the default), 2 or 4, widens the state:
// word i >= 1 holds fmix64(v + an odd constant of i), so every word is loaded, stored, shuffled and
// compared (equal v <=> equal words), while the graph, the key and the description stay those of v.
// An optional eighth parameter dup (default 0, dup <= roots, roots + dup <= 512) repeats the init states
// 0 .. dup-1 after the roots, as Spread's does: duplicates that the search counts, queues and expands again.
// -----------------------------------------------------------------------------------------------
template <int W_>
struct LiveGraphT {
    static_assert(W_ == 1 || W_ == 2 || W_ == 4, "LiveGraph: 1, 2 or 4 words");
    static constexpr int W = W_, MW = 1, NPROPS = 1;
    static constexpr bool FAIR_SLOTS = true;  // edge k of every state is one fairness class (live.hpp, weak fairness)
    int n_bits, degree;
    u64 seed;
    u32 p_mod, t_mod;
    int roots;
    int dup = 0;
    SR_HD u64 r(u64 v, u64 k) const { return fmix64(fmix64(seed ^ v) + k); }
    int max_actions() const { return degree; }
    int max_out_degree() const { return degree; }
    u32 emask() const { return 1u; }
    SR_HD void enabled(const u64* s, u64* m) const { m[0] = t_mod && r(s[0], (u64)degree) % t_mod == 0 ? 0ull : (1ull << degree) - 1; }
    SR_HD static void pack(u64 v, u64* o) {
        o[0] = v;
#pragma unroll
        for (int i = 1; i < W_; ++i) o[i] = fmix64(v + 0x9E3779B97F4A7C15ull * (u64)(2 * i + 1));
    }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        pack(r(s[0], (u64)a) & ((1ull << n_bits) - 1), o);
        return true;
    }
    SR_HD bool discovers(int, const u64* s) const { return p_mod && r(s[0], (u64)degree + 1) % p_mod == 0; }  // the condition holds
    int init_count() const { return roots + dup; }
    int init_states(u64* out) const {
        for (int i = 0; i < roots + dup; ++i) pack((u64)(i < roots ? i : i - roots), out + i * W_);
        return roots + dup;
    }
    int expectation(int) const { return EVENTUALLY; }
    const char* prop_name(int) const { return "marked"; }
    int qkey_bits() const { return n_bits + 8; }
    SR_HD unsigned __int128 qkey(const u64* s) const { return s[0]; }
    int describe_width() const { return 1; }
    void describe(const u64* s, i64* d) const { d[0] = (i64)s[0]; }
    void undescribe(const i64* d, u64* s) const { pack((u64)d[0] & ((1ull << n_bits) - 1), s); }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return degree; }
    std::string action_name(i64 id) const { return "Edge(" + std::to_string(id) + ")"; }
};
using LiveGraph = LiveGraphT<1>;

// -----------------------------------------------------------------------------------------------
// LeadsGraph(n_bits, degree, seed, p_mod, t_mod, roots, q_mod[, words[, dup]]): LiveGraph's graph, key
// and description, with the leads-to properties of the complete check (live.hpp, LEADS-TO):
//   0  eventually "marked", as in LiveGraph;
//   1  leads-to "armed ~> marked": the trigger is q_mod > 0 and r(v, degree + 2) % q_mod == 0;
//   2  leads-to "always eventually marked": the trigger is true ([]<>marked).
// -----------------------------------------------------------------------------------------------
template <int W_>
struct LeadsGraphT : LiveGraphT<W_> {
    using B = LiveGraphT<W_>;
    static constexpr int NPROPS = 3;
    u32 q_mod = 0;
    u32 emask() const { return 1u; }
    SR_HD u32 lmask() const { return 6u; }
    SR_HD bool leads_from(int p, const u64* s) const {
        return p == 2 || (p == 1 && q_mod && B::r(s[0], (u64)B::degree + 2) % q_mod == 0);
    }
    int expectation(int p) const { return p == 0 ? EVENTUALLY : LEADS_TO; }
    const char* prop_name(int p) const { return p == 0 ? "marked" : p == 1 ? "armed ~> marked" : "always eventually marked"; }
};
using LeadsGraph = LeadsGraphT<1>;

// -----------------------------------------------------------------------------------------------
// StepGraph(n_bits, degree, seed, f_mod, t_mod, roots[, words[, dup]]): LiveGraph's graph, key and
// description, with the two step properties of the step pass (step.hpp) and no other:
//   0  "no forbidden step": the step (v, slot k) is forbidden iff f_mod > 0 and
//      r(v, degree + 3 + k) % f_mod == 0 (f_mod up to 2^63 - 1: a large one forbids nothing);
//   1  "never down": violated iff the successor is below v, so the hook has to read the successor.
// -----------------------------------------------------------------------------------------------
template <int W_>
struct StepGraphT : LiveGraphT<W_> {
    using B = LiveGraphT<W_>;
    static constexpr int NPROPS = 2;
    u64 f_mod = 0;
    u32 emask() const { return 0u; }
    u32 smask() const { return 3u; }
    SR_HD bool discovers(int, const u64*) const { return false; }
    SR_HD bool step_holds(int p, const u64* s, int a, const u64* t) const {
        if (p == 0) return !(f_mod && B::r(s[0], (u64)B::degree + 3 + (u64)a) % f_mod == 0);
        return !(t[0] < s[0]);
    }
    int expectation(int) const { return ALWAYS_STEP; }
    const char* prop_name(int p) const { return p == 0 ? "no forbidden step" : "never down"; }
};
using StepGraph = StepGraphT<1>;

// -----------------------------------------------------------------------------------------------
// SpinLock(n): n threads take a lock in turn while a clock ticks (no reference counterpart; the
// model of the complete `eventually` check's weak-fairness mode, live.hpp). One word, and the
// packed key is the word. The key is DECLARED 8 bits wider than the word, as LiveGraph's is: (n + 1)
// 2^(n+1) of the word's 2^(n+6) values are reachable, and a table with as many slots as a dense key
// space has values homes every key in its first half (kernels.hpp make_table_view), which from
// n = 16 on has fewer slots than the model has states; the spare bits keep the hashed keys sparse.
//   [0,5)      holder  0 = free, i + 1 = thread i holds the lock (n <= 20)
//   [5,5+n)    served  bit i: thread i has released the lock at least once
//   5+n        tick
// Slot i < n is Acquire(i), enabled iff the lock is free; slot n + i is Release(i), enabled iff
// thread i holds it: it sets served bit i and frees the lock; slot 2n is Tick, always enabled,
// flipping tick. No slot is a no-op, and a slot is a fairness class (FAIR_SLOTS): a thread's
// acquire, a thread's release, the clock. (n + 1) 2^n 2 states, one init state (all zero).
//   0  eventually "some thread served":  refuted with no fairness and under progress fairness by
//      the two-state Tick cycle; holds under weak fairness (Acquire(i) stays moving-enabled round
//      that cycle and is never taken)
//   1  eventually "every thread served": refuted under weak fairness too, by a starvation lasso:
//      Acquire(1) is disabled whenever thread 0 holds the lock, so weak fairness does not protect
//      thread 1 (strong fairness would)
// -----------------------------------------------------------------------------------------------
struct SpinLock {
    static constexpr int W = 1, MW = 1, NPROPS = 2;
    static constexpr bool FAIR_SLOTS = true;
    static constexpr bool SELF_LOOPS_EXACT = true;  // every enabled slot changes the state
    int n;
    int max_actions() const { return 2 * n + 1; }
    int max_out_degree() const { return n + 1; }
    u32 emask() const { return 3u; }
    SR_HD u64 served_mask() const { return ((1ull << n) - 1) << 5; }
    SR_HD void enabled(const u64* sp, u64* m) const {
        const u32 holder = (u32)(sp[0] & 31);
        m[0] = (holder ? 1ull << (n + holder - 1) : (1ull << n) - 1) | 1ull << (2 * n);
    }
    SR_HD bool apply(const u64* sp, int a, u64* o) const {
        const u64 s = sp[0];
        if (a < n) o[0] = s | (u64)(a + 1);                               // (enabled: holder == 0)
        else if (a < 2 * n) o[0] = (s & ~31ull) | 1ull << (5 + a - n);     // (enabled: holder == a - n + 1)
        else o[0] = s ^ 1ull << (5 + n);
        return true;
    }
    SR_HD bool discovers(int p, const u64* sp) const {  // the condition holds
        const u64 sv = sp[0] & served_mask();
        return p == 0 ? sv != 0 : sv == served_mask();
    }
    int init_states(u64* out) const { out[0] = 0; return 1; }
    int expectation(int) const { return EVENTUALLY; }
    const char* prop_name(int p) const { return p == 0 ? "some thread served" : "every thread served"; }
    int qkey_bits() const { return 14 + n; }
    SR_HD unsigned __int128 qkey(const u64* s) const { return s[0]; }
    int describe_width() const { return 3; }
    void describe(const u64* s, i64* d) const {
        d[0] = (i64)(s[0] & 31);
        d[1] = (i64)((s[0] & served_mask()) >> 5);
        d[2] = (i64)(s[0] >> (5 + n) & 1);
    }
    void undescribe(const i64* d, u64* s) const { s[0] = ((u64)d[0] & 31) | (u64)d[1] << 5 | ((u64)d[2] & 1) << (5 + n); }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return 2 * n + 1; }
    std::string action_name(i64 id) const {
        if (id == 2 * n) return "Tick";
        return std::string(id < n ? "Acquire(" : "Release(") + std::to_string(id < n ? id : id - n) + ")";
    }
};

// -----------------------------------------------------------------------------------------------
// ReqLock(n): SpinLock's lock with threads that first have to ASK for it (no reference counterpart; the
// model of the leads-to check, live.hpp LEADS-TO). One word, the packed key is the word, declared 8 bits
// wider as SpinLock's is. N threads (1..8) is a template parameter: the model has N + 1 properties.
//   [0,5)      holder   0 = free, i + 1 = thread i holds the lock
//   [5,5+n)    waiting  bit i: thread i has asked and does not hold yet
//   5+n        tick
// Slot i < n is Request(i), enabled iff thread i neither waits nor holds: it sets waiting(i); n + i is
// Acquire(i), enabled iff the lock is free and i waits: i holds, waiting(i) is cleared; 2n + i is Release(i),
// enabled iff i holds: the lock is free again; 3n is Tick, always enabled, flipping tick. No slot is a no-op
// and a slot is a fairness class. (2^n + n 2^(n-1)) 2 states, one init state (all zero).
//   p < n  leads-to "thread p waiting ~> thread p holds": refuted with no fairness and under progress fairness
//          by the clock's cycle, under weak fairness for n >= 2 by starvation (Acquire(p) is disabled whenever
//          another thread holds), proved under strong fairness
//   n      eventually "some thread holds": refuted with no and under progress fairness, holds under weak
// -----------------------------------------------------------------------------------------------
template <int N>
struct ReqLockT {
    static_assert(N >= 1 && N <= 8, "ReqLock: 1..8 threads");
    static constexpr int W = 1, MW = 1, NPROPS = N + 1;
    static constexpr bool FAIR_SLOTS = true;
    static constexpr bool SELF_LOOPS_EXACT = true;  // every enabled slot changes the state
    static constexpr int n = N;
    int max_actions() const { return 3 * n + 1; }
    int max_out_degree() const { return n + 1; }
    u32 emask() const { return 1u << n; }
    SR_HD u32 lmask() const { return (1u << n) - 1; }
    SR_HD void enabled(const u64* sp, u64* m) const {
        const u32 holder = (u32)(sp[0] & 31);
        const u64 all = (1ull << n) - 1, waiting = sp[0] >> 5 & all;
        u64 e = 1ull << (3 * n);
        if (holder) e |= (~waiting & all & ~(1ull << (holder - 1))) | 1ull << (2 * n + holder - 1);
        else e |= (~waiting & all) | waiting << n;
        m[0] = e;
    }
    SR_HD bool apply(const u64* sp, int a, u64* o) const {
        const u64 s = sp[0];
        if (a < n) o[0] = s | 1ull << (5 + a);                                          // Request
        else if (a < 2 * n) o[0] = (s & ~(1ull << (5 + a - n))) | (u64)(a - n + 1);     // Acquire (enabled: holder == 0)
        else if (a < 3 * n) o[0] = s & ~31ull;                                          // Release
        else o[0] = s ^ 1ull << (5 + n);
        return true;
    }
    SR_HD bool discovers(int p, const u64* sp) const {  // the condition holds
        const u32 holder = (u32)(sp[0] & 31);
        return p < n ? holder == (u32)p + 1 : holder != 0;
    }
    SR_HD bool leads_from(int p, const u64* sp) const { return p < n && (sp[0] >> (5 + p) & 1); }
    int init_states(u64* out) const { out[0] = 0; return 1; }
    int expectation(int p) const { return p < n ? LEADS_TO : EVENTUALLY; }
    const char* prop_name(int p) const {
        static const char* const names[8] = {
            "thread 0 waiting ~> thread 0 holds", "thread 1 waiting ~> thread 1 holds", "thread 2 waiting ~> thread 2 holds",
            "thread 3 waiting ~> thread 3 holds", "thread 4 waiting ~> thread 4 holds", "thread 5 waiting ~> thread 5 holds",
            "thread 6 waiting ~> thread 6 holds", "thread 7 waiting ~> thread 7 holds"};
        return p < n ? names[p] : "some thread holds";
    }
    int qkey_bits() const { return 14 + n; }
    SR_HD unsigned __int128 qkey(const u64* s) const { return s[0]; }
    int describe_width() const { return 3; }
    void describe(const u64* s, i64* d) const {
        d[0] = (i64)(s[0] & 31);
        d[1] = (i64)(s[0] >> 5 & ((1ull << n) - 1));
        d[2] = (i64)(s[0] >> (5 + n) & 1);
    }
    void undescribe(const i64* d, u64* s) const { s[0] = ((u64)d[0] & 31) | ((u64)d[1] & ((1ull << n) - 1)) << 5 | ((u64)d[2] & 1) << (5 + n); }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return 3 * n + 1; }
    std::string action_name(i64 id) const {
        if (id == 3 * n) return "Tick";
        const char* kind = id < n ? "Request(" : id < 2 * n ? "Acquire(" : "Release(";
        return std::string(kind) + std::to_string(id % n) + ")";
    }
};

// -----------------------------------------------------------------------------------------------
// FairRings(d, w, core, lanes): nested rings, the fixture of the complete `eventually` check's
// strong-fairness mode (live.hpp; no reference counterpart). Lane j < lanes has the rings 0 .. d_j,
// d_j = 1 + (j mod d), of w positions each, and one `done` state. One word, and the packed key is
// the word, declared 8 bits wider as SpinLock's is:
//   [0,6)    x     the position on the ring, x < w (4 <= w <= 64)
//   [6,11)   k     the ring, k <= d_j (1 <= d <= 28)
//   [11,20)  j     the lane (1 <= lanes <= 512)
//   20       done
// Slots, 2d + 3 of them, each a fairness class (FAIR_SLOTS); no step is a no-op:
//   0          Step    (k, x) -> (k, (x + 1) mod w), always enabled off `done`
//   1 + k      Out(k)  enabled at (k, 0): for k = 0 to the lane's `done` state, else to (k - 1, 0); where
//                      the lane's CORE is on (core == 1, or core == 2 and j is odd) and k = d_j, also
//                      enabled at (k, 2), leading to (k, 0)
//   d + 2 + k  In(k)   enabled at (k, 1) iff k < d_j: to (k + 1, 1)
// `done` is terminal. One property, eventually "done"; init states (j, 0, 0) for every lane.
// A lane is one strongly connected component and unfair under strong fairness (Out(0) leaves it);
// without the states that enable Out(0) the rings 1 .. d_j are one and Out(1) leaves them, and so on
// inwards: the innermost ring is a component at depth d_j + 1, fair iff the core is on. So the
// property holds under strong fairness iff core = 0, and weak fairness refutes it in every lane.
// lanes + sum_j (d_j + 1) w states.
// -----------------------------------------------------------------------------------------------
struct FairRings {
    static constexpr int W = 1, MW = 1, NPROPS = 1;
    static constexpr bool FAIR_SLOTS = true;
    static constexpr bool SELF_LOOPS_EXACT = true;  // every enabled slot changes the state
    static constexpr u64 DONE = 1ull << 20;
    int d, w, core, lanes;
    int max_actions() const { return 2 * d + 3; }
    int max_out_degree() const { return 2; }
    u32 emask() const { return 1u; }
    SR_HD static u64 pack(u32 j, u32 k, u32 x) { return (u64)x | (u64)k << 6 | (u64)j << 11; }
    SR_HD u32 depth_of(u32 j) const { return 1u + j % (u32)d; }
    SR_HD bool core_on(u32 j) const { return core == 1 || (core == 2 && (j & 1)); }
    SR_HD void enabled(const u64* sp, u64* m) const {
        const u64 s = sp[0];
        const u32 x = (u32)(s & 63), k = (u32)(s >> 6 & 31), j = (u32)(s >> 11 & 511);
        u64 e = 0;
        if (!(s & DONE)) {
            e = 1;
            if (x == 0 || (x == 2 && k == depth_of(j) && core_on(j))) e |= 1ull << (1 + k);
            if (x == 1 && k < depth_of(j)) e |= 1ull << (d + 2 + k);
        }
        m[0] = e;
    }
    SR_HD bool apply(const u64* sp, int a, u64* o) const {
        const u64 s = sp[0];
        const u32 x = (u32)(s & 63), k = (u32)(s >> 6 & 31), j = (u32)(s >> 11 & 511);
        if (a == 0) o[0] = pack(j, k, x + 1 == (u32)w ? 0 : x + 1);
        else if (a <= d + 1) o[0] = x ? pack(j, k, 0) : k ? pack(j, k - 1, 0) : pack(j, 0, 0) | DONE;
        else o[0] = pack(j, k + 1, 1);
        return true;
    }
    SR_HD bool discovers(int, const u64* sp) const { return (sp[0] & DONE) != 0; }  // the condition holds
    int init_count() const { return lanes; }
    int init_states(u64* out) const {
        for (int j = 0; j < lanes; ++j) out[j] = pack((u32)j, 0, 0);
        return lanes;
    }
    int expectation(int) const { return EVENTUALLY; }
    const char* prop_name(int) const { return "done"; }
    int qkey_bits() const { return 29; }
    SR_HD unsigned __int128 qkey(const u64* s) const { return s[0]; }
    int describe_width() const { return 4; }
    void describe(const u64* s, i64* o) const {
        o[0] = (i64)(s[0] >> 11 & 511);
        o[1] = (i64)(s[0] >> 6 & 31);
        o[2] = (i64)(s[0] & 63);
        o[3] = (i64)(s[0] >> 20 & 1);
    }
    void undescribe(const i64* o, u64* s) const { s[0] = pack((u32)o[0] & 511, (u32)o[1] & 31, (u32)o[2] & 63) | (o[3] & 1 ? DONE : 0); }
    i64 action_id(const u64*, int a) const { return a; }
    i64 action_id_bound() const { return 2 * d + 3; }
    std::string action_name(i64 id) const {
        if (id == 0) return "Step";
        return std::string(id <= d + 1 ? "Out(" : "In(") + std::to_string(id <= d + 1 ? id - 1 : id - d - 2) + ")";
    }
};

// Models whose action slots are fairness classes (`static constexpr bool FAIR_SLOTS = true`): the
// complete `eventually` check's weak-fairness mode (live.hpp) treats every slot as one action that
// a fair run may not ignore for ever. Where a slot is a network position or a queue entry (the actor
// encodings, paxos, the registers) it names no action of the model, and the mode is refused.
template <class M, class = void>
struct fair_slots : std::false_type {};
template <class M>
struct fair_slots<M, std::void_t<decltype(M::FAIR_SLOTS)>> : std::integral_constant<bool, M::FAIR_SLOTS> {};
template <class M>
constexpr bool fair_slots_model = fair_slots<M>::value && !is_canon<M>::value && !is_evbits<M>::value;

}  // namespace sr
