// The simulation checker's kernel (gfx950): simulate_walks<M, REFILL, LOOPS, UNIQUE> runs one batch of random walks, the
// walks of consecutive indices [b0, b0 + n), with the walk defined in sim.hpp (this header is
// included from there, after that definition).
//
// One lane carries one walk with its state in registers (W words); no LDS, no visited set. With
// loop detection (LOOPS = true, sim.hpp "Loop detection") a lane also keeps the checkpoint in
// registers and the window of its last 8 fingerprints in LDS (SimRingLds below); the LOOPS = false
// instantiations hold none of that code. Results
// are keyed by the walk index, never by lane or wave, so both forms below give the same per-walk
// records and the same hits:
//   static form (REFILL = false): lane g of the grid walks index b0 + g, and a wave runs as long as
//     its longest walk;
//   persistent form (REFILL = true): a fixed grid; a lane whose walk has ended takes the next
//     unstarted index of the batch. Indices are reserved with ONE atomic per wave and refill: the
//     idle lanes are balloted, one lane adds their count to the batch cursor, and the lanes rank
//     themselves by prefix popcount. The reservation is issued one step BEFORE the index is
//     needed (every lane holds its next index while it still walks), and its result is read at the
//     top of the next step: a returning atomic waited on at once stalls the wave (DESIGN.md §3
//     "dynamic chunks").
// Hits: per property one 64-bit word, the minimum of t << 40 | w. A lane compares with a plain load
// of the current best first and issues atomicMin only for a better key, so after the first hits
// almost nothing is issued (a stale load can only cost one atomic, never a result).
// Counters: per lane in registers, reduced per wave at its exit and added once per wave to one of
// the NSHARD shard lines (blockIdx % NSHARD), as the BFS counters are.
//
// Distinct-state table (UNIQUE = true, sim.hpp "Distinct-state count"; the UNIQUE = false
// instantiations hold none of this code). Visiting s_t inserts f = state_fp<M>(s_t) into an
// open-addressing table of 8-byte slots in HBM that all lanes share and that lives across the batches
// of a check. The step is laid out around the memory latency, and the walk never waits on an insert:
//   1. f and its home slot are computed and the home slot is LOADED (a plain load) before
//      sim_advance, which then runs under that load's latency (with LOOPS it takes f as given);
//   2. after sim_advance the lane probes on with plain loads: a slot that holds f ends the insert
//      (a duplicate: in a covered state space nearly every insert ends at this first load), another
//      fingerprint moves it one slot on, and only a VACANT slot costs an atomicCAS. A stale vacant
//      value (another compute unit claimed the slot since) only falls through to the CAS, which is
//      the arbiter: a slot goes vacant -> fingerprint exactly once;
//   3. the CAS is issued and NOT waited for: only the claimant needs what it returns, and a returning
//      atomic waited on at once stalls the whole wave for a round trip to the memory side. Its
//      result is read one pass later, after that pass's sim_advance (behind the next home-slot load,
//      which returns after it anyway): vacant -> the lane counts a new fingerprint; f -> another lane
//      won with the same fingerprint, a duplicate; anything else -> the same probe goes on from the
//      next slot, now waiting on its accesses (rare: two different new fingerprints met in one slot).
// Step 0 of a batch is every lane arriving at the few init states' slots. Once such a slot is
// claimed they cost loads only; for the first arrivals, the lanes of a wave that are about to
// claim are deduplicated in ONE round: the lanes whose fingerprint equals that of the lowest such
// lane leave the claim to it (it carries the insert to its end, so they are duplicates whatever
// its CAS returns). That is two readlanes and a compare, only on passes where some lane claims; a
// full match-any over up to 64 distinct fingerprints would cost every early pass of a run more than
// the atomics it saves, since apart from step 0 the claiming lanes of a wave hold different states.
// New fingerprints are counted per lane and added per wave to the shard line, like the states.
// Probing is bounded by SimArgs::uq_limit = min(slots, 1024); an insert that exhausts it is dropped
// and sets *uq_flag (an atomic vector store), which every lane reads at the top of a pass: once it
// is set nothing more is inserted (the count is then a lower bound; the walks go on unchanged).
// What keeps that layout in the compiled code (checked in the gfx950 assembly of the 2pc N=9
// counting kernel: between the flag load at the top of a pass and the end of sim_advance there is no
// vector-memory wait outside the branch that starts a walk and the branches of a property's new
// hit, and none between the CAS and the loop's back edge). vmcnt retires in order, so ANY wait for
// an older access also waits for the claim in flight, and the compiler inserts such waits freely:
//   - the flag is loaded through an index the compiler cannot see through (uq_zero): a uniform load
//     is moved to a scalar register where it is issued, which waits on the spot;
//   - the init state is loaded per source (device memory or kernel arguments) so that the loads
//     are global, not flat (an outstanding flat load turns every wait into vmcnt(0)), and it is
//     waited for inside the branch that starts the walk;
//   - every load is consumed on every path (the flag, the home slot when the flag is set, no load
//     behind the last probe): a value left in flight is waited for where its register is next written.
#pragma once

namespace sr {

constexpr u32 SIM_BLOCK = 256;
constexpr u32 SIM_PERSIST_WAVES = 16;  // persistent form: waves per compute unit

struct alignas(16) SimRecord {  // record_walks: one per walk, at index w - b0
    u32 steps;
    u32 end;  // the SimEnd in the low byte; SIM_LOOP: loop_start (<= 2^20) in the bits above it
    u64 fp;   // state_fp<M> of the walk's last state
};
static_assert(sizeof(SimRecord) == 16, "one 16-byte store per record");

struct alignas(128) SimShard {
    u64 states;    // states visited
    u64 ended[SIM_ENDS];  // walks ended, by SimEnd
    u32 longest;   // the longest walk, in steps
    u64 fresh;     // distinct-state count: fingerprints this batch claimed in the table
};
static_assert(sizeof(SimShard) == 128, "one shard line");
struct SimDevice {
    SimShard shard[NSHARD];
    alignas(128) u32 cursor;  // persistent form: indices handed out past the grid's first ones
    alignas(128) u64 best[MAX_PROPS];
};

struct SimArgs {
    u64 seed, b0;
    u32 n, max_depth, init_count, emask;
    const u64* inits;  // nullptr: the init states ride in the kernel arguments
    SimDevice* dev;
    SimRecord* records;  // nullptr: none
    // distinct-state table (UNIQUE instantiations only; null / 0 otherwise)
    u64* uq_keys;        // 2^uq_log2 slots, 0 = vacant
    u32* uq_flag;        // set once an insert was dropped
    u32 uq_log2, uq_limit;
    u32 uq_refill;       // the counting forms are compiled with REFILL = true: 0 = reserve nothing (the static form)
};

__device__ __forceinline__ u64 sim_wave_sum(u64 v) {
    unsigned long long x = v;
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ u32 sim_wave_max(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, (u32)__shfl_xor((int)v, o, 64));
    return v;
}

// The window of a lane's loop memory (sim.hpp SimLoops): the workgroup's LDS, laid out
// ring[slot][thread], 8 x 256 x 8 B = 16 KiB. A wave's 8-byte access at one slot covers 512
// consecutive bytes, and a slot is 2 KiB (a multiple of the 256-byte bank row), so lanes at
// different slots (the persistent form: different t) keep their own banks too: no conflict in the
// 32-lane groups of a 64-bit read or the 16-lane groups of a 64-bit write. 16 KiB per workgroup of
// four waves leaves the wave limit of a compute unit (32 waves: 128 KiB) inside its 160 KiB.
struct SimRingLds {
    u64* lane;  // &ring[0][threadIdx.x]
    __device__ __forceinline__ u64 get(u32 slot) const { return lane[slot * SIM_BLOCK]; }
    __device__ __forceinline__ void put(u32 slot, u64 v) { lane[slot * SIM_BLOCK] = v; }
};

// The distinct-state insert of one lane (UNIQUE). A claim in flight: fingerprint f (0: none), issued
// at slot i as probe number k of f's insert; prev is what the CAS returned.
struct SimClaim {
    u64 f = 0, i = 0, prev = 0;
    u32 k = 0;
};
__device__ __forceinline__ u64 sim_unique_cas(u64* keys, u64 i, u64 f) {
    return atomicCAS(reinterpret_cast<unsigned long long*>(keys + i), 0ull, (unsigned long long)f);
}
__device__ __forceinline__ void sim_unique_drop(const SimArgs& a) {
    __hip_atomic_store(a.uq_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Carries the insert of f to its end from slot i (probe number k), waiting on every access: the
// slow path behind a claim that lost its slot to another fingerprint. Bounded by uq_limit.
__device__ __forceinline__ void sim_unique_finish(const SimArgs& a, u64 f, u64 i, u32 k, u32& fresh) {
    const u64 mask = (1ull << a.uq_log2) - 1;
    for (; k < a.uq_limit; ++k, i = (i + 1) & mask) {
        u64 v = a.uq_keys[i];
        if (v == 0) v = sim_unique_cas(a.uq_keys, i, f), fresh += v == 0;  // (vacant: the slot is ours now)
        if (v == 0 || v == f) return;
    }
    sim_unique_drop(a);
}
// Probes on for f from slot i, whose value v is loaded, with plain loads. Returns true if the insert
// needs a claim of slot i (probe number k); false if it is settled (a duplicate, or dropped).
__device__ __forceinline__ bool sim_unique_seek(const SimArgs& a, u64 f, u64& i, u64 v, u32& k) {
    const u64 mask = (1ull << a.uq_log2) - 1;
    for (k = 0;;) {  // (no load is left unread at the exit: see the kernel on loads left in flight)
        if (v == f) return false;
        if (v == 0) return true;
        if (++k >= a.uq_limit) break;
        i = (i + 1) & mask;
        v = a.uq_keys[i];
    }
    sim_unique_drop(a);
    return false;
}

// The fingerprints of the distinct-state table, in no order: every non-vacant slot is appended to
// out (room for out_cap; the host passes the count it summed, which is the number of such slots).
// (A template only for its linkage: this header is part of every reg_*.hip unit.)
template <int UNUSED = 0>
__global__ void __launch_bounds__(SIM_BLOCK) sim_unique_gather(const u64* keys, u64 slots, u64* out, u64 out_cap,
                                                                unsigned long long* cursor) {
    const u32 lane = threadIdx.x & 63;
    const u64 stride = (u64)gridDim.x * SIM_BLOCK;
    // (whole waves pass the loop together: the bound is rounded up to the wave)
    for (u64 i0 = (u64)blockIdx.x * SIM_BLOCK + (threadIdx.x & ~63u); i0 < slots; i0 += stride) {
        const u64 i = i0 + lane;
        const u64 v = i < slots ? keys[i] : 0;
        const u64 have = __ballot(v != 0);
        if (!have) continue;
        unsigned long long base = 0;
        const int src = __builtin_ctzll(have);
        if ((int)lane == src) base = atomicAdd(cursor, (unsigned long long)__builtin_popcountll(have));
        base = __shfl(base, src, 64);
        const u64 pos = base + (u64)__builtin_popcountll(have & ((1ull << lane) - 1));
        if (v != 0 && pos < out_cap) out[pos] = v;
    }
}

template <class M, bool REFILL, bool LOOPS, bool UNIQUE = false>
__global__ void __launch_bounds__(SIM_BLOCK) simulate_walks(M m, SimArgs a, InlineStates inl) {
    constexpr u32 NONE = ~0u;
    const u32 lane = threadIdx.x & 63;
    const u32 g = blockIdx.x * SIM_BLOCK + threadIdx.x;
    const u32 first = gridDim.x * SIM_BLOCK;  // the persistent form's cursor starts past these
    const u64* inits = a.inits ? a.inits : inl.w;

    SimWalk<M> wk;
    u32 cur = NONE;                // index (relative to b0) of the walk this lane carries
    u32 next = g < a.n ? g : NONE; // the index it starts next
    bool exhausted = !REFILL || g >= a.n;  // no further index to reserve
    if constexpr (UNIQUE) exhausted = exhausted || !a.uq_refill;  // (the counting forms choose the form at run time)
    u32 pend_base = 0;             // (the reserving lane) the cursor before its add
    u64 pend_mask = 0;             // lanes of the reservation in flight
    int pend_src = 0;
    u64 c_states = 0;
    u32 c_term = 0, c_depth = 0, c_fault = 0, c_longest = 0;
    u32 c_loop = 0;
    std::conditional_t<LOOPS, SimLoops<SimRingLds>, SimNoLoops> lp;
    if constexpr (LOOPS) {
        __shared__ u64 ring[SIM_LOOP_WINDOW][SIM_BLOCK];
        lp.ring.lane = &ring[0][threadIdx.x];  // (never cleared: a walk reads only what it wrote, by its own t)
    }
    SimClaim claim;   // (UNIQUE) this lane's claim in flight
    u32 c_fresh = 0;  // (UNIQUE) fingerprints this lane claimed
    u32 uq_zero = 0;  // (UNIQUE) zero, in a vector register the compiler takes for unknown: see the flag load
    if constexpr (UNIQUE) asm volatile("" : "+v"(uq_zero));

    // Bounded: every pass either advances a walk (at most max_depth + 1 passes each), starts one, or
    // lands a reservation; the batch has n walks and a lane reserves past n at most once.
    for (;;) {
        if constexpr (REFILL) {
            if (pend_mask) {  // (wave-uniform) last pass's reservation lands
                const u32 base = (u32)__shfl((int)pend_base, pend_src, 64);
                if (pend_mask >> lane & 1) {
                    const u32 rank = (u32)__builtin_popcountll(pend_mask & ((1ull << lane) - 1));
                    const u64 idx = (u64)first + base + rank;
                    if (idx < a.n) next = (u32)idx;
                    else exhausted = true;
                }
                pend_mask = 0;
            }
        }
        if (cur == NONE && next != NONE) {
            cur = next;
            next = NONE;
            if constexpr (UNIQUE) {
                // `inits` is a select between device memory and the kernel arguments, so its loads are
                // FLAT, and while a flat load is outstanding the compiler waits for every vector memory
                // access at once (vmcnt(0)): that would drain the home-slot load and the claim in
                // flight at the first use of the state. One call per source keeps the loads global.
                if (a.inits) sim_start<M>(wk, a.seed, a.b0 + cur, a.inits, a.init_count);
                else sim_start<M>(wk, a.seed, a.b0 + cur, inl.w, a.init_count);
                // ... and the init state is waited for HERE, in the branch that loaded it (taken once
                // per walk). Left in flight, every pass would wait for "all but the youngest access"
                // at the state's first use, and vmcnt retires in order: that is the claim in flight.
#pragma unroll
                for (int j = 0; j < M::W; ++j) asm volatile("" ::"v"(wk.s[j]));
            } else {
                sim_start<M>(wk, a.seed, a.b0 + cur, inits, a.init_count);
            }
        }
        if constexpr (REFILL) {
            const u64 need = __ballot(next == NONE && !exhausted);
            if (need) {
                pend_mask = need;
                pend_src = __builtin_ctzll(need);
                if ((int)lane == pend_src) pend_base = atomicAdd(&a.dev->cursor, (u32)__builtin_popcountll(need));
            }
        }
        bool ins = false;  // (UNIQUE) this pass visits a state whose fingerprint is to be inserted
        u64 ins_i = 0, ins_v = 0;
        std::conditional_t<UNIQUE, SimFpGiven, SimFpOwn> fpv{};
        u32 full = 0;
        if constexpr (UNIQUE) {
            // the flag at the top of the pass (L2-served: another compute unit may have set it); like
            // the home slot it is only LOADED here, and consumed after sim_advance, so nothing
            // between here and there depends on either load
            // (uq_zero: a wave-uniform load is moved to a scalar register where it is issued, which
            // waits for it, and for every older access, on the spot; an index the compiler cannot
            // see through keeps the result in a vector register until it is used)
            full = __hip_atomic_load(a.uq_flag + uq_zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ins = cur != NONE;
            if (ins) {
                fpv.f = state_fp<M>(wk.s);
                ins_i = sim_unique_home(fpv.f, a.uq_log2);
                ins_v = a.uq_keys[ins_i];  // (in bounds whatever the flag says)
            }
        }
        if (cur != NONE) {
            const u64 w = a.b0 + cur;
            c_states += 1;
            const u32 e = sim_advance(
                m, wk, a.max_depth, a.emask,
                [&](int p, u32 t) {
                    const u64 key = sim_hit_key(t, w);
                    unsigned long long* best = reinterpret_cast<unsigned long long*>(&a.dev->best[p]);
                    if (key < __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        atomicMin(best, (unsigned long long)key);
                },
                [](const u64*, int) {}, lp, fpv);
            if (e != SIM_RUNNING) {
                c_term += e == SIM_TERMINAL;
                c_depth += e == SIM_DEPTH;
                c_fault += e == SIM_FAULT;
                u32 endw = e;
                if constexpr (LOOPS) {
                    c_loop += e == SIM_LOOP;
                    if (e == SIM_LOOP) endw |= lp.start << 8;
                }
                c_longest = max(c_longest, wk.t);
                if (a.records) {
                    const u64 fp = state_fp<M>(wk.s);
                    ulonglong2 r;
                    r.x = (u64)wk.t | (u64)endw << 32;
                    r.y = fp;
                    *reinterpret_cast<ulonglong2*>(&a.records[cur]) = r;  // cur < n: one 16-byte store
                }
                cur = NONE;
            }
        }
        if constexpr (UNIQUE) {
            if (claim.f) {  // last pass's claim lands
                if (claim.prev == 0) c_fresh += 1;
                else if (claim.prev != claim.f) sim_unique_finish(a, claim.f, (claim.i + 1) & ((1ull << a.uq_log2) - 1), claim.k + 1, c_fresh);
                claim.f = 0;
            }
            u32 k = 0;
            // Both loads of the pass's top are consumed here on every path: a home-slot value left
            // unread (the flag is set) would be waited for where its register is written next, at
            // the top of the next pass, together with everything older.
            bool want = false;
            asm volatile("" ::"v"(full));
            if (ins && full) asm volatile("" ::"v"(ins_v));
            else if (ins) want = sim_unique_seek(a, fpv.f, ins_i, ins_v, k);
            const u64 claimers = __ballot(want);
            if (claimers) {  // one round of dedup: the lowest claiming lane's fingerprint
                const int src = __builtin_ctzll(claimers);
                const u64 lf = (u64)__shfl((unsigned long long)fpv.f, src, 64);
                if (want && (int)lane != src && fpv.f == lf) want = false;
            }
            if (want) {
                claim.f = fpv.f;
                claim.i = ins_i;
                claim.k = k;
                claim.prev = sim_unique_cas(a.uq_keys, ins_i, fpv.f);  // not waited for: read next pass
            }
        }
        if (!__ballot(cur != NONE || next != NONE) && !pend_mask) break;
    }
    if constexpr (UNIQUE) {
        if (claim.f) {  // the last pass's claim
            if (claim.prev == 0) c_fresh += 1;
            else if (claim.prev != claim.f) sim_unique_finish(a, claim.f, (claim.i + 1) & ((1ull << a.uq_log2) - 1), claim.k + 1, c_fresh);
        }
    }

    const u64 s_states = sim_wave_sum(c_states);
    const u64 s_term = sim_wave_sum(c_term), s_depth = sim_wave_sum(c_depth), s_fault = sim_wave_sum(c_fault);
    const u32 s_longest = sim_wave_max(c_longest);
    u64 s_loop = 0;
    if constexpr (LOOPS) s_loop = sim_wave_sum(c_loop);
    u64 s_fresh = 0;
    if constexpr (UNIQUE) s_fresh = sim_wave_sum(c_fresh);
    if (lane == 0 && s_states) {
        SimShard* sh = &a.dev->shard[blockIdx.x % NSHARD];
        atomicAdd((unsigned long long*)&sh->states, (unsigned long long)s_states);
        if (s_term) atomicAdd((unsigned long long*)&sh->ended[SIM_TERMINAL], (unsigned long long)s_term);
        if (s_depth) atomicAdd((unsigned long long*)&sh->ended[SIM_DEPTH], (unsigned long long)s_depth);
        if (s_fault) atomicAdd((unsigned long long*)&sh->ended[SIM_FAULT], (unsigned long long)s_fault);
        if constexpr (LOOPS) {
            if (s_loop) atomicAdd((unsigned long long*)&sh->ended[SIM_LOOP], (unsigned long long)s_loop);
        }
        if constexpr (UNIQUE) {
            if (s_fresh) atomicAdd((unsigned long long*)&sh->fresh, (unsigned long long)s_fresh);
        }
        atomicMax(&sh->longest, s_longest);
    }
}

}  // namespace sr
