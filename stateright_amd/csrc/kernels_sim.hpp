// The simulation checker's kernel (gfx950): simulate_walks<M, REFILL, LOOPS> runs one batch of random walks, the
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
};
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

template <class M, bool REFILL, bool LOOPS>
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
            sim_start<M>(wk, a.seed, a.b0 + cur, inits, a.init_count);
        }
        if constexpr (REFILL) {
            const u64 need = __ballot(next == NONE && !exhausted);
            if (need) {
                pend_mask = need;
                pend_src = __builtin_ctzll(need);
                if ((int)lane == pend_src) pend_base = atomicAdd(&a.dev->cursor, (u32)__builtin_popcountll(need));
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
                [](const u64*, int) {}, lp);
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
        if (!__ballot(cur != NONE || next != NONE) && !pend_mask) break;
    }

    const u64 s_states = sim_wave_sum(c_states);
    const u64 s_term = sim_wave_sum(c_term), s_depth = sim_wave_sum(c_depth), s_fault = sim_wave_sum(c_fault);
    const u32 s_longest = sim_wave_max(c_longest);
    u64 s_loop = 0;
    if constexpr (LOOPS) s_loop = sim_wave_sum(c_loop);
    if (lane == 0 && s_states) {
        SimShard* sh = &a.dev->shard[blockIdx.x % NSHARD];
        atomicAdd((unsigned long long*)&sh->states, (unsigned long long)s_states);
        if (s_term) atomicAdd((unsigned long long*)&sh->ended[SIM_TERMINAL], (unsigned long long)s_term);
        if (s_depth) atomicAdd((unsigned long long*)&sh->ended[SIM_DEPTH], (unsigned long long)s_depth);
        if (s_fault) atomicAdd((unsigned long long*)&sh->ended[SIM_FAULT], (unsigned long long)s_fault);
        if constexpr (LOOPS) {
            if (s_loop) atomicAdd((unsigned long long*)&sh->ended[SIM_LOOP], (unsigned long long)s_loop);
        }
        atomicMax(&sh->longest, s_longest);
    }
}

}  // namespace sr
