// The kernels of the complete `eventually` check (gfx950), over the rule defined in live.hpp (this
// header is included from there, after that definition). They run after a search that explored
// everything, on its arena and its final visited set; a state is named by its visited-set SLOT
// (find_slot over probe_key), so they work with every slot encoding and with the table any growth
// or doubling left behind. Nothing here is shared with the expanding kernels but those lookups.
//
//   live_mark  one lane per arena state: finds the state's own slot once (kept per arena index),
//              sets its bit in the ALIVE bitmap (one bit per table slot) iff it is in N_p, and
//              appends it to the first worklist. A duplicate init state (the arena holds level 0
//              as given) marks and is listed once: the lane whose atomicOr set the bit.
//   live_trim  one lane per worklist entry: live_step over the state's successors, a lookup and a
//              bit test each, stopping at the first alive one. A terminal state keeps its bit and
//              leaves the worklist for good; a state with an alive successor keeps its bit and goes
//              to the next worklist (its witness may die later); any other state clears its bit.
//              Bits are cleared in place while other lanes read them: a lane that still sees a
//              cleared bit set only keeps its state one round longer, and the host stops after a
//              round that removed nothing, in which every read was exact.
//   live_first_init  one workgroup: the init state of lowest index whose bit survived.
//   live_walk  one wave follows the witness rule from the state in out[0]: its lanes share the
//              enabled slots (lane, lane + 64, ..), each finds its lowest alive successor, and the
//              lowest slot of the wave wins. Every state is written to `out` and its slot marked in
//              the ON-PATH bitmap; the walk ends at a terminal state, at a state whose slot is
//              already marked, or after max_steps steps (the host launches it again from the last
//              state, so no launch is long).
// The trim is latency-bound on dependent lookups, as the probe is: a lane's successors are looked up
// one after the other (the scan stops at the first hit), so its parallelism is the worklist's, 256
// lanes per workgroup and as many workgroups as the worklist has entries for. Worklists hold 4-byte
// arena indices and are appended per wave with one atomic (live_append, wave_append's aggregation
// for an index instead of a staged state).
// live_trim and live_walk are instantiated for both values of live_step's FAIR switch (progress
// fairness, live.hpp); live_mark and live_first_init do not step and are shared. With FAIR a stutter
// end (every successor is the state itself) keeps its bit and leaves the worklist for good, like a
// terminal state, and the walk ends there with LIVE_WALK_STUTTER; the FAIR = false instantiations are
// the kernels as they were, and the only ones launched with the mode off. FAIR adds a W-word compare
// per successor (none for a model whose `enabled_moves` names its self-loops exactly), no LDS and no
// lookup: the trim stays bound by the latency of its dependent lookups.
#pragma once

namespace sr {

constexpr u32 LIVE_BLOCK = 256;
constexpr u32 LIVE_WALK_STEPS = 1u << 16;  // steps of one live_walk launch at most

enum LiveErr : u32 {
    LIVE_ERR_LOOKUP = 1,  // find_slot did not find a reachable state or a successor of one
    LIVE_ERR_STUCK = 2,   // a state of the fixpoint with successors, none of them alive
};
enum LiveWalkEnd : u32 { LIVE_WALK_MORE = 0, LIVE_WALK_TERMINAL = 1, LIVE_WALK_LOOP = 2, LIVE_WALK_STUTTER = 3 };

struct LiveCounters {
    u32 next_n;   // entries appended to the worklist being written
    u32 removed;  // states this round removed
    u32 err;      // LiveErr
    u32 steps;    // live_walk: steps taken by the launch
    u32 end;      // live_walk: LiveWalkEnd
    u32 first_init;  // live_first_init: the lowest init index whose state is alive (~0: none)
};

__device__ __forceinline__ bool live_bit(const u32* bits, u64 slot) {
    return __hip_atomic_load(&bits[slot >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (slot & 31) & 1;
}

// Appends v for every lane with nw, one atomic per wave; called by whole waves.
__device__ __forceinline__ void live_append(bool nw, u32 v, u32* __restrict__ list, u32* cursor) {
    const u64 mask = __ballot(nw);
    if (!mask) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(mask);
    u32 base = 0;
    if (lane == leader) base = atomicAdd(cursor, (u32)__popcll(mask));
    base = lane_u32(base, (u32)leader);
    if (nw) list[base + (u32)__popcll(mask & ((1ull << lane) - 1))] = v;
}

// wl has room for n entries (every arena index is appended at most once).
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_mark(M m, const u64* __restrict__ arena, u32 n, TableView t, int p,
                                                        u64* __restrict__ slot_of, u32* alive, u32* __restrict__ wl,
                                                        LiveCounters* lc) {
    const u32 i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool nw = false;
    if (i < n) {
        u64 s[M::W];
        load_state<M::W>(arena, i, s);
        const u64 slot = find_slot(t, probe_key(m, t, s));
        slot_of[i] = slot;
        if (slot == ~0ull) {
            atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
        } else if (live_not_p(m, p, s)) {
            const u32 bit = 1u << (slot & 31);
            nw = !(atomicOr(&alive[slot >> 5], bit) & bit);
        }
    }
    live_append(nw, i, wl, &lc->next_n);
}

// next has room for n entries (it takes a subset of wl's).
template <class M, bool FAIR = false>
__global__ void __launch_bounds__(LIVE_BLOCK) live_trim(M m, const u64* __restrict__ arena, TableView t,
                                                        const u64* __restrict__ slot_of, u32* alive,
                                                        const u32* __restrict__ wl, u32 n, u32* __restrict__ next,
                                                        LiveCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool keep = false, dead = false;
    u32 idx = 0;
    if (g < n) {
        idx = wl[g];
        u64 s[M::W], out[M::W];
        load_state<M::W>(arena, idx, s);
        bool lost = false;
        const int r = live_step<FAIR>(
            m, s,
            [&](const u64* ns) {
                const u64 sl = find_slot(t, probe_key(m, t, ns));
                if (sl == ~0ull) {
                    lost = true;
                    return false;
                }
                return live_bit(alive, sl);
            },
            out);
        if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
        keep = r >= 0;
        dead = r == LIVE_DEAD;  // (LIVE_TERMINAL, LIVE_STUTTER: a sink, neither kept nor dead)
        if (dead) {
            const u64 sl = slot_of[idx];
            atomicAnd(&alive[sl >> 5], ~(1u << (sl & 31)));
        }
    }
    live_append(keep, idx, next, &lc->next_n);
    const u64 dm = __ballot(dead);
    if (dm && (int)(threadIdx.x & 63) == __builtin_ctzll(dm)) atomicAdd(&lc->removed, (u32)__popcll(dm));
}

// The lowest i < k whose init state is alive, into lc->first_init (set to ~0 before the launch). Level 0
// of the arena holds the init states in REVERSE order: init state i is arena index k - 1 - i. One
// workgroup (k <= a few hundred).
template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_first_init(const u64* __restrict__ slot_of, const u32* alive, u32 k,
                                                              LiveCounters* lc) {
    for (u32 i = threadIdx.x; i < k; i += LIVE_BLOCK)
        if (live_bit(alive, slot_of[k - 1 - i])) atomicMin(&lc->first_init, i);
}

// One wave. out holds max_steps + 1 states: out[0] is the state to go on from (resume = 0: the
// walk's first state, marked on the path here; 1: the last state of the previous launch), state
// k + 1 the one step k reached. lc->steps / lc->end say where and why the launch stopped. FAIR: the
// wave ends TERMINAL only if no lane saw any successor, STUTTER if none found a successor other than
// the state itself and some lane saw the state itself; LIVE_ERR_STUCK means what it meant.
template <class M, bool FAIR = false>
__global__ void __launch_bounds__(64) live_walk(M m, TableView t, const u32* alive, u32* onpath, u64* out, u32 max_steps,
                                                u32 resume, LiveCounters* lc) {
    constexpr int W = M::W;
    const u32 lane = threadIdx.x;
    u64 cur[W];
    load_state<W>(out, 0, cur);
    u32 err = 0;
    if (!resume) {
        const u64 sl = find_slot(t, probe_key(m, t, cur));
        if (sl == ~0ull) err |= LIVE_ERR_LOOKUP;
        else if (lane == 0) atomicOr(&onpath[sl >> 5], 1u << (sl & 31));
        __threadfence();
    }
    u32 k = 0, end = LIVE_WALK_MORE;
    while (!err && k < max_steps) {  // (every condition below is wave-uniform)
        u64 nx[W];
        bool lost = false;
        const int r = live_step<FAIR>(
            m, cur,
            [&](const u64* ns) {
                const u64 sl = find_slot(t, probe_key(m, t, ns));
                if (sl == ~0ull) {
                    lost = true;
                    return false;
                }
                return live_bit(alive, sl);
            },
            nx, lane, 64u);
        if (__ballot(lost)) {
            err |= LIVE_ERR_LOOKUP;
            break;
        }
        int best = r >= 0 ? r : 0x7fffffff;
#pragma unroll
        for (int o = 32; o; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        if (best == 0x7fffffff) {
            if (__ballot(r == LIVE_DEAD)) err |= LIVE_ERR_STUCK;
            else if (FAIR && __ballot(r == LIVE_STUTTER)) end = LIVE_WALK_STUTTER;
            else end = LIVE_WALK_TERMINAL;
            break;
        }
        const int winner = __builtin_ctzll(__ballot(r == best));
#pragma unroll
        for (int x = 0; x < W; ++x) cur[x] = (u64)__shfl((unsigned long long)nx[x], winner, 64);
        ++k;
        if (lane == 0) store_state<W>(out, k, cur);
        const u64 sl = find_slot(t, probe_key(m, t, cur));  // (found: live_step looked it up)
        if (sl == ~0ull) {
            err |= LIVE_ERR_LOOKUP;
            break;
        }
        if (live_bit(onpath, sl)) {
            end = LIVE_WALK_LOOP;
            break;
        }
        if (lane == 0) atomicOr(&onpath[sl >> 5], 1u << (sl & 31));
        __threadfence();  // the mark is in the L2 before the next step's test reads it (a self-loop reads it at once)
    }
    if (lane == 0) {
        lc->steps = k;
        lc->end = end;
        if (err) atomicOr(&lc->err, err);
    }
}

}  // namespace sr
