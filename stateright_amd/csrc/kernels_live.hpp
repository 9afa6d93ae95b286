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

// ---- weak fairness (live.hpp: WEAK FAIRNESS). Launched only with sr_opts.liveness = SR_LIVENESS_WEAK, after
// live_mark and the progress trim (live_trim<M, true>), which run as they are. A state of N_p is named by
// its arena index here: IDX maps a visited-set slot to the arena index that live_mark listed for it (~0 for
// a slot outside N_p), so colours, component numbers and ranks are 4-byte arrays by arena index, and a
// successor costs one find_slot and one IDX load. A component is named by its ROOT, the highest arena
// index in it.
//   live_index     IDX and the NP list's states; RANK 0 for the sinks of F_p' (alive, not in U).
//   live_set_bits  the U bitmap from the trim's last worklist (F_p' minus its sinks); live_trim<M, true> on
//                  that bitmap then leaves the states with a successor in U.
//   live_colour_init / live_colour_push  forward max-colouring: every state of U starts with its arena
//                  index and pushes its colour along succ' inside U with atomicMax; a state whose colour
//                  rose is listed once per round (a round stamp) and pushes again in the next round.
//   live_scc_seed / live_scc_join  a state whose colour is its own index is a root and joins its component;
//                  s joins iff it has the root's colour and a successor in U that has joined (a backward
//                  fixpoint evaluated forwards, all roots at once; joins are written in place, which only
//                  lets a state join a round earlier). live_scc_leave clears the U bits of what joined.
//   live_comp_acc  per member of a component: its size, the AND of the me masks and the OR of the slots whose
//                  successor is a member. Lanes of a wave that share the component (the common case: a few
//                  large components) reduce in registers and issue one atomic per word.
//   live_goal      sinks and members of fair components of two or more states get rank 0; the other states
//                  of F_p' are listed for live_reach; roots count the components.
//   live_reach     one level of ranks towards rank 0 inside a domain (the states whose RANK entry is not
//                  frozen at ~0 outside the list): a listed state joins in round r only through a successor
//                  of rank < r, so ranks written in the same round are never read as a reason.
//   live_members / live_targets  one component's members; a slot's target set inside it.
//   live_first_ranked  the init state of lowest index with a rank.
//   live_descend   one wave, lanes sharing the slots as live_walk does: the lowest rank-decreasing slot
//                  down to rank 0, the states to `out`; accumulates the loop's "not moving-enabled
//                  somewhere" and "taken" masks; bounded and resumable like live_walk.
// All of them are bound by the latency of dependent lookups, as live_trim is; none uses LDS.

constexpr int LIVE_MW_MAX = 4;  // mask words of a model in the weak mode (DGraph: 256 slots)

enum LiveDescendEnd : u32 { LIVE_DESCEND_MORE = 0, LIVE_DESCEND_DONE = 1 };

struct LiveWeakCounters {
    u32 next_n;      // entries appended to the list being written
    u32 joined;      // states that joined (a component, the ranked set) / bits set this round
    u32 err;         // LiveErr
    u32 steps;       // live_descend: steps taken by the launch
    u32 end;         // live_descend: LiveDescendEnd
    u32 first_init;  // live_first_ranked
    u32 last_idx;    // live_descend: the arena index of the launch's last state
    u32 comps, fair_comps, goal;
    u64 notme[LIVE_MW_MAX], taken[LIVE_MW_MAX];  // live_descend: accumulated over launches (the host clears them)
};

// The arena index of the N_p state ns (a successor), ~0 if it is outside N_p; a failed lookup sets lost.
template <class M>
__device__ __forceinline__ u32 live_idx_of(const M& m, const TableView& t, const u32* __restrict__ idx, const u64* ns, bool& lost,
                                           u64* slot = nullptr) {
    const u64 sl = find_slot(t, probe_key(m, t, ns));
    if (slot) *slot = sl;
    if (sl == ~0ull) {
        lost = true;
        return ~0u;
    }
    return idx[sl];
}

__device__ __forceinline__ u32 live_load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void live_store(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// np: live_mark's list (every slot of N_p once). u0: the bitmap of F_p' minus its sinks.
template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_index(const u32* __restrict__ np, u32 n, const u64* __restrict__ slot_of,
                                                         const u32* alive, const u32* u0, u32* __restrict__ idx,
                                                         u32* __restrict__ rank) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g >= n) return;
    const u32 i = np[g];
    const u64 sl = slot_of[i];
    idx[sl] = i;
    rank[i] = live_bit(alive, sl) && !live_bit(u0, sl) ? 0u : ~0u;
}

template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_set_bits(const u32* __restrict__ list, u32 n, const u64* __restrict__ slot_of,
                                                            u32* bits) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g >= n) return;
    const u64 sl = slot_of[list[g]];
    atomicOr(&bits[sl >> 5], 1u << (sl & 31));
}

template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_colour_init(const u32* __restrict__ list, u32 n, u32* __restrict__ colour) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g < n) colour[list[g]] = list[g];
}

// next has room for every state of U (a state is listed at most once per round: stamp[t] == round).
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_colour_push(M m, const u64* __restrict__ arena, TableView t,
                                                               const u32* __restrict__ idx, const u32* u, u32* colour, u32* stamp,
                                                               u32 round, const u32* __restrict__ wl, u32 n, u32* __restrict__ next,
                                                               LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g >= n) return;
    const u32 i = wl[g];
    u64 s[M::W], me[M::MW];
    load_state<M::W>(arena, i, s);
    const u32 c = live_load(&colour[i]);
    bool lost = false;
    live_moving(m, s, me, [&](int, const u64* ns) {
        u64 sl;
        const u32 ti = live_idx_of(m, t, idx, ns, lost, &sl);
        if (ti == ~0u || !live_bit(u, sl)) return;
        if (atomicMax(&colour[ti], c) < c && atomicExch(&stamp[ti], round) != round) next[atomicAdd(&lc->next_n, 1u)] = ti;
    });
    if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
}

template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_scc_seed(const u32* __restrict__ list, u32 n, const u32* __restrict__ colour,
                                                            u32* comp) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g < n && colour[list[g]] == list[g]) comp[list[g]] = list[g];
}

// next takes the states of wl that have not joined (a subset of wl).
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_scc_join(M m, const u64* __restrict__ arena, TableView t,
                                                            const u32* __restrict__ idx, const u32* u,
                                                            const u32* __restrict__ colour, u32* comp, const u32* __restrict__ wl,
                                                            u32 n, u32* __restrict__ next, LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool keep = false, join = false;
    u32 i = 0;
    if (g < n) {
        i = wl[g];
        if (live_load(&comp[i]) == ~0u) {
            u64 s[M::W], me[M::MW];
            load_state<M::W>(arena, i, s);
            const u32 c = colour[i];
            bool lost = false;
            live_moving(m, s, me, [&](int, const u64* ns) {
                if (join) return;
                u64 sl;
                const u32 ti = live_idx_of(m, t, idx, ns, lost, &sl);
                if (ti == ~0u || !live_bit(u, sl)) return;
                join = colour[ti] == c && live_load(&comp[ti]) != ~0u;
            });
            if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
            if (join) live_store(&comp[i], c);
            keep = !join;
        }
    }
    live_append(keep, i, next, &lc->next_n);
    const u64 jm = __ballot(join);
    if (jm && (int)(threadIdx.x & 63) == __builtin_ctzll(jm)) atomicAdd(&lc->joined, (u32)__popcll(jm));
}

template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_scc_leave(const u32* __restrict__ list, u32 n, const u64* __restrict__ slot_of,
                                                             const u32* __restrict__ comp, u32* u) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g >= n || comp[list[g]] == ~0u) return;
    const u64 sl = slot_of[list[g]];
    atomicAnd(&u[sl >> 5], ~(1u << (sl & 31)));
}

// and_me (all ones before the launch), or_took and size (zero) are by root.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_comp_acc(M m, const u64* __restrict__ arena, TableView t,
                                                            const u32* __restrict__ idx, const u32* __restrict__ comp,
                                                            const u32* __restrict__ list, u32 n, u32* size, u64* and_me,
                                                            u64* or_took, LiveWeakCounters* lc) {
    constexpr int MW = M::MW;
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    u32 root = ~0u;
    u64 me[MW], took[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) me[w] = ~0ull, took[w] = 0;
    if (g < n) {
        const u32 i = list[g];
        root = comp[i];
        if (root != ~0u) {
            u64 s[M::W];
            load_state<M::W>(arena, i, s);
            bool lost = false;
            live_moving(m, s, me, [&](int a, const u64* ns) {
                const u32 ti = live_idx_of(m, t, idx, ns, lost);
                if (ti != ~0u && comp[ti] == root) took[a >> 6] |= 1ull << (a & 63);
            });
            if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
        }
    }
    const u64 active = __ballot(root != ~0u);
    if (!active) return;
    const int leader = __builtin_ctzll(active);
    const u32 first = lane_u32(root, (u32)leader);
    if (!__ballot(root != ~0u && root != first)) {  // the wave's members share one component
#pragma unroll
        for (int w = 0; w < MW; ++w) {
            u64 a = me[w], o = took[w];  // (a lane without a member holds the neutral values)
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                a &= (u64)__shfl_xor((unsigned long long)a, d, 64);
                o |= (u64)__shfl_xor((unsigned long long)o, d, 64);
            }
            if ((int)(threadIdx.x & 63) == leader) {
                atomicAnd((unsigned long long*)&and_me[(size_t)first * MW + w], (unsigned long long)a);
                if (o) atomicOr((unsigned long long*)&or_took[(size_t)first * MW + w], (unsigned long long)o);
            }
        }
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&size[first], (u32)__popcll(active));
    } else if (root != ~0u) {
#pragma unroll
        for (int w = 0; w < MW; ++w) {
            atomicAnd((unsigned long long*)&and_me[(size_t)root * MW + w], (unsigned long long)me[w]);
            if (took[w]) atomicOr((unsigned long long*)&or_took[(size_t)root * MW + w], (unsigned long long)took[w]);
        }
        atomicAdd(&size[root], 1u);
    }
}

// list: the NP list. rank holds 0 for the sinks (live_index) and ~0 elsewhere. next takes the states of F_p'
// without a rank.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_goal(const u32* __restrict__ list, u32 n, const u64* __restrict__ slot_of,
                                                        const u32* alive, const u32* __restrict__ comp, const u32* __restrict__ size,
                                                        const u64* __restrict__ and_me, const u64* __restrict__ or_took, u32* rank,
                                                        u32* __restrict__ next, LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool todo = false, goal = false, is_comp = false, is_fair = false;
    u32 i = 0;
    if (g < n) {
        i = list[g];
        if (live_bit(alive, slot_of[i])) {
            goal = rank[i] == 0;
            const u32 root = comp[i];
            if (!goal && root != ~0u && size[root] >= 2) {
                const bool fair = live_fair_masks<M::MW>(&and_me[(size_t)root * M::MW], &or_took[(size_t)root * M::MW]);
                is_comp = root == i;
                is_fair = is_comp && fair;
                if (fair) rank[i] = 0, goal = true;
            }
            todo = !goal;
        }
    }
    live_append(todo, i, next, &lc->next_n);
    const u64 gm = __ballot(goal), cm = __ballot(is_comp), fm = __ballot(is_fair);
    if ((threadIdx.x & 63) == 0) {
        if (gm) atomicAdd(&lc->goal, (u32)__popcll(gm));
        if (cm) atomicAdd(&lc->comps, (u32)__popcll(cm));
        if (fm) atomicAdd(&lc->fair_comps, (u32)__popcll(fm));
    }
}

// One level: a listed state (rank ~0) with a moving successor of rank < round takes rank `round`; the
// others go to next.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_reach(M m, const u64* __restrict__ arena, TableView t,
                                                         const u32* __restrict__ idx, u32* rank, u32 round,
                                                         const u32* __restrict__ wl, u32 n, u32* __restrict__ next,
                                                         LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool keep = false, join = false;
    u32 i = 0;
    if (g < n) {
        i = wl[g];
        u64 s[M::W], me[M::MW];
        load_state<M::W>(arena, i, s);
        bool lost = false;
        live_moving(m, s, me, [&](int, const u64* ns) {
            if (join) return;
            const u32 ti = live_idx_of(m, t, idx, ns, lost);
            join = ti != ~0u && live_load(&rank[ti]) < round;
        });
        if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
        if (join) live_store(&rank[i], round);
        keep = !join;
    }
    live_append(keep, i, next, &lc->next_n);
    const u64 jm = __ballot(join);
    if (jm && (int)(threadIdx.x & 63) == __builtin_ctzll(jm)) atomicAdd(&lc->joined, (u32)__popcll(jm));
}

// list: the NP list; out takes the members of the component `root`.
template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_members(const u32* __restrict__ list, u32 n, const u32* __restrict__ comp, u32 root,
                                                           u32* __restrict__ out, LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    const bool in = g < n && comp[list[g]] == root;
    live_append(in, in ? list[g] : 0u, out, &lc->next_n);
}

// The target set of a loop segment inside the component `root` (members: its list): plan LIVE_PLAN_NOTME the
// members with !me(., a); LIVE_PLAN_TAKE those with me(., a) whose a-step stays in the component;
// LIVE_PLAN_HOME the state `home`. A target gets rank 0 (lc->joined counts them), every other member ~0
// and a place in next.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_targets(M m, const u64* __restrict__ arena, TableView t,
                                                           const u32* __restrict__ idx, const u32* __restrict__ comp, u32 root,
                                                           int plan, int a, u32 home, const u32* __restrict__ members, u32 n,
                                                           u32* rank, u32* __restrict__ next, LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool hit = false, keep = false;
    u32 i = 0;
    if (g < n) {
        i = members[g];
        if (plan == LIVE_PLAN_HOME) {
            hit = i == home;
        } else {
            u64 s[M::W], me[M::MW];
            load_state<M::W>(arena, i, s);
            bool lost = false, stays = false;
            live_moving(m, s, me, [&](int b, const u64* ns) {
                if (b != a || plan != LIVE_PLAN_TAKE) return;
                const u32 ti = live_idx_of(m, t, idx, ns, lost);
                stays = ti != ~0u && comp[ti] == root;
            });
            if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
            const bool mv = me[a >> 6] >> (a & 63) & 1;
            hit = plan == LIVE_PLAN_NOTME ? !mv : stays;
        }
        rank[i] = hit ? 0u : ~0u;
        keep = !hit;
    }
    live_append(keep, i, next, &lc->next_n);
    const u64 hm = __ballot(hit);
    if (hm && (int)(threadIdx.x & 63) == __builtin_ctzll(hm)) atomicAdd(&lc->joined, (u32)__popcll(hm));
}

// The lowest i < k whose init state has a rank, into lc->first_init (~0 before the launch). One workgroup.
template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_first_ranked(const u64* __restrict__ slot_of, const u32* __restrict__ idx,
                                                                const u32* __restrict__ rank, u32 k, LiveWeakCounters* lc) {
    for (u32 i = threadIdx.x; i < k; i += LIVE_BLOCK) {
        const u32 j = idx[slot_of[k - 1 - i]];
        if (j != ~0u && rank[j] != ~0u) atomicMin(&lc->first_init, i);
    }
}

// One wave. out holds max_steps + 2 states: out[0] is the state to go on from, state k + 1 the one step k
// reached. From a state of rank r > 0 the wave takes the lowest slot whose moving successor has a rank
// below r; at rank 0 it takes slot `then` if that is >= 0 and stops (LIVE_DESCEND_DONE). After max_steps
// steps it stops with LIVE_DESCEND_MORE and the host launches it again from the last state. all = 1 (a
// loop segment): every state passed adds the slots it does not move on to lc->notme and every step its
// slot to lc->taken; all = 0 (the stem): only the state of rank 0 adds to lc->notme.
template <class M>
__global__ void __launch_bounds__(64) live_descend(M m, TableView t, const u32* __restrict__ idx, const u32* __restrict__ rank,
                                                   u64* out, u32 max_steps, int then, u32 all, LiveWeakCounters* lc) {
    constexpr int W = M::W, MW = M::MW;
    const u32 lane = threadIdx.x;
    u64 cur[W], notme[MW], taken[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) notme[w] = taken[w] = 0;
    load_state<W>(out, 0, cur);
    u32 err = 0, k = 0, end = LIVE_DESCEND_MORE, ci = ~0u;
    auto wave_me = [&](u64* me) {  // the lanes' shares of the me mask, joined
#pragma unroll
        for (int w = 0; w < MW; ++w)
#pragma unroll
            for (int d = 32; d; d >>= 1) me[w] |= (u64)__shfl_xor((unsigned long long)me[w], d, 64);
    };
    while (!err) {  // (every condition below is wave-uniform)
        bool lost = false;
        ci = live_idx_of(m, t, idx, cur, lost);
        const u32 r = ci == ~0u ? ~0u : rank[ci];
        if (lost || r == ~0u) {
            err |= lost ? LIVE_ERR_LOOKUP : LIVE_ERR_STUCK;
            break;
        }
        if (r && k >= max_steps) break;
        u64 me[MW], nx[W];
        const int a = live_descend_step(
            m, cur, r,
            [&](const u64* ns) {
                const u32 ti = live_idx_of(m, t, idx, ns, lost);
                return ti == ~0u ? ~0u : rank[ti];
            },
            me, nx, lane, 64u);
        if (__ballot(lost)) {
            err |= LIVE_ERR_LOOKUP;
            break;
        }
        wave_me(me);
        if (all || !r)
#pragma unroll
            for (int w = 0; w < MW; ++w) notme[w] |= ~me[w];
        if (!r) {
            end = LIVE_DESCEND_DONE;
            if (then >= 0) {  // (every lane computes the same step)
                if (!m.apply(cur, then, nx)) {
                    err |= LIVE_ERR_STUCK;
                    break;
                }
#pragma unroll
                for (int x = 0; x < W; ++x) cur[x] = nx[x];
                ++k;
                if (lane == 0) store_state<W>(out, k, cur);
                taken[then >> 6] |= 1ull << (then & 63);
                ci = live_idx_of(m, t, idx, cur, lost);
                if (lost || ci == ~0u) {
                    err |= LIVE_ERR_LOOKUP;
                    break;
                }
                live_moving(m, cur, me, [](int, const u64*) {}, lane, 64u);
                wave_me(me);
#pragma unroll
                for (int w = 0; w < MW; ++w) notme[w] |= ~me[w];
            }
            break;
        }
        int best = a >= 0 ? a : 0x7fffffff;
#pragma unroll
        for (int o = 32; o; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        if (best == 0x7fffffff) {
            err |= LIVE_ERR_STUCK;
            break;
        }
        const int winner = __builtin_ctzll(__ballot(a == best));
#pragma unroll
        for (int x = 0; x < W; ++x) cur[x] = (u64)__shfl((unsigned long long)nx[x], winner, 64);
        ++k;
        if (lane == 0) store_state<W>(out, k, cur);
        if (all) taken[best >> 6] |= 1ull << (best & 63);
    }
    if (lane == 0) {
        lc->steps = k;
        lc->end = end;
        lc->last_idx = ci;
        if (err) atomicOr(&lc->err, err);
#pragma unroll
        for (int w = 0; w < MW; ++w) lc->notme[w] |= notme[w], lc->taken[w] |= taken[w];
    }
}

// ---- strong fairness (live.hpp: STRONG FAIRNESS). Launched only with sr_opts.liveness = SR_LIVENESS_STRONG,
// after live_mark and the progress trim, in place of the weak mode's pass and over the same arrays. The
// decomposition tree is built LEVEL BY LEVEL, all open components at once: W (a bitmap and a list) starts as
// the weak mode's U; one level takes the components of G'[W] with the kernels above (colour, seed, join,
// leave), accumulates per component, and refines:
//   live_level_open     per member of the level: the accumulators at its index cleared. A root is the highest
//                       arena index of its component and a member of its level, and the same index can be a
//                       root again at a deeper level, so the accumulators are reset per level.
//   live_comp_acc_or    live_comp_acc with the OR of the me masks in place of their AND (the in-wave reduction
//                       as it is there). comp holds a number only for the members of THIS level and for frozen
//                       states (live_refine clears every other), and a frozen component's root never returns
//                       to W, so `comp[t] == root` is membership in the component of this level.
//   live_refine         per member of the level, with bad = or_me & ~or_took of its component: in a component
//                       of one state it leaves for good; in a fair node (bad empty) it is FROZEN, keeping its
//                       component number for the goal set and the witness, and never returns to W; with
//                       me(s) & bad != 0 it leaves for good; every other member returns to W (its bit set, a
//                       place in next) with its number cleared. Roots count the nodes and the fair nodes.
//   live_goal_strong    sinks (rank 0 from live_index) and frozen states get rank 0; the other states of F_p'
//                       are listed for live_reach.
// The witness runs on live_reach, live_first_ranked, live_members, live_targets (LIVE_PLAN_TAKE and
// LIVE_PLAN_HOME only) and live_descend as they are.

template <int MW>
__global__ void __launch_bounds__(LIVE_BLOCK) live_level_open(const u32* __restrict__ list, u32 n, u32* __restrict__ size,
                                                              u64* __restrict__ or_me, u64* __restrict__ or_took) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    if (g >= n) return;
    const u32 i = list[g];
    size[i] = 0;
#pragma unroll
    for (int w = 0; w < MW; ++w) or_me[(size_t)i * MW + w] = or_took[(size_t)i * MW + w] = 0;
}

// or_me, or_took and size (zero before the launch: live_level_open) are by root.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_comp_acc_or(M m, const u64* __restrict__ arena, TableView t,
                                                               const u32* __restrict__ idx, const u32* __restrict__ comp,
                                                               const u32* __restrict__ list, u32 n, u32* size, u64* or_me,
                                                               u64* or_took, LiveWeakCounters* lc) {
    constexpr int MW = M::MW;
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    u32 root = ~0u;
    u64 me[MW], took[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) me[w] = took[w] = 0;
    if (g < n) {
        const u32 i = list[g];
        root = comp[i];
        if (root != ~0u) {
            u64 s[M::W];
            load_state<M::W>(arena, i, s);
            bool lost = false;
            live_moving(m, s, me, [&](int a, const u64* ns) {
                const u32 ti = live_idx_of(m, t, idx, ns, lost);
                if (ti != ~0u && comp[ti] == root) took[a >> 6] |= 1ull << (a & 63);
            });
            if (lost) atomicOr(&lc->err, (u32)LIVE_ERR_LOOKUP);
        }
    }
    const u64 active = __ballot(root != ~0u);
    if (!active) return;
    const int leader = __builtin_ctzll(active);
    const u32 first = lane_u32(root, (u32)leader);
    if (!__ballot(root != ~0u && root != first)) {  // the wave's members share one component
#pragma unroll
        for (int w = 0; w < MW; ++w) {
            u64 e = me[w], o = took[w];  // (a lane without a member holds the neutral values)
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                e |= (u64)__shfl_xor((unsigned long long)e, d, 64);
                o |= (u64)__shfl_xor((unsigned long long)o, d, 64);
            }
            if ((int)(threadIdx.x & 63) == leader) {
                if (e) atomicOr((unsigned long long*)&or_me[(size_t)first * MW + w], (unsigned long long)e);
                if (o) atomicOr((unsigned long long*)&or_took[(size_t)first * MW + w], (unsigned long long)o);
            }
        }
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&size[first], (u32)__popcll(active));
    } else if (root != ~0u) {
#pragma unroll
        for (int w = 0; w < MW; ++w) {
            if (me[w]) atomicOr((unsigned long long*)&or_me[(size_t)root * MW + w], (unsigned long long)me[w]);
            if (took[w]) atomicOr((unsigned long long*)&or_took[(size_t)root * MW + w], (unsigned long long)took[w]);
        }
        atomicAdd(&size[root], 1u);
    }
}

// list: the members of the level (every one has a component number). next takes the members that return to W
// (a subset of list); lc->joined counts the members frozen in fair nodes, lc->comps and lc->fair_comps the
// level's nodes and fair nodes.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) live_refine(M m, const u64* __restrict__ arena, const u64* __restrict__ slot_of,
                                                          const u32* __restrict__ list, u32 n, u32* __restrict__ comp,
                                                          const u32* __restrict__ size, const u64* __restrict__ or_me,
                                                          const u64* __restrict__ or_took, u32* w_bits, u32* __restrict__ next,
                                                          LiveWeakCounters* lc) {
    constexpr int MW = M::MW;
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool back = false, frozen = false, is_comp = false, is_fair = false, orphan = false;
    u32 i = 0;
    if (g < n) {
        i = list[g];
        const u32 root = comp[i];
        orphan = root == ~0u;
        if (!orphan && size[root] >= 2) {
            const u64 *om = &or_me[(size_t)root * MW], *ot = &or_took[(size_t)root * MW];
            frozen = live_strong_masks<MW>(om, ot);
            is_comp = root == i;
            is_fair = is_comp && frozen;
            if (!frozen) {
                u64 s[M::W], me[MW];
                load_state<M::W>(arena, i, s);
                live_moving(m, s, me, [](int, const u64*) {});
                bool hit = false;
#pragma unroll
                for (int w = 0; w < MW; ++w) hit = hit || (me[w] & om[w] & ~ot[w]) != 0;
                back = !hit;
            }
        }
        if (!frozen) comp[i] = ~0u;
        if (back) {
            const u64 sl = slot_of[i];
            atomicOr(&w_bits[sl >> 5], 1u << (sl & 31));
        }
    }
    live_append(back, i, next, &lc->next_n);
    const u64 zm = __ballot(frozen), cm = __ballot(is_comp), fm = __ballot(is_fair);
    if ((threadIdx.x & 63) == 0) {
        if (zm) atomicAdd(&lc->joined, (u32)__popcll(zm));
        if (cm) atomicAdd(&lc->comps, (u32)__popcll(cm));
        if (fm) atomicAdd(&lc->fair_comps, (u32)__popcll(fm));
    }
    if (__ballot(orphan) && (threadIdx.x & 63) == 0) atomicOr(&lc->err, (u32)LIVE_ERR_STUCK);
}

// list: the NP list. rank holds 0 for the sinks (live_index) and ~0 elsewhere; comp a number for the frozen
// states only. next takes the states of F_p' without a rank; lc->goal counts the goal set.
template <int = 0>
__global__ void __launch_bounds__(LIVE_BLOCK) live_goal_strong(const u32* __restrict__ list, u32 n, const u64* __restrict__ slot_of,
                                                               const u32* alive, const u32* __restrict__ comp, u32* rank,
                                                               u32* __restrict__ next, LiveWeakCounters* lc) {
    const u32 g = blockIdx.x * LIVE_BLOCK + threadIdx.x;
    bool todo = false, goal = false;
    u32 i = 0;
    if (g < n) {
        i = list[g];
        if (live_bit(alive, slot_of[i])) {
            goal = rank[i] == 0;
            if (!goal && comp[i] != ~0u) rank[i] = 0, goal = true;
            todo = !goal;
        }
    }
    live_append(todo, i, next, &lc->next_n);
    const u64 gm = __ballot(goal);
    if (gm && (threadIdx.x & 63) == 0) atomicAdd(&lc->goal, (u32)__popcll(gm));
}

// ---- leads-to (live.hpp: LEADS-TO). Launched only for a leads-to property, in every mode, behind the mode's
// own stages for the condition Q (live_mark and the trim; in a fair mode also the components and the ranks),
// in place of live_first_init / live_first_ranked, which stay the kernels they are. RANKED says how "s is in
// X_Q" is answered: false, the alive bit at the state's slot (F_p, F_p'); true, a rank at the arena index that
// the slot maps to (FairF). Neither kernel probes the visited set: a state's slot is live_mark's slot_of.
//   live_leads_scan  per arena state: the trigger, the condition and the membership test (live_leads_class). A
//                    lane strides over the arena (a grid of at most LIVE_LEADS_GRID workgroups) and keeps its
//                    three counts and its lowest violating arena index in registers; at its end a wave reduces
//                    them by shuffles and issues one atomic per counter that is not zero, and one atomicMin. All
//                    waves add to the same four words, and atomics on one address are served one after the
//                    other: with one lane per state (209 K waves on 13.4 M states) they were 5.1-6.7 ms of a
//                    stage whose reads take a tenth of that (profiles/leads_pass.txt). Level 0 of the arena
//                    holds the init states as given, duplicates too: of equal init states (equal slots) only
//                    the one of lowest arena index counts.
//   live_leads_min   one lane per state of ONE level (the level of that lowest index, which the host reads off
//                    its level offsets): round j < W takes the minimum of word j over the violating states that
//                    match the seed's words fixed so far (a wave-level reduction, then one 64-bit atomicMin per
//                    wave); for one-word states that is one round. Round j = W takes the lowest arena index of
//                    the state that matches all W words (equal init states: any of them has the same path).

constexpr u32 LIVE_LEADS_GRID = 2048;  // workgroups of live_leads_scan at most (8 per CU)

struct LiveLeadsCounters {
    u32 triggered, pending, violating;
    u32 min_idx;  // the lowest arena index of a violating state (~0 before the launch)
};

template <bool RANKED>
__device__ __forceinline__ bool live_in_x(u64 slot, const u32* alive, const u32* __restrict__ idx, const u32* __restrict__ rank) {
    if constexpr (RANKED) {
        const u32 j = idx[slot];
        return j != ~0u && rank[j] != ~0u;
    } else {
        return live_bit(alive, slot);
    }
}

// k: the init states (level 0 is the arena's first k states).
template <class M, bool RANKED>
__global__ void __launch_bounds__(LIVE_BLOCK) live_leads_scan(M m, const u64* __restrict__ arena, u32 n, u32 k, int p,
                                                              const u64* __restrict__ slot_of, const u32* alive,
                                                              const u32* __restrict__ idx, const u32* __restrict__ rank,
                                                              LiveLeadsCounters* lc) {
    u32 nt = 0, np = 0, nv = 0, lowest = ~0u;
    for (u64 g = blockIdx.x * LIVE_BLOCK + threadIdx.x; g < n; g += (u64)gridDim.x * LIVE_BLOCK) {  // (64 bits: n may be near 2^32)
        const u32 i = (u32)g;
        const u64 sl = slot_of[i];
        bool dup = false;
        if (i < k)
            for (u32 j = 0; j < i; ++j) dup = dup || slot_of[j] == sl;
        if (dup) continue;
        u64 s[M::W];
        load_state<M::W>(arena, i, s);
        const u32 c = live_leads_class(m, p, s, [&] { return live_in_x<RANKED>(sl, alive, idx, rank); });
        nt += c & LIVE_LEADS_TRIGGERED ? 1u : 0u;
        np += c & LIVE_LEADS_PENDING ? 1u : 0u;
        if (c & LIVE_LEADS_VIOLATING) nv += 1, lowest = min(lowest, i);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {  // (every lane is back here: the loop's trip counts differ by one at most)
        nt += __shfl_xor(nt, d, 64);
        np += __shfl_xor(np, d, 64);
        nv += __shfl_xor(nv, d, 64);
        lowest = min(lowest, (u32)__shfl_xor(lowest, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (nt) atomicAdd(&lc->triggered, nt);
        if (np) atomicAdd(&lc->pending, np);
        if (nv) atomicAdd(&lc->violating, nv), atomicMin(&lc->min_idx, lowest);
    }
}

// The states lo .. hi - 1 of the arena (one level). seed: W words, all ones before round 0; seed_idx: ~0 before
// round W.
template <class M, bool RANKED>
__global__ void __launch_bounds__(LIVE_BLOCK) live_leads_min(M m, const u64* __restrict__ arena, u32 lo, u32 hi, int p,
                                                             const u64* __restrict__ slot_of, const u32* alive,
                                                             const u32* __restrict__ idx, const u32* __restrict__ rank, int j,
                                                             u64* seed, u32* seed_idx) {
    constexpr int W = M::W;
    const u64 g = (u64)lo + (u64)blockIdx.x * LIVE_BLOCK + threadIdx.x;  // (64 bits: hi may be near 2^32)
    const u32 i = (u32)g;
    bool cand = false;
    u64 s[W];
#pragma unroll
    for (int x = 0; x < W; ++x) s[x] = ~0ull;
    if (g < hi) {
        load_state<W>(arena, i, s);
        const u64 sl = slot_of[i];
        cand = (live_leads_class(m, p, s, [&] { return live_in_x<RANKED>(sl, alive, idx, rank); }) & LIVE_LEADS_VIOLATING) != 0;
#pragma unroll
        for (int x = 0; x < W; ++x)
            if (x < j) cand = cand && s[x] == seed[x];
    }
    const u64 cm = __ballot(cand);
    if (!cm) return;
    if (j >= W) {
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(cm)) atomicMin(seed_idx, i);
        return;
    }
    u64 v = ~0ull;
#pragma unroll
    for (int x = 0; x < W; ++x)  // (no dynamic index: the state stays in registers)
        if (x == j && cand) v = s[x];
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u64 o = (u64)__shfl_xor((unsigned long long)v, d, 64);
        v = o < v ? o : v;
    }
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(cm)) atomicMin((unsigned long long*)&seed[j], (unsigned long long)v);
}

}  // namespace sr
