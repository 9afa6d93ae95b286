// The kernels of the certificate pass (gfx950), over the definitions in certify.hpp (this header is included
// from there). They run after a search, on what it left behind: the arena, its level offsets, the parent
// ranks, the final visited set and, in FIFO order, its meta words. They call the model's `enabled`, `apply`
// and `discovers`, and load_state, probe_key and find_slot, and nothing else of the search: no stage, no
// duplicate filter, no action table, no enabled_moves / self_loops, no find_or_claim.
//
// Every kernel is a persistent grid of CERT_BLOCK lanes per workgroup that strides over arena indices with
// 64 bits, one lane per state. A lane keeps its counts in registers for the whole launch; at its end a wave
// reduces them by shuffles and issues one 64-bit atomic per value that is not zero (step_scan's lesson,
// kernels_step.hpp). Where successors are generated (cert_tree, cert_closure) the lanes of a wave walk the
// UNION of their enabled slots in lockstep, so `apply` runs with a wave-uniform slot; a lane's slots are not
// taken in increasing order by that walk, so "the first slot" is kept as a running minimum.
//
//   cert_roots    arena index i < k against the expected level 0 (a host copy, in arena order)
//   cert_map      every state writes its level into lvl[its slot] (atomicMin: repeated init states share one)
//   cert_tree     levels >= 1: the parent rank is in range (compared BEFORE any load), the parent generates the
//                 state, and in FIFO order the slot's tag names the parent's rank and its first such slot
//   cert_closure  every successor of every state is in the table, listed, and at most one level down; in FIFO
//                 order no earlier generator exists than the one recorded
//   cert_order    FIFO order: neighbours of a level have strictly increasing tags
//   cert_props    per property: the states it is discovered at, the lowest such index, and whether it is at
//                 the engine's own discovery index
#pragma once

namespace sr {

constexpr u32 CERT_BLOCK = 256;
constexpr int CERT_MAX_PROPS = 32;
constexpr u64 CERT_TAG_MASK = (1ull << META_SHIFT) - 1;
constexpr u32 CERT_UNLISTED = 0xffffffffu;  // lvl[slot] before cert_map

// The global words of a pass, 64 bits each (zero before it, the CERT_FIRST ones all ones).
enum CertWord : size_t {
    CERT_ROOTS_WRONG, CERT_MAP_MISSING, CERT_TREE_RANGE, CERT_TREE_EDGE, CERT_TREE_SLOT, CERT_EDGES, CERT_REP_EDGES,
    CERT_CL_MISSING, CERT_CL_UNLISTED, CERT_CL_LATE, CERT_NOT_FIRST, CERT_ORDER,
    CERT_HOLDS,
    CERT_DISC_WRONG = CERT_HOLDS + CERT_MAX_PROPS,
    CERT_FIRST = CERT_DISC_WRONG + CERT_MAX_PROPS,
    CERT_WORDS = CERT_FIRST + CERT_MAX_PROPS
};

struct CertDisc {
    u64 at[CERT_MAX_PROPS];  // the engine's discovery index per property (all ones: none)
};

__device__ __forceinline__ u64 cert_wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}
__device__ __forceinline__ u64 cert_wave_min(u64 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u64 o = (u64)__shfl_xor((unsigned long long)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 cert_lane_u64(u64 v, u32 lane) { return (u64)__shfl((unsigned long long)v, (int)lane, 64); }
// (called by every lane of a wave, at the end of a launch)
__device__ __forceinline__ void cert_add(u64* g, size_t w, u64 v) {
    v = cert_wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(g + w), (unsigned long long)v);
}
// The level L with lstart[L] <= i < lstart[L + 1] (i < lstart[nlevels]).
__device__ __forceinline__ u32 cert_level(const u64* __restrict__ lstart, u32 nlevels, u64 i) {
    u32 lo = 0, hi = nlevels;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) / 2;
        (lstart[mid] <= i ? lo : hi) = mid;
    }
    return lo;
}
template <int W>
__device__ __forceinline__ bool cert_same(const u64* a, const u64* b) {
    bool eq = true;
#pragma unroll
    for (int x = 0; x < W; ++x) eq = eq && a[x] == b[x];
    return eq;
}

// f(a, out) for every enabled slot a of s whose apply succeeds, on the lanes with `live`; every lane of the
// wave calls this (the loop's conditions are wave-uniform).
template <class M, class F>
__device__ __forceinline__ void cert_walk(const M& m, bool live, const u64* s, F&& f) {
    constexpr int W = M::W, MW = M::MW;
    u64 mask[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) mask[w] = 0;
    if (live) m.enabled(s, mask);
    for (int w = 0; w < MW; ++w) {
        u64 bits = mask[w];
        for (;;) {
            const u64 pend = __ballot(bits != 0);
            if (!pend) break;
            const u32 first = (u32)__builtin_ctzll(pend);
            const int b = __builtin_ctzll(cert_lane_u64(bits, first));
            const bool en = (bits >> b & 1) != 0;
            bits &= ~(1ull << b);
            u64 out[W];
            if (en && m.apply(s, w * 64 + b, out)) f(w * 64 + b, out);
        }
    }
}

// want: k states, in arena order.
template <class M>
__global__ void __launch_bounds__(CERT_BLOCK) cert_roots(const u64* __restrict__ arena, const u64* __restrict__ want, u64 k, u64* __restrict__ g) {
    constexpr int W = M::W;
    u64 wrong = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = (u64)blockIdx.x * CERT_BLOCK; base < k; base += stride) {
        const u64 i = base + threadIdx.x;
        if (i < k) {
            u64 s[W], q[W];
            load_state<W>(arena, i, s);
            load_state<W>(want, i, q);
            wrong += cert_same<W>(s, q) ? 0 : 1;
        }
    }
    cert_add(g, CERT_ROOTS_WRONG, wrong);
}

// lvl: one word per slot, CERT_UNLISTED before the launch.
template <class M>
__global__ void __launch_bounds__(CERT_BLOCK) cert_map(M m, TableView t, const u64* __restrict__ arena, u64 n, const u64* __restrict__ lstart,
                                                       u32 nlevels, u32* __restrict__ lvl, u64* __restrict__ g) {
    constexpr int W = M::W;
    u64 missing = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = (u64)blockIdx.x * CERT_BLOCK; base < n; base += stride) {
        const u64 i = base + threadIdx.x;
        if (i < n) {
            u64 s[W];
            load_state<W>(arena, i, s);
            const u64 slot = find_slot(t, probe_key(m, t, s));
            if (slot == ~0ull) missing += 1;
            else atomicMin(&lvl[slot], cert_level(lstart, nlevels, i));
        }
    }
    cert_add(g, CERT_MAP_MISSING, missing);
}

// The states lstart[1] .. n - 1. A: the model's max_actions (FIFO only).
template <class M, bool FIFO>
__global__ void __launch_bounds__(CERT_BLOCK) cert_tree(M m, TableView t, const u64* __restrict__ arena, const u32* __restrict__ apar, u64 n,
                                                        const u64* __restrict__ lstart, u32 nlevels, u32 A, u64* __restrict__ g) {
    constexpr int W = M::W;
    u64 c_range = 0, c_edge = 0, c_slot = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = lstart[1] + (u64)blockIdx.x * CERT_BLOCK; base < n; base += stride) {  // (uniform over the workgroup)
        const u64 i = base + threadIdx.x;
        u64 s[W], par[W];
        u32 p = 0;
        bool walk = false;
        if (i < n) {
            const u32 d = cert_level(lstart, nlevels, i);  // >= 1
            p = apar[i];
            if ((u64)p >= lstart[d] - lstart[d - 1]) {
                c_range += 1;  // counted, never dereferenced
            } else {
                load_state<W>(arena, lstart[d - 1] + p, par);
                load_state<W>(arena, i, s);
                walk = true;
            }
        }
        u32 best = ~0u;
        cert_walk(m, walk, par, [&](int a, const u64* out) {
            if (cert_same<W>(out, s) && (u32)a < best) best = (u32)a;
        });
        if (walk) {
            if (best == ~0u) {
                c_edge += 1;
            } else if (FIFO) {
                const u64 slot = find_slot(t, probe_key(m, t, s));
                if (slot != ~0ull && (t.meta[slot] & CERT_TAG_MASK) != (u64)p * A + best) c_slot += 1;
            }
        }
    }
    cert_add(g, CERT_TREE_RANGE, c_range);
    cert_add(g, CERT_TREE_EDGE, c_edge);
    if (FIFO) cert_add(g, CERT_TREE_SLOT, c_slot);
}

// skip: one bit per arena index below k0, the indices that repeat another init state (k0 = 0: not read).
template <class M, bool FIFO>
__global__ void __launch_bounds__(CERT_BLOCK) cert_closure(M m, TableView t, const u64* __restrict__ arena, u64 n, const u64* __restrict__ lstart,
                                                           u32 nlevels, const u32* __restrict__ skip, u32 k0, u32 A,
                                                           const u32* __restrict__ lvl, u64* __restrict__ g) {
    constexpr int W = M::W;
    u64 edges = 0, rep = 0, c_missing = 0, c_unlisted = 0, c_late = 0, c_first = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = (u64)blockIdx.x * CERT_BLOCK; base < n; base += stride) {
        const u64 i = base + threadIdx.x;
        const bool live = i < n;
        bool repeated = false;
        u64 s[W], rank = 0;
        u32 d = 0;
        if (live) {
            if (i < (u64)k0) repeated = (skip[i >> 5] >> (i & 31) & 1) != 0;
            load_state<W>(arena, i, s);
            d = cert_level(lstart, nlevels, i);
            rank = i - lstart[d];
        }
        cert_walk(m, live, s, [&](int a, const u64* out) {
            if (repeated) {
                rep += 1;
                return;
            }
            edges += 1;
            const u64 slot = find_slot(t, probe_key(m, t, out));
            if (slot == ~0ull) {
                c_missing += 1;
                return;
            }
            const u32 L = lvl[slot];
            if (L == CERT_UNLISTED) c_unlisted += 1;
            else if (L > d + 1) c_late += 1;
            else if (FIFO && L == d + 1 && rank * A + (u64)a < (t.meta[slot] & CERT_TAG_MASK)) c_first += 1;
        });
    }
    cert_add(g, CERT_EDGES, edges);
    cert_add(g, CERT_REP_EDGES, rep);
    cert_add(g, CERT_CL_MISSING, c_missing);
    cert_add(g, CERT_CL_UNLISTED, c_unlisted);
    cert_add(g, CERT_CL_LATE, c_late);
    if (FIFO) cert_add(g, CERT_NOT_FIRST, c_first);
}

// FIFO order: the states lstart[1] .. n - 1 against their left neighbour in the same level. A state that the
// table does not hold has no tag: its pairs are not counted (cert_map counts the state).
template <class M>
__global__ void __launch_bounds__(CERT_BLOCK) cert_order(M m, TableView t, const u64* __restrict__ arena, u64 n, const u64* __restrict__ lstart,
                                                         u32 nlevels, u64* __restrict__ g) {
    constexpr int W = M::W;
    u64 bad = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = lstart[1] + (u64)blockIdx.x * CERT_BLOCK; base < n; base += stride) {
        const u64 i = base + threadIdx.x;
        if (i < n && i > lstart[cert_level(lstart, nlevels, i)]) {
            u64 s[W], q[W];
            load_state<W>(arena, i, s);
            load_state<W>(arena, i - 1, q);
            const u64 a = find_slot(t, probe_key(m, t, s)), b = find_slot(t, probe_key(m, t, q));
            if (a != ~0ull && b != ~0ull && !((t.meta[b] & CERT_TAG_MASK) < (t.meta[a] & CERT_TAG_MASK))) bad += 1;
        }
    }
    cert_add(g, CERT_ORDER, bad);
}

// pmask: the properties to count (bits below M::NPROPS).
template <class M>
__global__ void __launch_bounds__(CERT_BLOCK) cert_props(M m, const u64* __restrict__ arena, u64 n, u32 pmask, CertDisc disc, u64* __restrict__ g) {
    constexpr int W = M::W, NP = M::NPROPS > 0 ? M::NPROPS : 1;
    static_assert(M::NPROPS <= CERT_MAX_PROPS, "the property counters");
    u64 holds[NP], low[NP], wrong[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) holds[p] = 0, low[p] = ~0ull, wrong[p] = 0;
    const u64 stride = (u64)gridDim.x * CERT_BLOCK;
    for (u64 base = (u64)blockIdx.x * CERT_BLOCK; base < n; base += stride) {
        const u64 i = base + threadIdx.x;
        if (i < n) {
            u64 s[W];
            load_state<W>(arena, i, s);
#pragma unroll
            for (int p = 0; p < M::NPROPS; ++p) {
                if (!(pmask >> p & 1)) continue;
                const bool h = m.discovers(p, s);
                if (h) holds[p] += 1, low[p] = i < low[p] ? i : low[p];
                if (!h && disc.at[p] == i) wrong[p] += 1;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < M::NPROPS; ++p) {
        if (!(pmask >> p & 1)) continue;  // (uniform: a kernel argument)
        cert_add(g, CERT_HOLDS + p, holds[p]);
        cert_add(g, CERT_DISC_WRONG + p, wrong[p]);
        const u64 lo = cert_wave_min(low[p]);
        if ((threadIdx.x & 63) == 0 && lo != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(g + CERT_FIRST + p), (unsigned long long)lo);
    }
}

}  // namespace sr
