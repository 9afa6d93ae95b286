// The kernel of the coverage pass (gfx950), over the rule defined in cover.hpp (this header is included
// from there, after that definition). It runs after a search that explored everything, on its arena
// alone: one expansion of every state, no probe, no visited set.
//
//   cover_count  a persistent grid (resident workgroups per CU x CUs, at most one workgroup per
//                COVER_BLOCK states) strides over the arena with 64-bit indices, one lane per state. The
//                lanes of a wave walk the UNION of their enabled slots in lockstep: the lowest pending
//                slot of the first lane that has one is taken by every lane that has it, so `apply`
//                runs with a wave-uniform slot, and the three per-slot outcomes (enabled, taken, moved)
//                are three ballots. Where the class is the slot, one lane adds their popcounts to the
//                workgroup's LDS histograms: at most three LDS adds per slot per wave. With the model's
//                `cover_class` hook the lanes may disagree on the class; the lanes are then peeled by
//                class (the class of the first lane left, a ballot of the lanes that share it), one
//                round per distinct class among them (Increment: at most 2, paxos: at most 9).
//                Per state: out_degree and max_out_degree go to LDS with one atomic per lane; terminal,
//                stutter_ends and each property's condition are one ballot and one LDS add per wave.
//   flush        every `chunk` strides and at the end, each workgroup adds its LDS counters that are
//                not zero to the 64-bit global ones (vector atomics, one per class and workgroup) and
//                clears them. An LDS counter grows by at most COVER_BLOCK * 64 * MW per stride, and
//                the host bounds `chunk` so that it cannot wrap (cover_chunk_max).
// The first k0 arena indices are level 0, which holds the init states as given; the host hands a bit
// mask of the indices that repeat another init state, and those lanes count nothing.
#pragma once

namespace sr {

constexpr u32 COVER_BLOCK = 256;

// The global counters of a pass, 64 bits each: [3][classes] enabled, taken, moved; then COVER_DEGREES
// out-degree buckets; then 32 properties; then terminal, stutter_ends, max_out_degree and
// bad_class (slots whose class was outside [0, classes): counted nowhere else, an error of the model's hook).
SR_HD size_t cover_words(u32 classes) { return (size_t)3 * classes + COVER_DEGREES + 32 + 4; }

// Strides between two flushes at most: COVER_BLOCK states add at most 64 * MW each to one LDS counter.
template <class M>
constexpr u32 cover_chunk_max() {
    return (u32)(0xffffffffull / ((u64)COVER_BLOCK * 64 * M::MW));
}

struct CoverLds {
    u32 h[3][COVER_MAX_CLASSES];
    u32 deg[COVER_DEGREES];
    u32 props[32];
    u32 terminal, stutter, max_deg, bad;
};

__device__ __forceinline__ u64 cover_lane_u64(u64 v, u32 src) {
    return (u64)lane_u32((u32)v, src) | (u64)lane_u32((u32)(v >> 32), src) << 32;
}

__device__ __forceinline__ void cover_flush(CoverLds& L, u32 classes, u64* __restrict__ g) {
    using ull = unsigned long long;
    for (u32 k = 0; k < 3; ++k)
        for (u32 c = threadIdx.x; c < classes; c += COVER_BLOCK) {
            const u32 v = L.h[k][c];
            if (!v) continue;
            atomicAdd(reinterpret_cast<ull*>(g + (size_t)k * classes + c), (ull)v);
            L.h[k][c] = 0;
        }
    u64* tail = g + (size_t)3 * classes;
    if (threadIdx.x < (u32)COVER_DEGREES) {
        const u32 v = L.deg[threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<ull*>(tail + threadIdx.x), (ull)v);
        L.deg[threadIdx.x] = 0;
    } else if (threadIdx.x < (u32)COVER_DEGREES + 32) {
        const u32 p = threadIdx.x - COVER_DEGREES;
        const u32 v = L.props[p];
        if (v) atomicAdd(reinterpret_cast<ull*>(tail + COVER_DEGREES + p), (ull)v);
        L.props[p] = 0;
    } else if (threadIdx.x == (u32)COVER_DEGREES + 32) {
        u64* sc = tail + COVER_DEGREES + 32;
        if (L.terminal) atomicAdd(reinterpret_cast<ull*>(sc), (ull)L.terminal);
        if (L.stutter) atomicAdd(reinterpret_cast<ull*>(sc + 1), (ull)L.stutter);
        if (L.max_deg) atomicMax(reinterpret_cast<ull*>(sc + 2), (ull)L.max_deg);
        if (L.bad) atomicAdd(reinterpret_cast<ull*>(sc + 3), (ull)L.bad);
        L.terminal = L.stutter = L.max_deg = L.bad = 0;
    }
}

// g has cover_words(classes) words, zeroed; skip has (k0 + 31) / 32 words (k0 = 0: not read);
// 1 <= chunk <= cover_chunk_max<M>(); classes <= COVER_MAX_CLASSES.
template <class M>
__global__ void __launch_bounds__(COVER_BLOCK) cover_count(M m, const u64* __restrict__ arena, u64 n, const u32* __restrict__ skip,
                                                           u32 k0, u32 always, u32 classes, u32 chunk, u64* __restrict__ g) {
    constexpr int W = M::W, MW = M::MW;
    static_assert(M::NPROPS <= 32, "the property counters");
    __shared__ CoverLds L;
    for (u32 x = threadIdx.x; x < sizeof(CoverLds) / sizeof(u32); x += COVER_BLOCK) reinterpret_cast<u32*>(&L)[x] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const u64 stride = (u64)gridDim.x * COVER_BLOCK;
    u32 since = 0;
    for (u64 base = (u64)blockIdx.x * COVER_BLOCK; base < n; base += stride) {  // (base is uniform over the workgroup)
        const u64 i = base + threadIdx.x;
        bool live = i < n;
        if (live && i < (u64)k0) live = !(skip[i >> 5] >> (i & 31) & 1);
        u64 s[W], out[W], mask[MW];
#pragma unroll
        for (int w = 0; w < MW; ++w) mask[w] = 0;
        if (live) {
            load_state<W>(arena, i, s);
            m.enabled(s, mask);
        }
        u32 deg = 0, mdeg = 0;
        for (int w = 0; w < MW; ++w) {
            u64 bits = mask[w];
            for (;;) {  // (every condition of this loop is wave-uniform)
                const u64 pend = __ballot(bits != 0);
                if (!pend) break;
                const u32 first = (u32)__builtin_ctzll(pend);
                const int b = __builtin_ctzll(cover_lane_u64(bits, first));
                const int a = w * 64 + b;
                const bool en = (bits >> b & 1) != 0;
                bits &= ~(1ull << b);
                bool tk = false, mv = false;
                int c = a;
                if (en) {
                    c = cover_class_of(m, s, a);
                    tk = m.apply(s, a, out);
                    mv = tk && cover_moved<W>(s, out);
                    deg += tk;
                    mdeg += mv;
                }
                const u64 eb = __ballot(en), tb = __ballot(tk), mb = __ballot(mv);
                if constexpr (!cover_hook_model<M>) {
                    if (lane == first) {
                        if ((u32)a < classes) {
                            atomicAdd(&L.h[0][a], (u32)__popcll(eb));
                            if (tb) atomicAdd(&L.h[1][a], (u32)__popcll(tb));
                            if (mb) atomicAdd(&L.h[2][a], (u32)__popcll(mb));
                        } else {
                            atomicAdd(&L.bad, (u32)__popcll(eb));
                        }
                    }
                } else {
                    for (u64 rem = eb; rem;) {  // peel the lanes by class
                        const u32 head = (u32)__builtin_ctzll(rem);
                        const u32 hc = lane_u32((u32)c, head);
                        const u64 same = __ballot(en && (u32)c == hc);
                        if (lane == head) {
                            if (hc < classes) {
                                atomicAdd(&L.h[0][hc], (u32)__popcll(same));
                                if (same & tb) atomicAdd(&L.h[1][hc], (u32)__popcll(same & tb));
                                if (same & mb) atomicAdd(&L.h[2][hc], (u32)__popcll(same & mb));
                            } else {
                                atomicAdd(&L.bad, (u32)__popcll(same));
                            }
                        }
                        rem &= ~same;
                    }
                }
            }
        }
        u32 holds = 0;
        if (live) {
            holds = cover_conditions(m, always, s);
            atomicAdd(&L.deg[cover_bucket(deg)], 1u);
            if (deg) atomicMax(&L.max_deg, deg);
        }
        const u64 term = __ballot(live && deg == 0), stut = __ballot(live && deg > 0 && mdeg == 0);
        if (lane == 0) {
            if (term) atomicAdd(&L.terminal, (u32)__popcll(term));
            if (stut) atomicAdd(&L.stutter, (u32)__popcll(stut));
        }
#pragma unroll
        for (int p = 0; p < M::NPROPS; ++p) {
            const u64 hb = __ballot((holds >> p & 1) != 0);
            if (hb && lane == 0) atomicAdd(&L.props[p], (u32)__popcll(hb));
        }
        if (++since == chunk) {
            __syncthreads();
            cover_flush(L, classes, g);
            __syncthreads();
            since = 0;
        }
    }
    __syncthreads();
    cover_flush(L, classes, g);
}

}  // namespace sr
