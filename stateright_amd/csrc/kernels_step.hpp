// The kernels of the step pass (gfx950), over the rule defined in step.hpp (this header is included from
// there, after that definition). They run after a search that explored everything, on its arena alone: one
// expansion of every state, no probe, no visited set, as the coverage pass does (kernels_cover.hpp).
//
//   step_scan  a persistent grid (resident workgroups per CU x CUs, at most one workgroup per STEP_BLOCK
//              states) strides over the arena with 64-bit indices, one lane per state. The lanes of a wave
//              walk the UNION of their enabled slots in lockstep, as cover_count does: the lowest pending slot
//              of the first lane that has one is taken by every lane that has it, so `apply` and the model's
//              `step_holds` run with a wave-uniform slot. Every step property of the model is evaluated on
//              each taken edge. A lane keeps its edge count and, per step property, its violations, its
//              violating sources and its lowest violating arena index in registers for the whole launch; at
//              its end a wave reduces them by shuffles and issues one 64-bit atomic per value that is not
//              zero (and one atomicMin per property with a violation). All waves add to the same few words,
//              and atomics on one address are served one after the other (live_leads_scan's lesson: one
//              atomic per wave per stride cost several ms on 13 M states), so a wave issues them once per
//              launch: at most 1 + 3 per step property.
//   step_min   one lane per state of ONE level (the level of the lowest violating index of property p, which
//              the host reads off its level offsets). A lane whose state matches the seed's words fixed so far
//              expands it again, slot by slot, up to its first violating slot. Round j < W takes the minimum
//              of word j over those violating sources (a wave-level reduction, then one 64-bit atomicMin per
//              wave); round W takes, of the states equal to the seed's source, the lowest violating slot and
//              the lowest arena index (equal states have equal slots, so the two minima need one round).
// The first k0 arena indices are level 0, which holds the init states as given; the host hands the coverage
// pass' bit mask of the indices that repeat another init state, and those lanes count nothing in step_scan
// (step_min takes minima over states, which a repeated state does not change).
#pragma once

namespace sr {

constexpr u32 STEP_BLOCK = 256;
constexpr int STEP_MAX_PROPS = 32;

// The global words of a pass, 64 bits each: edges; then per property violations, sources and the lowest
// violating arena index (all ones before the launch).
constexpr size_t STEP_VIOL = 1, STEP_SRC = 1 + STEP_MAX_PROPS, STEP_LOW = 1 + 2 * STEP_MAX_PROPS, STEP_WORDS = 1 + 3 * STEP_MAX_PROPS;

__device__ __forceinline__ u64 step_wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}
__device__ __forceinline__ u64 step_wave_min(u64 v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u64 o = (u64)__shfl_xor((unsigned long long)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// g has STEP_WORDS words: zero, the STEP_LOW ones all ones; skip has (k0 + 31) / 32 words (k0 = 0: not read);
// smask: the model's step properties (bits below M::NPROPS).
template <class M>
__global__ void __launch_bounds__(STEP_BLOCK) step_scan(M m, const u64* __restrict__ arena, u64 n, const u32* __restrict__ skip, u32 k0,
                                                        u32 smask, u64* __restrict__ g) {
    constexpr int W = M::W, MW = M::MW, NP = M::NPROPS;
    static_assert(NP <= STEP_MAX_PROPS, "the property counters");
    using ull = unsigned long long;
    u64 edges = 0, viol[NP], src[NP], low[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) viol[p] = 0, src[p] = 0, low[p] = ~0ull;
    const u64 stride = (u64)gridDim.x * STEP_BLOCK;
    for (u64 base = (u64)blockIdx.x * STEP_BLOCK; base < n; base += stride) {  // (base is uniform over the workgroup)
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
        u32 bad = 0;
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
                if (en && m.apply(s, a, out)) {
                    edges += 1;
                    const u32 v = step_violated(m, smask, s, a, out);
                    bad |= v;
#pragma unroll
                    for (int p = 0; p < NP; ++p) viol[p] += v >> p & 1;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (bad >> p & 1) src[p] += 1, low[p] = i < low[p] ? i : low[p];
    }
    // (every lane is back here: the trip count of the loop above is uniform over the workgroup)
    const bool lead = (threadIdx.x & 63) == 0;
    edges = step_wave_sum(edges);
    if (lead && edges) atomicAdd(reinterpret_cast<ull*>(g), (ull)edges);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (!(smask >> p & 1)) continue;  // (uniform: a kernel argument)
        const u64 nv = step_wave_sum(viol[p]);
        if (!nv) continue;  // (uniform: the reduction leaves every lane the wave's sum)
        const u64 ns = step_wave_sum(src[p]), lo = step_wave_min(low[p]);
        if (lead) {
            atomicAdd(reinterpret_cast<ull*>(g + STEP_VIOL + p), (ull)nv);
            atomicAdd(reinterpret_cast<ull*>(g + STEP_SRC + p), (ull)ns);
            atomicMin(reinterpret_cast<ull*>(g + STEP_LOW + p), (ull)lo);
        }
    }
}

// The states lo .. hi - 1 of the arena (one level). seed: W + 2 words, all ones before round 0: the source's
// words, then its lowest violating slot and the lowest arena index of a state equal to it (both from round W).
template <class M>
__global__ void __launch_bounds__(STEP_BLOCK) step_min(M m, const u64* __restrict__ arena, u64 lo, u64 hi, int p, int j, u64* seed) {
    constexpr int W = M::W, MW = M::MW;
    using ull = unsigned long long;
    const u64 i = lo + (u64)blockIdx.x * STEP_BLOCK + threadIdx.x;
    bool cand = false;
    u32 slot = ~0u;
    u64 s[W];
#pragma unroll
    for (int x = 0; x < W; ++x) s[x] = ~0ull;
    if (i < hi) {
        load_state<W>(arena, i, s);
        cand = true;
#pragma unroll
        for (int x = 0; x < W; ++x)
            if (x < j) cand = cand && s[x] == seed[x];
        if (cand) {  // its first violating slot, if it has one
            u64 mask[MW], out[W];
            m.enabled(s, mask);
            for (int w = 0; w < MW && slot == ~0u; ++w)
                for (u64 bits = mask[w]; bits && slot == ~0u; bits &= bits - 1) {
                    const int a = w * 64 + __builtin_ctzll(bits);
                    if (m.apply(s, a, out) && !step_holds_of(m, p, s, a, out)) slot = (u32)a;
                }
            cand = slot != ~0u;
        }
    }
    const u64 cm = __ballot(cand);
    if (!cm) return;
    if (j >= W) {
        if (cand) {  // (more than one lane only where an init state repeats)
            atomicMin(reinterpret_cast<ull*>(seed + W), (ull)slot);
            atomicMin(reinterpret_cast<ull*>(seed + W + 1), (ull)i);
        }
        return;
    }
    u64 v = ~0ull;
#pragma unroll
    for (int x = 0; x < W; ++x)  // (no dynamic index: the state stays in registers)
        if (x == j && cand) v = s[x];
    v = step_wave_min(v);
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(cm)) atomicMin(reinterpret_cast<ull*>(seed + j), (ull)v);
}

}  // namespace sr
