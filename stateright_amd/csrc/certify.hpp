// The certificate pass: a finished check verified from what it leaves behind, with no oracle
// and at any size. The arena lists exactly the reachable set of the model, level by level, iff
//   (roots)    it starts with the init states;
//   (tree)     every listed state has a listed parent in the level before it and an action that produces it;
//   (closure)  every successor of a listed state is listed, at most one level below its generator;
//   (set)      table and arena are equal as sets (the map pass shows arena -> table; the visited-set audit of
//              a counting run, kernels_audit.hpp, shows the rest).
// By induction over levels: level 0 is the init states; a state of level d + 1 has a generator in level d
// (tree), so its depth is at most d + 1, and no state of depth d + 1 sits anywhere else (closure: a successor of
// a level-d state is listed at a level <= d + 1, and listed once: the table holds a state once and the map pass
// writes one level per slot). In FIFO order the reference's visit order is pinned the same way: a level is sorted
// by tag = (parent's rank) * A + (first generating slot), strictly (order), every tag names a generator
// (tree_slot), and no earlier generator exists (fifo_not_first).
//
// Definitions, all counts 64 bits and exact. n = lstart.back() arena states, level L holds the indices
// lstart[L] .. lstart[L + 1] - 1; A = max_actions(); tag(s) = meta[slot(s)] & (2^44 - 1) in FIFO order;
// slot(s) is the lookup every reader of the table uses (probe_key, then linear probing up to a vacant slot).
//   roots_wrong      indices i < k whose state is not the expected one. Level 0 is the init states in REVERSE
//                    order (the reference pops its pending states from the back, bfs.rs:43-66): index i holds
//                    init state k - 1 - i.
//   map_missing      states that the table does not hold. The map: level_of_slot[slot(s)] = the lowest level of
//                    an arena state s with that slot.
//   tree_range       states of a level d >= 1 whose parent rank p = apar[i] is >= the size of level d - 1. Such
//                    a rank is compared and counted, never used as an index.
//   tree_edge        in-range ones whose parent (index lstart[d - 1] + p) has no enabled slot a with
//                    apply(parent, a) equal to the state, word by word.
//   tree_slot        FIFO: ... whose lowest such slot a does not satisfy tag(s) == p * A + a (a state the table
//                    does not hold has no tag and is not counted here).
// Only when the search explored everything; an index below k that repeats an earlier init state counts its
// successors in repeated_edges and nothing else (the search expands such a state again and counts them again):
//   edges            pairs (s, a): s listed, a enabled, apply(s, a, t) succeeding. inits + edges + repeated_edges
//                    is the search's state_count.
//   closure_missing  such pairs whose t the table does not hold;
//   closure_unlisted ... whose slot no arena state mapped to;
//   closure_late     ... whose mapped level is greater than level(s) + 1;
//   fifo_not_first   FIFO: ... whose mapped level is level(s) + 1 and rank(s) * A + a < tag(t).
// FIFO only:
//   fifo_order       indices i > lstart[d], d >= 1, with tag(arena[i - 1]) >= tag(arena[i]) (both in the table).
// Per property p outside emask() | lmask() | smask():
//   holds[p]         states where discovers(p, s); first_index[p] the lowest such index (all ones: none);
//   disc_wrong[p]    1 when discovers(p, .) is false at the engine's own discovery index disc_index[p].
//
// The kernels (kernels_certify.hpp) and the host evaluation (cert_host below: plain loops over host copies,
// sharing nothing with the kernels beyond the model and probe_key, the table's address function) are two
// writings of these definitions; sr_selftest_certify_gpu compares them on planted errors (certify_selftest.hpp).
#pragma once
#include <string>
#include <vector>

#include "../../include/stateright_gpu.h"
#include "device.hpp"
#include "kernels.hpp"
#include "kernels_certify.hpp"

namespace sr {

inline sr_certificate cert_none() {
    sr_certificate c{};
    for (int p = 0; p < 32; ++p) c.first_index[p] = c.disc_index[p] = ~0ull, c.first_level[p] = c.disc_level[p] = ~0u;
    return c;
}

// What a pass is given besides the model, the table and the arena.
struct CertInput {
    std::vector<u64> lstart;  // nlevels + 1 offsets
    bool fifo = false, explored_all = false;
    u32 pmask = 0;            // the properties to count
    u64 disc_index[32];       // the engine's discovery indices (all ones: none)
    u32 grid = 0;             // != 0: the persistent grid (SR_CERT_GRID)
    CertInput() {
        for (u64& d : disc_index) d = ~0ull;
    }
};

template <class M>
std::vector<u64> init_states_of(const M& m);  // (engine.hpp)

// Level 0 as the arena must hold it (the init states reversed), and the bit mask of its indices that repeat an
// earlier init state; returns how many do.
template <class M>
inline u64 cert_level0(const M& m, std::vector<u64>& want, std::vector<u32>& skip) {
    constexpr int W = M::W;
    const std::vector<u64> inits = init_states_of(m);
    const size_t k = inits.size() / W;
    want.resize(k * W);
    skip.assign((k + 31) / 32, 0u);
    u64 dups = 0;
    for (size_t i = 0; i < k; ++i) {
        std::copy(&inits[i * W], &inits[i * W] + W, &want[(k - 1 - i) * W]);
        bool seen = false;
        for (size_t j = 0; j < i && !seen; ++j) seen = std::equal(&inits[i * W], &inits[i * W] + W, &inits[j * W]);
        if (seen) {
            const size_t at = k - 1 - i;
            skip[at >> 5] |= 1u << (at & 31);
            ++dups;
        }
    }
    return dups;
}

// The levels of the first discovering index and of the engine's own, off the level offsets.
inline void cert_fill_levels(sr_certificate& c, const CertInput& in) {
    auto level_of = [&](u64 i) {
        return i < in.lstart.back() ? (u32)(std::upper_bound(in.lstart.begin(), in.lstart.end(), i) - in.lstart.begin()) - 1 : ~0u;
    };
    for (int p = 0; p < 32; ++p) c.first_level[p] = level_of(c.first_index[p]), c.disc_level[p] = level_of(c.disc_index[p]);
}

inline void cert_fill_header(sr_certificate& c, const CertInput& in, u64 k, u64 dups) {
    c.fifo = in.fifo ? 1u : 0u;
    c.explored_all = in.explored_all ? 1u : 0u;
    c.states = in.lstart.back();
    c.levels = in.lstart.size() - 1;
    c.inits = k;
    c.repeated_inits = dups;
    c.pmask = in.pmask;
    for (int p = 0; p < 32; ++p) c.disc_index[p] = in.disc_index[p];
}

// The pass on the device: arena, apar and the table `t` of `cap` slots are device memory; every buffer of the
// pass lives for this call only. If the level map cannot be allocated the pass reports ran = 0, skipped = 1.
template <class M>
inline sr_certificate cert_device(const M& m, const TableView& t, u64 cap, const u64* arena, const u32* apar, const CertInput& in, int device,
                                  hipStream_t s) {
    constexpr int W = M::W;
    const auto t0 = std::chrono::steady_clock::now();
    sr_certificate c = cert_none();
    std::vector<u64> want;
    std::vector<u32> skip;
    const u64 dups = cert_level0(m, want, skip);
    const u64 k = want.size() / W, n = in.lstart.back();
    const u32 nlevels = (u32)in.lstart.size() - 1, A = (u32)std::max(1, m.max_actions());
    c.nprops = (u32)M::NPROPS;
    cert_fill_header(c, in, k, dups);
    if (in.lstart.size() < 2 || in.lstart[0] != 0 || in.lstart[1] != k || n < k || !cap)
        throw Error(SR_ERR_ARG, "certificate: level 0 of the arena is not the model's init count");
    DBuf<u32> lvl, skip_d;
    try {
        lvl.alloc(device, (size_t)cap);
    } catch (const Error&) {
        (void)hipGetLastError();
        c.skipped = 1;
        return c;
    }
    DBuf<u64> g, ls, want_d;
    g.alloc(device, CERT_WORDS);
    ls.alloc(device, in.lstart.size());
    want_d.alloc(device, want.size());
    SR_HIP(hipMemsetAsync(lvl.p, 0xff, (size_t)cap * sizeof(u32), s));
    SR_HIP(hipMemsetAsync(g.p, 0, CERT_FIRST * sizeof(u64), s));
    SR_HIP(hipMemsetAsync(g.p + CERT_FIRST, 0xff, (CERT_WORDS - CERT_FIRST) * sizeof(u64), s));
    SR_HIP(hipMemcpyAsync(ls.p, in.lstart.data(), in.lstart.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    if (k) SR_HIP(hipMemcpyAsync(want_d.p, want.data(), want.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    if (dups) {
        skip_d.alloc(device, skip.size());
        SR_HIP(hipMemcpyAsync(skip_d.p, skip.data(), skip.size() * sizeof(u32), hipMemcpyHostToDevice, s));
    }
    int cus = 0;
    SR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // the persistent grid of kernel f over `count` states: its resident workgroups, at most one per CERT_BLOCK states
    auto grid_of = [&](const void* f, u64 count) {
        int per_cu = 0;
        SR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, CERT_BLOCK, 0));
        u64 grid = per_cu > 0 && cus > 0 ? (u64)per_cu * (u64)cus : 1024;
        if (in.grid) grid = in.grid;
        return (u32)std::max<u64>(1, std::min<u64>(grid, (count + CERT_BLOCK - 1) / CERT_BLOCK));
    };
    CertDisc disc;
    for (int p = 0; p < CERT_MAX_PROPS; ++p) disc.at[p] = in.disc_index[p];
    if (k) cert_roots<M><<<grid_of((const void*)cert_roots<M>, k), CERT_BLOCK, 0, s>>>(arena, want_d.p, k, g.p);
    if (n) {
        cert_map<M><<<grid_of((const void*)cert_map<M>, n), CERT_BLOCK, 0, s>>>(m, t, arena, n, ls.p, nlevels, lvl.p, g.p);
        if (in.pmask) cert_props<M><<<grid_of((const void*)cert_props<M>, n), CERT_BLOCK, 0, s>>>(m, arena, n, in.pmask, disc, g.p);
    }
    if (n > k) {
        if (in.fifo) {
            cert_tree<M, true><<<grid_of((const void*)cert_tree<M, true>, n - k), CERT_BLOCK, 0, s>>>(m, t, arena, apar, n, ls.p, nlevels, A, g.p);
            cert_order<M><<<grid_of((const void*)cert_order<M>, n - k), CERT_BLOCK, 0, s>>>(m, t, arena, n, ls.p, nlevels, g.p);
        } else {
            cert_tree<M, false><<<grid_of((const void*)cert_tree<M, false>, n - k), CERT_BLOCK, 0, s>>>(m, t, arena, apar, n, ls.p, nlevels, A, g.p);
        }
    }
    if (in.explored_all && n) {  // (behind cert_map on the stream: it reads the level map)
        const u32* sk = dups ? skip_d.p : nullptr;
        const u32 k0 = dups ? (u32)k : 0u;
        if (in.fifo)
            cert_closure<M, true><<<grid_of((const void*)cert_closure<M, true>, n), CERT_BLOCK, 0, s>>>(m, t, arena, n, ls.p, nlevels, sk, k0, A, lvl.p, g.p);
        else
            cert_closure<M, false><<<grid_of((const void*)cert_closure<M, false>, n), CERT_BLOCK, 0, s>>>(m, t, arena, n, ls.p, nlevels, sk, k0, A, lvl.p, g.p);
    }
    SR_HIP(hipGetLastError());
    std::vector<u64> h(CERT_WORDS);
    SR_HIP(hipMemcpyAsync(h.data(), g.p, CERT_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
    SR_HIP(stream_sync(s));
    c.roots_wrong = h[CERT_ROOTS_WRONG];
    c.map_missing = h[CERT_MAP_MISSING];
    c.tree_range = h[CERT_TREE_RANGE];
    c.tree_edge = h[CERT_TREE_EDGE];
    c.tree_slot = h[CERT_TREE_SLOT];
    c.edges = h[CERT_EDGES];
    c.repeated_edges = h[CERT_REP_EDGES];
    c.closure_missing = h[CERT_CL_MISSING];
    c.closure_unlisted = h[CERT_CL_UNLISTED];
    c.closure_late = h[CERT_CL_LATE];
    c.fifo_not_first = h[CERT_NOT_FIRST];
    c.fifo_order = h[CERT_ORDER];
    for (int p = 0; p < M::NPROPS; ++p) {
        if (!(in.pmask >> p & 1)) continue;
        c.holds[p] = h[CERT_HOLDS + p];
        c.disc_wrong[p] = h[CERT_DISC_WRONG + p];
        c.first_index[p] = h[CERT_FIRST + p];
    }
    cert_fill_levels(c, in);
    c.ran = 1;
    c.pass_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return c;
}

// A host copy of a table: slot values unpacked (one u64 per slot, whatever the slot width), meta in FIFO order.
struct CertHostTable {
    TableView t{};
    u64 cap = 0;
    std::vector<u64> v, meta;
};

// The same definitions evaluated on the host, state by state in plain loops.
template <class M>
inline sr_certificate cert_host(const M& m, const CertHostTable& T, const std::vector<u64>& arena, const std::vector<u32>& apar, const CertInput& in) {
    constexpr int W = M::W, MW = M::MW;
    sr_certificate c = cert_none();
    std::vector<u64> want;
    std::vector<u32> skip;
    const u64 dups = cert_level0(m, want, skip);
    const u64 k = want.size() / W, n = in.lstart.back(), A = (u64)std::max(1, m.max_actions());
    const size_t nlevels = in.lstart.size() - 1;
    c.nprops = (u32)M::NPROPS;
    cert_fill_header(c, in, k, dups);
    const u64 tagmask = (1ull << 44) - 1;
    // slot(s): linear probing from the key's home up to a vacant slot
    auto slot_of = [&](const u64* s) -> u64 {
        const ProbeKey pk = probe_key(m, T.t, s);
        for (u64 d = 0; d < (u64)MAX_PROBE; ++d) {
            const u64 i = (pk.home + d) & T.t.mask, cur = T.v[i];
            if (cur == pk.tag + (T.t.qbits ? d : 0)) return i;
            if (!cur) return ~0ull;
        }
        return ~0ull;
    };
    std::vector<u32> level_of(n);
    for (size_t L = 0; L < nlevels; ++L)
        for (u64 i = in.lstart[L]; i < in.lstart[L + 1]; ++i) level_of[i] = (u32)L;
    for (u64 i = 0; i < k; ++i)
        if (!std::equal(&arena[i * W], &arena[i * W] + W, &want[i * W])) c.roots_wrong += 1;
    std::vector<u32> slot_level(T.cap, 0xffffffffu);
    for (u64 i = 0; i < n; ++i) {
        const u64 sl = slot_of(&arena[i * W]);
        if (sl == ~0ull) c.map_missing += 1;
        else slot_level[sl] = std::min(slot_level[sl], level_of[i]);
    }
    for (u64 i = k; i < n; ++i) {
        const u32 d = level_of[i];
        const u64 p = apar[i];
        if (p >= in.lstart[d] - in.lstart[d - 1]) {
            c.tree_range += 1;
            continue;
        }
        const u64* par = &arena[(in.lstart[d - 1] + p) * W];
        u64 mask[MW], out[W];
        m.enabled(par, mask);
        i64 first = -1;
        for (int a = 0; a < 64 * MW && first < 0; ++a)
            if ((mask[a >> 6] >> (a & 63) & 1) && m.apply(par, a, out) && std::equal(out, out + W, &arena[i * W])) first = a;
        if (first < 0) {
            c.tree_edge += 1;
        } else if (in.fifo) {
            const u64 sl = slot_of(&arena[i * W]);
            if (sl != ~0ull && (T.meta[sl] & tagmask) != p * A + (u64)first) c.tree_slot += 1;
        }
    }
    if (in.explored_all)
        for (u64 i = 0; i < n; ++i) {
            const bool repeated = i < k && (skip[i >> 5] >> (i & 31) & 1);
            const u32 d = level_of[i];
            const u64 rank = i - in.lstart[d];
            u64 mask[MW], out[W];
            m.enabled(&arena[i * W], mask);
            for (int a = 0; a < 64 * MW; ++a) {
                if (!(mask[a >> 6] >> (a & 63) & 1) || !m.apply(&arena[i * W], a, out)) continue;
                if (repeated) {
                    c.repeated_edges += 1;
                    continue;
                }
                c.edges += 1;
                const u64 sl = slot_of(out);
                if (sl == ~0ull) c.closure_missing += 1;
                else if (slot_level[sl] == 0xffffffffu) c.closure_unlisted += 1;
                else if (slot_level[sl] > d + 1) c.closure_late += 1;
                else if (in.fifo && slot_level[sl] == d + 1 && rank * A + (u64)a < (T.meta[sl] & tagmask)) c.fifo_not_first += 1;
            }
        }
    if (in.fifo)
        for (u64 i = k + 1; i < n; ++i) {
            if (level_of[i] != level_of[i - 1]) continue;
            const u64 a = slot_of(&arena[i * W]), b = slot_of(&arena[(i - 1) * W]);
            if (a != ~0ull && b != ~0ull && (T.meta[b] & tagmask) >= (T.meta[a] & tagmask)) c.fifo_order += 1;
        }
    for (int p = 0; p < M::NPROPS; ++p) {
        if (!(in.pmask >> p & 1)) continue;
        for (u64 i = 0; i < n; ++i) {
            const bool h = m.discovers(p, &arena[i * W]);
            if (h) {
                c.holds[p] += 1;
                if (c.first_index[p] == ~0ull) c.first_index[p] = i;
            } else if (in.disc_index[p] == i) {
                c.disc_wrong[p] += 1;
            }
        }
    }
    cert_fill_levels(c, in);
    c.ran = 1;
    return c;
}

}  // namespace sr
