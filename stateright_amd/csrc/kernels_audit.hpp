// The visited-set audit (sr_opts.counters; sr_gpu_bfs_table_audit, include/stateright_gpu.h): the
// final table checked against the arena, which holds every visited state. Two passes, both read-only
// on the table:
//  * audit_table, one thread per slot: the slot's own invariants (displacement within the probe
//    limit, a home its key can have, no vacant slot between home and slot) and no second copy of its
//    key nearer its home;
//  * audit_arena, one thread per arena state: the state is found (find_slot over probe_key, the
//    lookup every reader of the table uses), no other arena state resolves to the same slot (a
//    bitmap over slots), and in FIFO order the slot's meta names the state's level and its parent.
// Together: table and arena are equal as sets when occupied == arena_states and every error field
// is 0. After a check that stopped early (every property discovered inside a level, or a target
// count), the level being expanded at the stop, or a speculative one past it, has claimed slots
// for states that no arena level lists: then occupied >= arena_states, and the other fields are
// still 0. Init states that the model lists twice are two arena states of one slot (arena_shared).
// Nothing here is launched unless sr_opts.counters is set.
#pragma once
#include "kernels.hpp"

namespace sr {

struct AuditCounters {
    unsigned long long occupied, misplaced, duplicates, arena_states, arena_missing, arena_shared, meta_wrong;
};

// Which states of an arena belong to the audited table: all of them, or (the partitioned engine's
// replicated head, dist.hpp) those a partition owns.
struct AuditKeepAll {
    template <class M>
    __device__ bool operator()(const M&, const u64*) const { return true; }
};

template <int = 0>
__global__ void __launch_bounds__(256) audit_table(TableView t, u64 cap, AuditCounters* out) {
    const u64 dmask = t.qbits ? (1ull << t.dbits) - 1 : 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < cap; base += (u64)gridDim.x * blockDim.x) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < cap ? slot_load(t, i) : 0;
        bool bad = false, dup = false;
        if (v) {
            // quotient mode stores 1 + the displacement (0 there is no slot value of any key)
            const u64 d = t.qbits ? (v & dmask) - 1 : (i - (v & t.mask)) & t.mask;
            if (d >= (u64)t.plimit) {
                bad = true;
            } else {
                const u64 home = (i - d) & t.mask;
                // a quotient key is below 2^B: a table larger than the key space homes its keys in
                // the first 2^(B - 1) slots (make_table_view)
                if (t.qbits && t.bbits < 128 && (quot_decode(t, i, v) >> t.bbits)) bad = true;
                for (u64 e = 0; e < d; ++e) {
                    const u64 w = slot_load(t, (home + e) & t.mask);
                    if (!w) bad = true;
                    // the same key at displacement e: tag + e (quotient), the fingerprint itself
                    if (w == (t.qbits ? v - (d - e) : v)) dup = true;
                }
            }
        }
        const u32 nocc = (u32)__syncthreads_count(v != 0), nbad = (u32)__syncthreads_count(bad),
                  ndup = (u32)__syncthreads_count(dup);
        if (threadIdx.x == 0) {
            if (nocc) atomicAdd(&out->occupied, (unsigned long long)nocc);
            if (nbad) atomicAdd(&out->misplaced, (unsigned long long)nbad);
            if (ndup) atomicAdd(&out->duplicates, (unsigned long long)ndup);
        }
    }
}

// arena: n states; lstart[0..nlevels] their levels' offsets (FIFO order: meta and apar, the parent
// ranks, are checked; else both are null). marks: one bit per slot, zeroed.
template <class M, class Keep>
__global__ void __launch_bounds__(256) audit_arena(M m, TableView t, const u64* __restrict__ arena,
                                                   const u32* __restrict__ apar, u64 n, const u64* __restrict__ lstart,
                                                   u32 nlevels, u32 A, u32* marks, AuditCounters* out, Keep keep) {
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += (u64)gridDim.x * blockDim.x) {
        const u64 idx = base + threadIdx.x;
        bool kept = false, missing = false, shared = false, meta_bad = false;
        u64 s[M::W];
        if (idx < n) {
            load_state<M::W>(arena, idx, s);
            kept = keep(m, s);
        }
        if (kept) {
            const u64 slot = find_slot(t, probe_key(m, t, s));
            if (slot == ~0ull) {
                missing = true;
            } else {
                const u32 bit = 1u << (slot & 31);
                shared = (atomicOr(&marks[slot >> 5], bit) & bit) != 0;
                if (t.meta) {
                    u32 lo = 0, hi = nlevels;  // the level L with lstart[L] <= idx < lstart[L + 1]
                    while (hi - lo > 1) {
                        const u32 mid = (lo + hi) / 2;
                        (lstart[mid] <= idx ? lo : hi) = mid;
                    }
                    const u64 meta = t.meta[slot];
                    if (lo == 0) meta_bad = meta != 0;
                    else
                        meta_bad = (meta >> META_SHIFT) != (u64)lo ||
                                   (meta & ((1ull << META_SHIFT) - 1)) / A != (u64)apar[idx];
                }
            }
        }
        const u32 nk = (u32)__syncthreads_count(kept);
        const u32 nm = (u32)__syncthreads_count(missing), ns = (u32)__syncthreads_count(shared),
                  nw = (u32)__syncthreads_count(meta_bad);
        if (threadIdx.x == 0) {
            if (nk) atomicAdd(&out->arena_states, (unsigned long long)nk);
            if (nm) atomicAdd(&out->arena_missing, (unsigned long long)nm);
            if (ns) atomicAdd(&out->arena_shared, (unsigned long long)ns);
            if (nw) atomicAdd(&out->meta_wrong, (unsigned long long)nw);
        }
    }
}

// Host: the two passes, enqueued on `s`; the counters are ADDED to *acc (zeroed by the caller, so
// the partitioned engine sums its parts into one). The table pass also clears marks (>= (cap + 31)
// / 32 words), which the arena passes over that table then share. lstart_d: nlevels + 1 offsets on
// the device (FIFO order only).
inline void launch_audit_table(const TableView& t, u64 cap, u32* marks, AuditCounters* acc, hipStream_t s) {
    SR_HIP(hipMemsetAsync(marks, 0, (size_t)((cap + 31) / 32) * sizeof(u32), s));
    audit_table<<<(u32)std::min<u64>((cap + 255) / 256, 8192), 256, 0, s>>>(t, cap, acc);
    SR_HIP(hipGetLastError());
}
template <class M, class Keep = AuditKeepAll>
inline void launch_audit_arena(const M& m, const TableView& t, const u64* arena, const u32* apar, u64 n, const u64* lstart_d,
                               u32 nlevels, u32 A, u32* marks, AuditCounters* acc, hipStream_t s, Keep keep = Keep{}) {
    if (!n) return;
    audit_arena<M, Keep><<<(u32)std::min<u64>((n + 255) / 256, 8192), 256, 0, s>>>(m, t, arena, apar, n, lstart_d, nlevels,
                                                                                   A ? A : 1u, marks, acc, keep);
    SR_HIP(hipGetLastError());
}

}  // namespace sr
