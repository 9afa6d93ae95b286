// GPU self-test of the visited set's growth kernels on synthetic tables (sr_selftest_rehash_gpu,
// include/stateright_gpu.h): rehash_ranges<u32|u64> + rehash_spill, rehash (with meta) and
// remap_slots, launched through launch_rehash, the routine both engines grow their tables with.
//
// The kernels read slot values only, so an old table is built on the host from permuted keys
// directly (home << remainder bits | remainder, no model state), uploaded, grown, downloaded and
// compared with a plain host rebuild: sequential linear probing into a std::vector<u64>. The set
// of occupied slots of a linear-probing table and the number of entries pushed past any boundary
// do not depend on the insertion order, so these are exact expectations whatever order the GPU
// inserted in: the occupied bitmap, the spill count (the sum over ranges of the entries that do
// not fit before the range's end), and the multiset of decoded keys (which holds every entry's
// stored displacement: a wrong one decodes to another home). The result is also checked for a
// vacant slot between any entry's home and its slot, and the error word for its expected value.
// A table that rehash_ranges builds is allocated full of a poison pattern, not zeros: the kernel
// has to write every slot.
//
// Views are Spread-style views from make_table_view (natural probe limits):
//   one word,  B = 30: 4-byte slots at every size here           -> rehash_ranges<u32>
//   two words, B = 50: 8-byte slots                              -> rehash_ranges<u64>
//   one word,  B = 35 at 2^12 slots: 8-byte slots (23 remainder bits) growing by 2, 8 or 64 into
//     4-byte slots (22, 20, 17 bits) range by range: `from` and `to` differ in slot width and
//     rehash_by_ranges holds, (B, cap, lg) = (35, 2^12, 1 | 3 | 6); rehash_ranges<u32> then reads
//     8-byte slots (B = 30 at 2^7 slots grown by 64, the one-range case below, is another)
//   one word,  B = 64: fingerprint mode (rehash by CAS only)
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace sr {
namespace rehash_test {

constexpr u64 POISON = 0xA5A5A5A5A5A5A5A5ull;
constexpr u64 GUARD = 0x6755415244ull;

inline TableView view_of(int W, int B, u64 cap) {
    if (W == 1) return make_table_view(Spread<1>{B, 1, 0, 0}, nullptr, nullptr, cap, true);
    return make_table_view(Spread<2>{B, 1, 0, 0}, nullptr, nullptr, cap, true);
}

// A linear-probing table on the host; keys are permuted keys (quotient mode) or fingerprints.
struct HostTable {
    TableView t;
    u64 cap;
    std::vector<u64> v;
    HostTable(const TableView& tv, u64 c) : t(tv), cap(c), v(c, 0) {}
    u64 home_of(u128 h) const { return t.qbits ? (u64)(h >> t.qbits) : (u64)h & t.mask; }
    u64 tag_of(u128 h) const { return t.qbits ? quot_probe(t, h).tag : (u64)h; }
    u128 key_at(u64 i) const { return t.qbits ? quot_decode(t, i, v[i]) : (u128)v[i]; }
    u64 disp_at(u64 i) const { return t.qbits ? (v[i] & ((1ull << t.dbits) - 1)) - 1 : (i - (v[i] & t.mask)) & t.mask; }
    // the slot, or ~0 when the table is full
    u64 insert(u128 h) {
        const u64 home = home_of(h), tag = tag_of(h), step = probe_step(t);
        for (u64 d = 0; d < cap; ++d) {
            const u64 i = (home + d) & t.mask;
            if (!v[i]) return v[i] = tag + d * step, i;
        }
        return ~0ull;
    }
    // no vacant slot between an entry's home and its slot, every displacement below the limit
    bool valid(std::string& why) const {
        for (u64 i = 0; i < cap; ++i) {
            if (!v[i]) continue;
            const u64 d = disp_at(i);
            if (d >= t.plimit) return why = "slot " + std::to_string(i) + " stores a displacement at or past the probe limit", false;
            for (u64 e = 0; e < d; ++e)
                if (!v[(i - d + e) & t.mask])
                    return why = "a vacant slot between slot " + std::to_string(i) + " and its home", false;
        }
        return true;
    }
};

// The key of old home `home` and remainder `rem` (quotient mode).
inline u128 qkey(const TableView& t, u64 home, u64 rem) { return ((u128)home << t.qbits) | (rem & ((1ull << t.qbits) - 1)); }

struct Case {
    std::string name;
    int W, B;
    u64 old_cap;
    u32 lg;
    std::vector<u128> keys;      // inserted into the old table in this order
    bool allow_ranges = true;
    bool with_meta = false;      // a meta array moves along (forces the CAS rehash), then remap_slots
    u32 plimit = 0;              // != 0: the new view's probe limit is lowered to this
    u64 spill_cap = 0;           // != 0: the spill list's capacity (a guard word behind it)
    u32 want_err = 0;
    bool want_ranges = true;
    i64 want_spills = -1;        // >= 0: the exact spill count; -2: more than 0
    u32 min_extensions = 0;      // of range `ext_range`'s window, from the host model
    u64 ext_range = 0;
};

inline u64 rnd(u64& r) { return r = fmix64(r + 0x9E3779B97F4A7C15ull); }

// n distinct random keys of the old view
inline void random_keys(const TableView& from, int B, u64 n, u64 seed, std::vector<u128>& out) {
    std::vector<u128> k;
    u64 r = seed;
    while (k.size() < n) {
        const u64 a = rnd(r), b = rnd(r);
        u128 h = ((u128)b << 64) | a;
        if (from.qbits) h &= ((u128)1 << B) - 1;
        else h = (u64)h ? (u64)h : 1;
        k.push_back(h);
        if (k.size() == n) {
            std::sort(k.begin(), k.end());
            k.erase(std::unique(k.begin(), k.end()), k.end());
        }
    }
    u64 s = seed ^ 0x5bd1e995;  // back out of sorted order
    for (size_t i = k.size(); i > 1; --i) std::swap(k[i - 1], k[rnd(s) % i]);
    out.insert(out.end(), k.begin(), k.end());
}

// Three keys homed in each of the last three old slots: inserted in order they fill the last three
// slots and wrap round into slots 0..5.
inline void wrap_cluster(const TableView& from, u64 old_cap, std::vector<u128>& out) {
    for (u64 h = old_cap - 3; h < old_cap; ++h)
        for (u64 j = 0; j < 3; ++j) out.push_back(from.qbits ? qkey(from, h, 0x155 + 7 * j + h) : (u128)(((0x9E37ull + j) << 40) | h));
}

// How often workgroup `r` of rehash_ranges extends its window over `old` before a vacant slot past
// its last home ends it (the kernel's loop, on the host).
inline u32 window_extensions(const std::vector<u64>& old, u64 old_cap, u64 a, u64 span) {
    u64 lo = 0, hi = std::min<u64>(span + REBUILD_BLOCK, old_cap);
    for (u32 ext = 0;; ++ext) {
        bool done = false;
        for (u64 off = std::max(lo, span); off < hi; ++off) done |= !old[(a + off) & (old_cap - 1)];
        if (done || hi >= old_cap) return ext;
        lo = hi;
        hi = std::min<u64>(hi + REBUILD_BLOCK, old_cap);
    }
}

// The entries rehash_ranges pushes past their range's end: per range of S new slots, the entries
// homed there that linear probing inside the range alone does not place.
inline u64 predicted_spills(const HostTable& old, const TableView& to, u64 cap, u64 S) {
    std::vector<std::vector<u64>> per(cap / S);
    for (u64 i = 0; i < old.cap; ++i)
        if (old.v[i]) {
            const u64 home = (u64)(old.key_at(i) >> to.qbits);
            per[home / S].push_back(home % S);
        }
    u64 spills = 0;
    std::vector<unsigned char> occ(S);
    for (auto& homes : per) {
        std::fill(occ.begin(), occ.end(), 0);
        for (u64 h : homes) {
            while (h < S && occ[h]) ++h;
            if (h < S) occ[h] = 1;
            else ++spills;
        }
    }
    return spills;
}

struct Runner {
    int dev;
    bool host_only = false;  // build every case and its expectations, launch nothing
    hipStream_t s = nullptr;
    DBuf<u64> spill;
    u64 cases = 0, by_ranges32 = 0, by_ranges64 = 0, by_cas = 0, mixed = 0, spilled = 0;
    u32 long_runs = 0;  // bit (4-byte slots ? 3 : 0) + (step 2, 8, 64: 0, 1, 2): the long-run case was built there

    template <class T>
    void upload(DBuf<T>& d, const std::vector<T>& h) {
        d.alloc(dev, h.size());
        SR_HIP(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));  // (blocking: h may be a temporary)
    }
    // slot values as the device stores them: 4-byte slots packed two to a word
    static std::vector<u64> packed(const TableView& t, const std::vector<u64>& v) {
        if (!t.s32) return v;
        std::vector<u64> w((v.size() + 1) / 2, 0);
        for (size_t i = 0; i < v.size(); ++i) w[i / 2] |= (v[i] & 0xffffffffull) << (32 * (i & 1));
        return w;
    }
    static std::vector<u64> unpacked(const TableView& t, const std::vector<u64>& w, u64 cap) {
        if (!t.s32) return w;
        std::vector<u64> v(cap);
        for (u64 i = 0; i < cap; ++i) v[i] = (w[i / 2] >> (32 * (i & 1))) & 0xffffffffull;
        return v;
    }

    // Empty: the case passed.
    std::string run(const Case& c) {
        ++cases;
        const u64 cap = c.old_cap << c.lg;
        TableView from = view_of(c.W, c.B, c.old_cap), to0 = view_of(c.W, c.B, cap);
        if (c.plimit) to0.plimit = c.plimit;
        const u64 S = to0.s32 ? rebuild_slots<u32>() : rebuild_slots<u64>();
        // the old table and its meta (a function of the key, so that it can be checked wherever the key lands)
        HostTable old(from, c.old_cap);
        for (u128 h : c.keys)
            if (old.insert(h) == ~0ull) return "the case does not fit its old table";
        std::string why;
        if (!old.valid(why)) return "old table: " + why;
        auto meta_of = [](u128 h) { return fmix64((u64)h ^ (u64)(h >> 64) ^ 0x4d455441ull) >> 1; };
        std::vector<u64> ometa;
        if (c.with_meta) {
            ometa.assign(c.old_cap, META_UNSET);
            for (u64 i = 0; i < c.old_cap; ++i)
                if (old.v[i]) ometa[i] = meta_of(old.key_at(i));
        }
        // the host rebuild
        HostTable want(to0, cap);
        if (!c.want_err)
            for (u64 i = 0; i < c.old_cap; ++i)
                if (old.v[i] && want.insert(old.key_at(i)) == ~0ull) return "the case does not fit its new table";
        const bool ranges_ok = c.allow_ranges && !c.with_meta && rehash_by_ranges(from, to0, c.lg, cap);
        if (ranges_ok != c.want_ranges) return c.want_ranges ? "the pair does not grow range by range" : "the pair grows range by range";
        const u64 spills = ranges_ok ? predicted_spills(old, to0, cap, S) : 0;
        if (c.want_spills >= 0 && spills != (u64)c.want_spills)
            return "the host model predicts " + std::to_string(spills) + " spills, the case was built for " + std::to_string(c.want_spills);
        if (c.want_spills == -2 && !spills) return "the host model predicts no spill: the case does not test the spill list";
        if (c.min_extensions) {
            const u64 span = S >> c.lg;
            const u32 ext = window_extensions(old.v, c.old_cap, c.ext_range * span, span);
            if (ext < c.min_extensions)
                return "the host model predicts " + std::to_string(ext) + " window extensions, the case needs " + std::to_string(c.min_extensions);
            long_runs |= 1u << ((to0.s32 ? 3 : 0) + (c.lg == 1 ? 0 : c.lg == 3 ? 1 : 2));
        }

        if (host_only) return "";

        // device: old table, new table through launch_rehash
        DBuf<u64> ok, om, nk, nm;
        DBuf<u32> err, cand;
        upload(ok, packed(from, old.v));
        if (c.with_meta) upload(om, ometa);
        from.keys = ok.p;
        from.meta = c.with_meta ? om.p : nullptr;
        err.alloc(dev, 1);
        SR_HIP(hipMemsetAsync(err.p, 0, sizeof(u32), s));
        if (c.spill_cap) {  // [0] count, spill_cap entries, the guard word
            const std::vector<u64> sp(c.spill_cap + 2, GUARD);
            upload(spill, sp);
        }
        const u64 words = table_words(to0, cap);
        TableView to = to0;
        const bool ranges = launch_rehash(
            from, c.old_cap, to0, cap, c.allow_ranges,
            [&](bool by_ranges) {
                nk.alloc(dev, words);
                SR_HIP(hipMemsetAsync(nk.p, by_ranges ? 0xA5 : 0, words * sizeof(u64), s));
                to.keys = nk.p;
                if (c.with_meta) {
                    nm.alloc(dev, cap);
                    SR_HIP(hipMemsetAsync(nm.p, 0xff, cap * sizeof(u64), s));
                    to.meta = nm.p;
                }
                return to;
            },
            spill, dev, err.p, s, c.spill_cap);
        if (ranges != ranges_ok) return "launch_rehash chose the other path";
        (ranges ? (to0.s32 ? by_ranges32 : by_ranges64) : by_cas)++;
        if (ranges && from.s32 != to0.s32) ++mixed;
        std::vector<u32> cand_h;
        if (c.with_meta) {
            // every occupied old slot is a candidate, every vacant one CAND_NONE
            cand_h.assign(c.old_cap, CAND_NONE);
            for (u64 i = 0; i < c.old_cap; ++i)
                if (old.v[i]) cand_h[i] = (u32)i;
            upload(cand, cand_h);
            remap_slots<<<(u32)((c.old_cap + 255) / 256), 256, 0, s>>>(cand.p, c.old_cap, from, to);
            SR_HIP(hipGetLastError());
        }
        std::vector<u64> got_w(words), got_meta(c.with_meta ? cap : 0), sp_h(ranges ? (c.spill_cap ? c.spill_cap + 2 : 1) : 0);
        u32 err_h = 0;
        SR_HIP(hipMemcpyAsync(got_w.data(), nk.p, words * sizeof(u64), hipMemcpyDeviceToHost, s));
        if (c.with_meta) {
            SR_HIP(hipMemcpyAsync(got_meta.data(), nm.p, cap * sizeof(u64), hipMemcpyDeviceToHost, s));
            SR_HIP(hipMemcpyAsync(cand_h.data(), cand.p, c.old_cap * sizeof(u32), hipMemcpyDeviceToHost, s));
        }
        if (!sp_h.empty()) SR_HIP(hipMemcpyAsync(sp_h.data(), spill.p, sp_h.size() * sizeof(u64), hipMemcpyDeviceToHost, s));
        SR_HIP(hipMemcpyAsync(&err_h, err.p, sizeof(u32), hipMemcpyDeviceToHost, s));
        SR_HIP(stream_sync(s));
        if (c.spill_cap) spill.reset();  // (the next case sizes its own)

        if (err_h != c.want_err) return "error word " + std::to_string(err_h) + ", expected " + std::to_string(c.want_err);
        if (ranges) {
            if (sp_h[0] != spills) return "spill count " + std::to_string(sp_h[0]) + ", the host model predicts " + std::to_string(spills);
            if (c.spill_cap && sp_h[c.spill_cap + 1] != GUARD) return "a write past the spill list's capacity";
            spilled += spills;
        }
        if (c.want_err) return "";  // (entries were dropped: nothing more to compare)
        HostTable got(to0, cap);
        got.v = unpacked(to0, got_w, cap);
        for (u64 i = 0; i < cap; ++i)
            if ((got.v[i] != 0) != (want.v[i] != 0))
                return "slot " + std::to_string(i) + " is " + (got.v[i] ? "occupied" : "vacant") + ", the host rebuild's is not";
        if (!got.valid(why)) return why;
        std::vector<u128> a, b;
        for (u64 i = 0; i < cap; ++i)
            if (got.v[i]) a.push_back(got.key_at(i)), b.push_back(want.key_at(i));
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b) return "the decoded keys differ from the host rebuild's";
        if (c.with_meta) {
            for (u64 i = 0; i < cap; ++i)
                if (got_meta[i] != (got.v[i] ? meta_of(got.key_at(i)) : META_UNSET))
                    return "meta of new slot " + std::to_string(i) + " is not its key's";
            for (u64 i = 0; i < c.old_cap; ++i) {
                if (!old.v[i]) {
                    if (cand_h[i] != CAND_NONE) return "remap_slots changed a CAND_NONE entry";
                } else if (cand_h[i] >= cap || !got.v[cand_h[i]] || got.key_at(cand_h[i]) != old.key_at(i)) {
                    return "remap_slots: old slot " + std::to_string(i) + " does not map to its key's new slot";
                }
            }
        }
        return "";
    }
};

// The cases of one (W, B) at one old size and growth step.
inline void build_cases(int W, int B, u64 old_cap, u32 lg, bool random_only, std::vector<Case>& out) {
    const u64 cap = old_cap << lg;
    const TableView from = view_of(W, B, old_cap), to = view_of(W, B, cap);
    const u64 S = to.s32 ? rebuild_slots<u32>() : rebuild_slots<u64>();
    const bool ranges = rehash_by_ranges(from, to, lg, cap);
    const u64 span = S >> lg, nranges = cap / S;
    auto base = [&](const char* what) {
        Case c;
        c.name = std::string(what) + " W=" + std::to_string(W) + " B=" + std::to_string(B) + " 2^" +
                 std::to_string(__builtin_ctzll(old_cap)) + " x" + std::to_string(1u << lg);
        c.W = W, c.B = B, c.old_cap = old_cap, c.lg = lg;
        c.want_ranges = ranges;
        return c;
    };
    {
        Case c = base("random fill at load 0.45");
        random_keys(from, B, (u64)(0.45 * (double)old_cap), 0xC0FFEEull + old_cap + lg, c.keys);
        wrap_cluster(from, old_cap, c.keys);
        out.push_back(c);
        if (ranges) {  // the same table by CAS
            c.name += " (by CAS)";
            c.allow_ranges = false, c.want_ranges = false;
            out.push_back(c);
        }
        c = base("random fill with meta, then remap_slots");
        random_keys(from, B, (u64)(0.45 * (double)old_cap), 0xFEEDull + old_cap + lg, c.keys);
        wrap_cluster(from, old_cap, c.keys);
        c.with_meta = true, c.want_ranges = false;
        out.push_back(c);
    }
    if (random_only) return;
    out.push_back(base("empty table"));
    {
        Case c = base("slot 0 and the last slot");
        c.keys = {from.qbits ? qkey(from, 0, 5) : (u128)(3ull << 40), from.qbits ? qkey(from, old_cap - 1, 6) : (u128)((5ull << 40) | (old_cap - 1))};
        out.push_back(c);
        c = base("cluster wrapped round the old table's end");
        wrap_cluster(from, old_cap, c.keys);
        out.push_back(c);
    }
    if (!ranges || to.qbits < 3) return;
    // k keys whose new home is the last slot of new range r: old home (r + 1) span - 1, the lg
    // remainder bits that become home bits all ones
    auto pile = [&](u64 r, u64 k, std::vector<u128>& keys) {
        for (u64 j = 0; j < k; ++j) keys.push_back(qkey(from, (r + 1) * span - 1, ((((1ull << lg) - 1)) << to.qbits) | j));
    };
    // ... and in the middle of range r (old home r span + span / 2, those bits zero)
    auto pile_mid = [&](u64 r, u64 k, std::vector<u128>& keys) {
        for (u64 j = 0; j < k; ++j) keys.push_back(qkey(from, r * span + span / 2, j));
    };
    {
        Case c = base("spill past the last range's end, round to slot 0");
        pile(nranges - 1, 5, c.keys);
        c.want_spills = 4;
        out.push_back(c);
        if (nranges > 1) {
            c = base("spill into the next range");
            pile(0, 5, c.keys);
            pile(nranges - 1, 4, c.keys);
            c.want_spills = 7;
            out.push_back(c);
        }
        c = base("spill capacity 1 with 3 spills");
        pile(nranges - 1, 4, c.keys);
        c.want_spills = 3, c.spill_cap = 1, c.want_err = ERR_TABLE_FULL;
        out.push_back(c);
        c = base("a run that reaches a lowered probe limit");
        pile_mid(nranges - 1, 6, c.keys);
        c.plimit = 4, c.want_err = ERR_TABLE_FULL, c.want_spills = 0;
        out.push_back(c);
        c.name += " (by CAS)";
        c.allow_ranges = false, c.want_ranges = false;
        out.push_back(c);
    }
    // a run of consecutive homes at displacement 0 from range 0's last home, longer than the first
    // window and two rows more
    const u64 run = span + 2 * REBUILD_BLOCK + 8;
    if (span - 1 + run < old_cap) {
        Case c = base("a run longer than the first window");
        for (u64 j = 0; j < run; ++j) c.keys.push_back(qkey(from, span - 1 + j, 0x2aaa + j));
        c.min_extensions = 2, c.ext_range = 0;
        out.push_back(c);
    }
}

inline bool run_all(int device, std::string& why, bool host_only = false) {
    if (!host_only) SR_HIP(hipSetDevice(device));
    Runner R{device, host_only};
    std::vector<Case> cases;
    // 4-byte and 8-byte slots: every case at 2^12 (4-byte: one range when grown by 2) and 2^13,
    // random fills at 2^15 and 2^18 (2^18 x 64: by 2 only for the wider slots' 128 MiB)
    for (int wide = 0; wide < 2; ++wide) {
        const int W = wide ? 2 : 1, B = wide ? 50 : 30;
        for (u32 lg : {1u, 3u, 6u}) {
            build_cases(W, B, 1ull << 12, lg, false, cases);
            build_cases(W, B, 1ull << 13, lg, false, cases);
            // (4-byte slots grown by 2: the smallest old table that holds the long run next to two ranges)
            if (!wide && lg == 1) build_cases(W, B, 1ull << 14, lg, false, cases);
            build_cases(W, B, 1ull << 15, lg, true, cases);
            if (lg == 1 || !wide) build_cases(W, B, 1ull << 18, lg, true, cases);
        }
        // a random fill large enough that some range certainly spills (the host model says so)
        Case c;
        c.name = std::string("random fill at load 0.45 must spill, W=") + std::to_string(W);
        c.W = W, c.B = B, c.old_cap = 1ull << 18, c.lg = 1, c.want_spills = -2;
        random_keys(view_of(W, B, c.old_cap), B, (u64)(0.45 * (double)c.old_cap), 0x5EEDull + (u64)W, c.keys);
        cases.push_back(c);
    }
    // 8-byte slots into 4-byte slots, range by range
    for (u32 lg : {1u, 3u, 6u}) build_cases(1, 35, 1ull << 12, lg, false, cases);
    // one range (the old table has exactly `span` slots) and the window's clamp to the old table
    // (fewer than span + REBUILD_BLOCK old slots in two ranges)
    build_cases(2, 50, 1ull << 11, 1, false, cases);
    build_cases(2, 50, 1ull << 7, 6, false, cases);
    build_cases(1, 30, 1ull << 8, 6, false, cases);
    build_cases(1, 30, 1ull << 7, 6, false, cases);
    // fingerprint mode: CAS only
    for (u32 lg : {1u, 3u, 6u}) build_cases(1, 64, 1ull << 12, lg, false, cases);
    for (const Case& c : cases) {
        const std::string r = R.run(c);
        if (!r.empty()) return why = c.name + ": " + r, false;
    }
    if (R.long_runs != 0x3f) return why = "the long-run case was not built for every slot width and step", false;
    if (host_only) return true;
    // what the cases must have reached
    if (!R.by_ranges32 || !R.by_ranges64 || !R.by_cas || !R.mixed || !R.spilled)
        return why = "the cases did not reach every path (ranges32 " + std::to_string(R.by_ranges32) + ", ranges64 " +
                     std::to_string(R.by_ranges64) + ", CAS " + std::to_string(R.by_cas) + ", mixed widths " +
                     std::to_string(R.mixed) + ", spills " + std::to_string(R.spilled) + ")", false;
    const TableView f = view_of(1, 35, 1ull << 12), t = view_of(1, 35, 1ull << 13);
    if (f.s32 || !t.s32 || !rehash_by_ranges(f, t, 1, 1ull << 13)) return why = "B = 35 at 2^12 slots is no mixed-width pair", false;
    return true;
}

}  // namespace rehash_test
}  // namespace sr
