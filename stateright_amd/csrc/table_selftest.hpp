// Host-only self-test of the visited set's encodings as make_table_view chooses them, walked
// through growth (sr_selftest_table_growth, include/stateright_gpu.h). Nothing is allocated: the
// views carry no memory, and every check is arithmetic on keys, homes and slot values.
//
// The models are Spread<W> fixtures (models.hpp) of every key width B; their key is words 0 and 1
// of the state, so a random key below 2^B is a state.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace sr {

// What make_table_view, min_table_cap and the filter rules give a model of W words with a key of
// B bits at `cap` slots (sr_table_encoding).
struct TableEncoding {
    u32 qbits, dbits, bbits, plimit, s32;
    u32 filter;       // 0: no duplicate filter, 1: 8-byte entries, 2: compact (4-byte) entries
    u32 filter_log2;  // its entries (log2)
    u32 min_cap_log2;
};
template <int W>
inline TableEncoding table_encoding_of(int B, u64 cap) {
    const Spread<W> m{B, 1, 0, 0};
    const TableView v = make_table_view(m, nullptr, nullptr, cap, true);
    TableEncoding e{v.qbits, v.dbits, v.bbits, v.plimit, v.s32, 0, 0, 0};
    u32 fl = filter_exact(m) ? default_filter_log2<W>() : 0;
    e.filter = fl ? 1 : 0;
    if (fl && filter_compact_ok(m, fl + 1)) fl += 1, e.filter = 2;
    e.filter_log2 = fl;
    while ((1ull << e.min_cap_log2) < min_table_cap(m)) ++e.min_cap_log2;
    return e;
}

namespace growth_test {

constexpr int NKEYS = 4096;
constexpr u32 MAX_LOG2 = 40;  // the smallest table of a 96-bit key on two words

struct Sample {
    u64 w[4];
};

inline std::string u128_text(u128 x) { return std::to_string((u64)(x >> 64)) + ":" + std::to_string((u64)x); }

// Sorted pairs hold a duplicate?
inline bool has_duplicate(std::vector<std::pair<u64, u64>>& v) {
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}

template <int W>
bool check_model(int B, std::string& why) {
    const Spread<W> m{B, 1, 0, 0};
    auto where = [&](u64 cap) {
        u32 k = 0;
        while ((1ull << k) < cap) ++k;
        return " at W=" + std::to_string(W) + " B=" + std::to_string(B) + " cap=2^" + std::to_string(k);
    };
    // distinct random keys below 2^B (0 and 2^B - 1 among them); the further words are random too
    std::vector<Sample> keys;
    {
        const u128 top = B >= 128 ? ~(u128)0 : ((u128)1 << B) - 1;
        u64 r = 0x243F6A8885A308D3ull + (u64)B * 0x9E3779B97F4A7C15ull + (u64)W;
        const u64 want = B >= 13 ? (u64)NKEYS : 1ull << B;  // every key of a small key space
        for (u64 i = 0; i < want; ++i) {
            r = fmix64(r + 0x9E3779B97F4A7C15ull);
            const u64 r2 = fmix64(r ^ 0xABCDEFull);
            u128 key = (((u128)r2 << 64) | r) & top;
            if (i == 0) key = 0;
            if (i == 1) key = top;
            if (B < 13) key = i;
            if (W == 1 && B == 64 && (u64)key == 0x8000000000000000ull) continue;  // fingerprint<1> maps it to 0
            keys.push_back(Sample{{(u64)key, W >= 2 ? (u64)(key >> 64) : 0, fmix64(r2 + 1), fmix64(r2 + 2)}});
        }
        auto less = [](const Sample& a, const Sample& b) { return a.w[1] != b.w[1] ? a.w[1] < b.w[1] : a.w[0] < b.w[0]; };
        std::sort(keys.begin(), keys.end(), less);
        keys.erase(std::unique(keys.begin(), keys.end(), [](const Sample& a, const Sample& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1]; }),
                   keys.end());
    }
    // the mode is a property of (W, B) alone, stated here apart from quotient_model
    const bool want_quot = W == 1 ? B <= 62 : B <= 96;
    if (quotient_model(m) != want_quot) return why = "quotient_model differs from the documented rule at W=" + std::to_string(W) + " B=" + std::to_string(B), false;
    const bool quot = quotient_model(m);
    const u64 cap0 = std::max<u64>(min_table_cap(m), 1ull << 10);
    const bool fexact = filter_exact(m);
    std::vector<std::pair<u64, u64>> pairs;
    for (u64 cap = cap0; cap <= (1ull << MAX_LOG2); cap *= 2) {
        const TableView t = make_table_view(m, nullptr, nullptr, cap, true);
        if (t.mask != cap - 1) return why = "mask is not cap - 1" + where(cap), false;
        if ((t.qbits != 0) != quot)
            return why = std::string("the table is in ") + (t.qbits ? "quotient" : "fingerprint") + " mode, the model's mode is " +
                         (quot ? "quotient" : "fingerprint") + where(cap), false;
        if (t.qbits) {
            const u32 width = t.s32 ? 32 : 64;
            if (t.bbits != (u32)B || t.qbits + t.dbits != width || t.dbits < 8 || t.qbits > 56)
                return why = "slot fields do not fill the slot" + where(cap), false;
            if (t.plimit != encoding_probe_limit(t.qbits, t.dbits) || t.plimit < 1)
                return why = "probe limit differs from the encoding's" + where(cap), false;
        } else if (t.s32 || t.plimit != (u32)MAX_PROBE) {
            return why = "fingerprint mode with narrow slots or a short probe limit" + where(cap), false;
        }
        pairs.clear();
        std::vector<std::pair<u64, u64>> fkeys;
        for (const Sample& s : keys) {
            const ProbeKey pk = probe_key(m, t, s.w);
            if (pk.home > t.mask) return why = "home slot past the table" + where(cap), false;
            const u64 step = probe_step(t);
            for (u64 d : {(u64)0, (u64)t.plimit - 1}) {
                const u64 v = pk.tag + d * step;
                if (!v) return why = "a slot value of 0 (vacant)" + where(cap), false;
                if (t.s32 && v >> 32) return why = "slot value does not fit 32 bits" + where(cap), false;
                if (t.qbits) {
                    const u128 h = quot_hash(m, t, s.w);
                    if (B < 128 && h >> B) return why = "permuted key past 2^B" + where(cap), false;
                    if (quot_decode(t, (pk.home + d) & t.mask, v) != h)
                        return why = "slot value at displacement " + std::to_string(d) + " does not decode to the permuted key " +
                                     u128_text(h) + where(cap), false;
                } else if (v != state_fp<Spread<W>>(s.w) || pk.home != (v & t.mask)) {
                    return why = "fingerprint slot is not the state's fingerprint" + where(cap), false;
                }
            }
            pairs.emplace_back(pk.home, pk.tag);
            const u64 fk = filter_key(t, pk);
            fkeys.emplace_back(fk, 0);
            if (fexact && t.qbits && (u128)fk != quot_hash(m, t, s.w) + 1)
                return why = "filter key is not the permuted key + 1" + where(cap), false;
            if (fexact && !fk) return why = "filter key 0 (the empty entry)" + where(cap), false;
            const u32 fl = default_filter_log2<W>() + 1;
            if (filter_compact_ok(m, fl) && (!t.qbits || (fk >> fl) >> 31))
                return why = "compact filter entry loses bits of the filter key" + where(cap), false;
        }
        // distinct keys: distinct (home, slot value) in quotient mode and for one-word states
        if ((t.qbits || W == 1) && has_duplicate(pairs)) return why = "two keys share home and slot value" + where(cap), false;
        if (fexact && has_duplicate(fkeys)) return why = "filter key is not injective" + where(cap), false;
        // growth by 2, 8 and 64
        for (u32 lg : {1u, 3u, 6u}) {
            const u64 cap2 = cap << lg;
            if (cap2 > (1ull << MAX_LOG2)) continue;
            const TableView to = make_table_view(m, nullptr, nullptr, cap2, true);
            auto at = [&]() { return where(cap) + " -> 2^" + std::to_string(__builtin_ctzll(cap2)); };
            if ((t.qbits != 0) != (to.qbits != 0))
                return why = std::string("growth switches the mode from ") + (t.qbits ? "quotient to fingerprint" : "fingerprint to quotient") +
                             at(), false;
            const bool ranges = rehash_by_ranges(t, to, lg, cap2);
            if (ranges) {
                const u64 S = to.s32 ? rebuild_slots<u32>() : rebuild_slots<u64>();
                if ((S >> lg) == 0 || cap2 % S || (cap2 / S) >> 32) return why = "rehash_ranges' ranges do not tile the table" + at(), false;
            }
            for (const Sample& s : keys) {
                const ProbeKey pf = probe_key(m, t, s.w), want = probe_key(m, to, s.w);
                for (u64 d : {(u64)0, std::min<u64>(t.plimit - 1, 5)}) {
                    const ProbeKey got = reprobe(t, to, (pf.home + d) & t.mask, pf.tag + d * probe_step(t));
                    if (got.home != want.home || got.tag != want.tag)
                        return why = "reprobe gives home " + std::to_string(got.home) + " value " + std::to_string(got.tag) +
                                     ", probe_key " + std::to_string(want.home) + " / " + std::to_string(want.tag) + at(), false;
                }
                // the workgroup of new slots [r S, (r + 1) S) takes the old homes [r S >> lg, (r + 1) S >> lg)
                if (ranges && (want.home >> lg) != pf.home) return why = "rehash by ranges, but new home >> lg is not the old home" + at(), false;
            }
        }
    }
    return true;
}

// Key widths of W words: all of them for one and two words, and the tested ones for four (the
// encodings are those of two).
template <int W>
bool check_words(std::string& why) {
    for (int B = 2; B <= std::min(64 * W, 128); ++B) {
        if (W == 4 && B != 18 && B != 24 && B != 50 && B != 60 && B != 78 && B != 79 && B != 96 && B != 97 && B != 120 && B != 128) continue;
        const Spread<W> m{B, 1, 0, 0};
        if (min_table_cap(m) > (1ull << MAX_LOG2)) continue;
        if (!check_model<W>(B, why)) return false;
    }
    return true;
}

}  // namespace growth_test

inline bool table_growth_selftest(std::string& why) {
    return growth_test::check_words<1>(why) && growth_test::check_words<2>(why) && growth_test::check_words<4>(why);
}

}  // namespace sr
