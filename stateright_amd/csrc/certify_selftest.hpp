// Self-test of the certificate kernels (sr_selftest_certify_gpu, include/stateright_gpu.h): before the
// certificate judges a check, it is judged itself.
//
// Arenas are built on the host by a sequential search in the reference's FIFO order (level 0 the init states
// reversed, a state keeps its first generator: parent rank and tag = rank * A + slot), tables by sequential
// linear probing through probe_key, 4-byte slots packed as the device stores them. Every case runs in both
// orders (FAST: the same arena without meta). Errors are planted into copies of a clean case; all of them keep
// every index in range but the deliberately out-of-range parent ranks, which the kernels must count and never
// load. Every counter of every case must equal cert_host, the plain host evaluation of the definitions
// (certify.hpp). Host only (device < 0): the cases are built, evaluated and cross-checked: a clean arena gives
// zeros and the count identities, every planted error moves the counter it was planted for.
//
// Models: LiveGraph with 1, 2 and 4 words (quotient slots of 4 and 8 bytes, repeated init states), Ladder(58, 8)
// (two mask words), a two-word IncrementLock, and CertHeap(n), a fixture with exactly n states for the sizes
// at which a grid goes wrong: 1, 63 .. 65, 255 .. 257, 3000 on a grid of 2 (several strides, a partial last
// one) and 131071 (a level of 65536).
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "certify.hpp"
#include "engine.hpp"

namespace sr {
namespace cert_test {

// States 0 .. n - 1 of a binary heap: slot 0 -> 2v + 1, slot 1 -> 2v + 2 (while below n); slot 2, enabled when
// 3 | v, -> v / 3 (an earlier state; a self-loop at 0), which apply refuses when 5 | v; slot 3 -> the first child
// of v's sibling, so that states have two generators in one level. sometimes "v mod 7 == 3".
struct CertHeap {
    static constexpr int W = 1, MW = 1, NPROPS = 1;
    u64 n;
    int max_actions() const { return 4; }
    int max_out_degree() const { return 4; }
    SR_HD static u64 sibling(u64 v) { return v & 1 ? v + 1 : v - 1; }
    SR_HD void enabled(const u64* s, u64* m) const {
        const u64 v = s[0];
        m[0] = (2 * v + 1 < n ? 1u : 0u) | (2 * v + 2 < n ? 2u : 0u) | (v % 3 == 0 ? 4u : 0u) | (v >= 1 && 2 * sibling(v) + 1 < n ? 8u : 0u);
    }
    SR_HD bool apply(const u64* s, int a, u64* o) const {
        const u64 v = s[0];
        if (a == 2 && v % 5 == 0) return false;
        o[0] = a == 0 ? 2 * v + 1 : a == 1 ? 2 * v + 2 : a == 2 ? v / 3 : 2 * sibling(v) + 1;
        return true;
    }
    SR_HD bool discovers(int, const u64* s) const { return s[0] % 7 == 3; }
    int init_states(u64* out) const { out[0] = 0; return 1; }
    int expectation(int) const { return SOMETIMES; }
    const char* prop_name(int) const { return "v mod 7 == 3"; }
};

template <class M>
struct Case {
    std::string name;
    M m;
    std::vector<u64> arena, tag;  // tag: per arena index (level 0: 0)
    std::vector<u32> apar;
    std::vector<u64> lstart;
    std::vector<u64> extra;       // states the table holds beyond the arena's (W words each)
    i64 omit = -1;                // an arena index whose state the table does not hold
    u32 grid = 0;
    u64 disc_index[32];
    const char* expect = nullptr; // the counter the case was planted for (nullptr: a clean case)
    u64 expect_exact = 0;         // != 0: its exact value
    std::function<void(u64*)> alien;  // writes a state no search reaches
};

template <class M>
inline Case<M> search(const M& m, const std::string& name, std::function<void(u64*)> alien, u32 grid = 0) {
    constexpr int W = M::W, MW = M::MW;
    Case<M> c;
    c.name = name, c.m = m, c.grid = grid, c.alien = alien;
    const u64 A = (u64)std::max(1, m.max_actions());
    const std::vector<u64> inits = init_states_of(m);
    const size_t k = inits.size() / W;
    std::map<std::vector<u64>, u64> seen;
    for (size_t i = 0; i < k; ++i) {
        const u64* s = &inits[(k - 1 - i) * W];
        seen.emplace(std::vector<u64>(s, s + W), i);
        c.arena.insert(c.arena.end(), s, s + W);
        c.apar.push_back(0xffffffffu);
        c.tag.push_back(0);
    }
    c.lstart = {0, (u64)k};
    for (size_t L = 0; c.lstart[L] < c.lstart[L + 1]; ++L) {
        for (u64 i = c.lstart[L]; i < c.lstart[L + 1]; ++i) {
            const std::vector<u64> s(&c.arena[i * W], &c.arena[i * W] + W);  // (a copy: the arena grows)
            u64 mask[MW], out[W];
            m.enabled(s.data(), mask);
            for (int a = 0; a < 64 * MW; ++a) {
                if (!(mask[a >> 6] >> (a & 63) & 1) || !m.apply(s.data(), a, out)) continue;
                if (!seen.emplace(std::vector<u64>(out, out + W), c.arena.size() / W).second) continue;
                c.arena.insert(c.arena.end(), out, out + W);
                c.apar.push_back((u32)(i - c.lstart[L]));
                c.tag.push_back((i - c.lstart[L]) * A + (u64)a);
            }
        }
        if (c.arena.size() / W == c.lstart.back()) break;
        c.lstart.push_back(c.arena.size() / W);
    }
    for (int p = 0; p < 32; ++p) c.disc_index[p] = ~0ull;
    for (int p = 0; p < M::NPROPS; ++p)
        for (u64 i = 0; i < c.lstart.back() && c.disc_index[p] == ~0ull; ++i)
            if (m.discovers(p, &c.arena[i * W])) c.disc_index[p] = i;
    return c;
}

template <class M>
inline u32 level_at(const Case<M>& c, u64 i) {
    u32 L = 0;
    while (c.lstart[L + 1] <= i) ++L;
    return L;
}

// The case's table: its arena's states but `omit`, then `extra`, by sequential linear probing.
template <class M>
inline CertHostTable table_of(const Case<M>& c, bool fifo) {
    constexpr int W = M::W;
    const u64 n = c.lstart.back();
    CertHostTable T;
    T.cap = std::max<u64>(64, min_table_cap(c.m));
    while (T.cap < 2 * (n + c.extra.size() / W) + 16) T.cap <<= 1;
    T.t = make_table_view(c.m, nullptr, nullptr, T.cap, true);
    T.v.assign(T.cap, 0);
    if (fifo) T.meta.assign(T.cap, META_UNSET);
    auto insert = [&](const u64* s, u64 meta) {
        const ProbeKey pk = probe_key(c.m, T.t, s);
        for (u64 d = 0; d < T.cap; ++d) {
            const u64 i = (pk.home + d) & T.t.mask, val = pk.tag + (T.t.qbits ? d : 0);
            if (T.v[i] == val) return;  // (a repeated init state)
            if (!T.v[i]) {
                T.v[i] = val;
                if (fifo) T.meta[i] = meta;
                return;
            }
        }
        throw Error(SR_ERR_ARG, "certificate self-test: a case does not fit its table");
    };
    for (u64 i = 0; i < n; ++i) {
        if ((i64)i == c.omit) continue;
        const u64 L = level_at(c, i);
        insert(&c.arena[i * W], L ? (L << META_SHIFT) | c.tag[i] : 0);
    }
    for (size_t e = 0; e < c.extra.size() / W; ++e) insert(&c.extra[e * W], ((u64)(c.lstart.size() - 1) << META_SHIFT) | e);
    return T;
}

template <class M>
inline CertInput input_of(const Case<M>& c, bool fifo) {
    CertInput in;
    in.lstart = c.lstart;
    in.fifo = fifo;
    in.explored_all = true;
    in.pmask = ((1u << M::NPROPS) - 1) & ~model_emask(c.m) & ~model_lmask(c.m) & ~model_smask(c.m);
    for (int p = 0; p < 32; ++p) in.disc_index[p] = c.disc_index[p];
    in.grid = c.grid;
    return in;
}

struct Field {
    const char* name;
    uint64_t sr_certificate::*at;
};
inline const std::vector<Field>& fields() {
    static const std::vector<Field> f = {
        {"states", &sr_certificate::states}, {"levels", &sr_certificate::levels}, {"inits", &sr_certificate::inits},
        {"repeated_inits", &sr_certificate::repeated_inits}, {"roots_wrong", &sr_certificate::roots_wrong},
        {"map_missing", &sr_certificate::map_missing}, {"tree_range", &sr_certificate::tree_range},
        {"tree_edge", &sr_certificate::tree_edge}, {"tree_slot", &sr_certificate::tree_slot}, {"edges", &sr_certificate::edges},
        {"repeated_edges", &sr_certificate::repeated_edges}, {"closure_missing", &sr_certificate::closure_missing},
        {"closure_unlisted", &sr_certificate::closure_unlisted}, {"closure_late", &sr_certificate::closure_late},
        {"fifo_not_first", &sr_certificate::fifo_not_first}, {"fifo_order", &sr_certificate::fifo_order}};
    return f;
}
inline u64 field(const sr_certificate& c, const std::string& name) {
    for (const Field& f : fields())
        if (name == f.name) return c.*(f.at);
    throw Error(SR_ERR_ARG, "certificate self-test: no counter " + name);
}
inline bool is_error_field(const std::string& n) {
    return n != "states" && n != "levels" && n != "inits" && n != "repeated_inits" && n != "edges" && n != "repeated_edges";
}

struct Runner {
    int dev;
    bool host_only;
    hipStream_t s = nullptr;
    u64 cases = 0, planted = 0;

    template <class T>
    void upload(DBuf<T>& d, const std::vector<T>& h) {
        d.alloc(dev, h.size());
        if (!h.empty()) SR_HIP(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    }

    // Empty: the case passed in this order.
    template <class M>
    std::string run(const Case<M>& c, bool fifo) {
        ++cases;
        const CertHostTable T = table_of(c, fifo);
        const CertInput in = input_of(c, fifo);
        const sr_certificate want = cert_host(c.m, T, c.arena, c.apar, in);
        // the host evaluation against what the case was built for
        if (!c.expect) {
            for (const Field& f : fields())
                if (is_error_field(f.name) && want.*(f.at)) return std::string("a clean case counts ") + f.name + " on the host";
            for (int p = 0; p < M::NPROPS; ++p)
                if (want.disc_wrong[p] || ((in.pmask >> p & 1) && want.first_index[p] != c.disc_index[p]))
                    return "a clean case's first discovering index is not the search's";
        } else {
            ++planted;
            const u64 got = field(want, c.expect);
            const bool fifo_only = std::string(c.expect) == "fifo_order" || std::string(c.expect) == "fifo_not_first" ||
                                   std::string(c.expect) == "tree_slot";
            if (fifo_only && !fifo) {
                if (got) return std::string("FAST order counts ") + c.expect;
            } else if (!got || (c.expect_exact && got != c.expect_exact)) {
                return std::string("the host evaluation counts ") + std::to_string(got) + " for " + c.expect + ", which the case was planted for";
            }
        }
        if (host_only) return "";

        DBuf<u64> keys, meta, arena;
        DBuf<u32> apar;
        std::vector<u64> packed = T.v;
        if (T.t.s32) {
            packed.assign((T.cap + 1) / 2, 0);
            for (u64 i = 0; i < T.cap; ++i) packed[i / 2] |= (T.v[i] & 0xffffffffull) << (32 * (i & 1));
        }
        upload(keys, packed);
        if (fifo) upload(meta, T.meta);
        upload(arena, c.arena);
        upload(apar, c.apar);
        TableView t = T.t;
        t.keys = keys.p;
        t.meta = fifo ? meta.p : nullptr;
        const sr_certificate got = cert_device(c.m, t, T.cap, arena.p, apar.p, in, dev, s);
        if (!got.ran || got.skipped) return "the pass did not run";
        if (got.fifo != want.fifo || got.explored_all != want.explored_all || got.pmask != want.pmask || got.nprops != want.nprops)
            return "the certificate's header differs from the host evaluation's";
        for (const Field& f : fields())
            if (got.*(f.at) != want.*(f.at))
                return std::string(f.name) + " is " + std::to_string(got.*(f.at)) + " on the device, " + std::to_string(want.*(f.at)) + " by the host evaluation";
        for (int p = 0; p < M::NPROPS; ++p)
            if (got.holds[p] != want.holds[p] || got.first_index[p] != want.first_index[p] || got.disc_wrong[p] != want.disc_wrong[p] ||
                got.disc_index[p] != want.disc_index[p] || got.first_level[p] != want.first_level[p] || got.disc_level[p] != want.disc_level[p])
                return "the figures of property " + std::to_string(p) + " differ from the host evaluation's";
        return "";
    }

    template <class M>
    bool both(const Case<M>& c, std::string& why) {
        for (int fifo = 0; fifo < 2; ++fifo) {
            const std::string r = run(c, fifo != 0);
            if (!r.empty()) return why = c.name + (fifo ? " (FIFO): " : " (FAST): ") + r, false;
        }
        return true;
    }
};

// The planted errors of one clean case.
template <class M>
inline bool plant_all(Runner& R, const Case<M>& clean, std::string& why) {
    constexpr int W = M::W, MW = M::MW;
    const u64 n = clean.lstart.back(), A = (u64)std::max(1, clean.m.max_actions());
    const size_t nlevels = clean.lstart.size() - 1;
    if (nlevels < 4 || clean.lstart[2] - clean.lstart[1] < 2 || clean.lstart[3] - clean.lstart[2] < 2)
        return why = clean.name + ": too small to plant errors in", false;
    auto fresh = [&](const char* what, const char* expect, u64 exact = 0) {
        Case<M> c = clean;
        c.name = clean.name + ", " + what;
        c.expect = expect, c.expect_exact = exact;
        return c;
    };
    auto size_of = [&](size_t L) { return clean.lstart[L + 1] - clean.lstart[L]; };
    {   // a parent rank pointing at a non-generator (the next rank round the parent's level, until it is none)
        bool done = false;
        for (u64 i = clean.lstart[2]; i < n && !done; ++i) {
            const u32 L = level_at(clean, i);
            Case<M> c = fresh("a parent rank pointing at a non-generator", "tree_edge", 1);
            c.apar[i] = (u32)((c.apar[i] + 1) % size_of(L - 1));
            const u64* par = &c.arena[(c.lstart[L - 1] + c.apar[i]) * W];
            u64 mask[MW], out[W];
            clean.m.enabled(par, mask);
            bool gen = false;
            for (int a = 0; a < 64 * MW; ++a)
                gen = gen || ((mask[a >> 6] >> (a & 63) & 1) && clean.m.apply(par, a, out) && std::equal(out, out + W, &c.arena[i * W]));
            if (gen) continue;
            done = true;
            if (!R.both(c, why)) return false;
        }
        if (!done) return why = clean.name + ": every neighbouring rank is a generator", false;
    }
    {   // a rank equal to the level size, and one equal to 2^32 - 2: counted, never loaded
        Case<M> c = fresh("parent ranks past the previous level", "tree_range", 2);
        c.apar[c.lstart[1]] = (u32)size_of(0);
        c.apar[n - 1] = 0xfffffffeu;
        if (!R.both(c, why)) return false;
    }
    {   // a state removed from the table
        Case<M> c = fresh("a state removed from the table", "map_missing", 1);
        c.omit = (i64)c.lstart[1];
        if (!R.both(c, why)) return false;
        c.expect = "closure_missing", c.expect_exact = 0;
        if (!R.both(c, why)) return false;
    }
    {   // a table entry no arena state owns: the last state leaves the arena and stays in the table
        Case<M> c = fresh("a table entry no arena state owns", "closure_unlisted");
        c.extra.assign(c.arena.end() - W, c.arena.end());
        c.arena.resize((n - 1) * W), c.apar.pop_back(), c.tag.pop_back();
        c.lstart.back() -= 1;
        if (c.lstart.back() == c.lstart[nlevels - 1]) c.lstart.pop_back();
        for (int p = 0; p < 32; ++p)
            if (c.disc_index[p] == n - 1) c.disc_index[p] = ~0ull;
        if (!R.both(c, why)) return false;
    }
    {   // a state moved one level down: the last state of level 1 becomes the first of level 2
        Case<M> c = fresh("a state moved one level down", "closure_late");
        c.lstart[2] -= 1;
        if (!R.both(c, why)) return false;
    }
    {   // an unreachable state appended to the last level
        Case<M> c = fresh("an unreachable state appended to a level", "tree_edge", 1);
        u64 s[W];
        c.alien(s);
        c.arena.insert(c.arena.end(), s, s + W);
        c.apar.push_back(0), c.tag.push_back(0);
        c.lstart.back() += 1;
        if (!R.both(c, why)) return false;
    }
    {   // two neighbours of a level swapped (FAST order: their children's parent ranks go wrong, the order does not count)
        Case<M> c = fresh("two neighbours of a level swapped", "fifo_order");
        const u64 i = c.lstart[2];
        for (int x = 0; x < W; ++x) std::swap(c.arena[i * W + x], c.arena[(i + 1) * W + x]);
        std::swap(c.apar[i], c.apar[i + 1]), std::swap(c.tag[i], c.tag[i + 1]);
        if (!R.both(c, why)) return false;
    }
    {   // a tag naming a later generator (and the parent rank with it: a valid tree, so FAST order counts nothing)
        bool done = false;
        for (u64 i = clean.lstart[2]; i < n && !done; ++i) {
            const u32 L = level_at(clean, i);
            for (u64 r = clean.apar[i] + 1; r < size_of(L - 1) && !done; ++r) {
                const u64* par = &clean.arena[(clean.lstart[L - 1] + r) * W];
                u64 mask[MW], out[W];
                clean.m.enabled(par, mask);
                for (int a = 0; a < 64 * MW && !done; ++a) {
                    if (!(mask[a >> 6] >> (a & 63) & 1) || !clean.m.apply(par, a, out) || !std::equal(out, out + W, &clean.arena[i * W])) continue;
                    Case<M> c = fresh("a tag naming a later generator", "fifo_not_first");
                    c.apar[i] = (u32)r, c.tag[i] = r * A + (u64)a;
                    done = true;
                    if (!R.both(c, why)) return false;
                }
            }
        }
        if (!done) return why = clean.name + ": no state with two generators in one level", false;
    }
    {   // the first init state replaced
        Case<M> c = fresh("the first init state replaced", "roots_wrong", 1);
        u64 s[W];
        c.alien(s);
        std::copy(s, s + W, c.arena.begin());
        if (!R.both(c, why)) return false;
    }
    return true;
}

template <class M>
inline bool clean_case(Runner& R, const Case<M>& c, std::string& why) {
    constexpr int W = M::W;
    // the identities of a clean arena, on the host evaluation: distinct states, and edges from a second count
    std::map<std::vector<u64>, int> distinct;
    for (u64 i = 0; i < c.lstart.back(); ++i) distinct[std::vector<u64>(&c.arena[i * W], &c.arena[i * W] + W)]++;
    const sr_certificate h = cert_host(c.m, table_of(c, false), c.arena, c.apar, input_of(c, false));
    if (h.states - h.repeated_inits != distinct.size()) return why = c.name + ": states - repeated_inits is not the number of distinct states", false;
    u64 edges = 0;
    for (const auto& kv : distinct)
        for_each_successor(c.m, kv.first.data(), [&](int, const u64*) { ++edges; });
    if (h.edges != edges) return why = c.name + ": edges is not the sum of the distinct states' successors", false;
    return R.both(c, why);
}

inline bool run_all(int device, std::string& why, bool host_only = false) {
    if (!host_only) SR_HIP(hipSetDevice(device));
    Runner R{device, host_only};
    auto live_alien = [](auto m) {
        return [m](u64* s) { decltype(m)::pack((1ull << m.n_bits) + 3, s); };
    };
    {
        const LiveGraphT<1> m{10, 3, 7, 0, 5, 3, 1};
        if (!clean_case(R, search(m, "LiveGraph(10, 3) one word", live_alien(m)), why)) return false;
    }
    {
        const LiveGraphT<2> m{10, 3, 11, 0, 5, 3, 1};
        const auto c = search(m, "LiveGraph(10, 3) two words", live_alien(m));
        if (!clean_case(R, c, why) || !plant_all(R, c, why)) return false;
    }
    {
        const LiveGraphT<4> m{9, 2, 5, 0, 4, 2, 0};
        if (!clean_case(R, search(m, "LiveGraph(9, 2) four words", live_alien(m)), why)) return false;
    }
    {
        const Ladder m{58, 8};
        const auto c = search(m, "Ladder(58, 8)", [](u64* s) { s[0] = 63; });
        if (c.lstart.back() != 59 * 256) return why = "Ladder(58, 8) does not have 59 * 256 states", false;
        if (!clean_case(R, c, why) || !plant_all(R, c, why)) return false;
    }
    {
        const IncrementLock<2> m{4};
        if (!clean_case(R, search(m, "IncrementLock(4) on two words", [](u64* s) { s[0] = 15, s[1] = 0; }), why)) return false;
    }
    for (u64 n : {1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 3000ull, 131071ull}) {
        const CertHeap m{n};
        const auto c = search(m, "CertHeap(" + std::to_string(n) + ")", [n](u64* s) { s[0] = n + 5; }, n == 3000 ? 2u : 0u);
        if (c.lstart.back() != n) return why = c.name + " does not have n states", false;
        if (n == 131071 && c.lstart.back() - c.lstart[c.lstart.size() - 2] != 65536) return why = c.name + " has no level of 65536 states", false;
        if (!clean_case(R, c, why)) return false;
        if (n == 3000 && !plant_all(R, c, why)) return false;
    }
    if (R.planted < 3 * 2 * 9) return why = "fewer planted cases ran than the three models' nine errors in both orders", false;
    return true;
}

}  // namespace cert_test
}  // namespace sr
