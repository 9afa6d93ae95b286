// The ABD linearizable register past actor.hpp's AbdSys (3 clients, 3 servers, 8 network slots):
// `AbdWideSysT<KK>`, the same actors (examples/linearizable-register.rs, oracle/actor.hpp AbdSys)
// for 1-6 clients, 1-4 servers and at most 8 actors, with KK = 16 or 32 network slots, and
// `abd_slots`, which picks the encoding of a (client_count, server_count).
//
// State: AW = 6 words, then the network (actor.hpp ActorGpu).
//   word 0     bits [0, 32): the high word of the history; bits 51..63 are ActorGpu's
//   word 1     the low word of the history (paxos.hpp PaxosHist: phases, returned values, Get `last`
//              vectors; 5C + 2C(C-1) <= 90 bits). A client's `awaiting` and `op_count` follow from
//              its history phase (0: awaiting PutOk(id), 1: awaiting GetOk(2 id), 2: done), as in
//              SingleCopySys, so no client field and no host-interned history closure.
//   word 2 + i server i (21 + 10 S <= 61 bits): seq clock [0,3) (at most C <= 6 writes), seq id [3,6),
//              val [6,9) ('\0' 0, 'A'.. 1..6), phase [9,11), request id [11,15) ((op_count + 1) * id
//              <= 14), requester [15,18), write/read [18,21) (0 None, else val + 1), then from bit 21
//              EITHER the phase-1 response of server j at [21 + 10j, 31 + 10j) (present, clock 3, id
//              3, val 3) OR the phase-2 acks mask [21, 21 + S): the two are never live together, and
//              each phase change clears the whole run, so equal states are equal words.
// Message (16 of MSG_BITS, the oracle's key order (kind, req, seq, val)): kind << 13 | req << 9 |
// clock << 6 | id << 3 | val.
#pragma once
#include <cstdlib>

#include "actor.hpp"

namespace sr {
namespace act {

// The largest network of the ABD register with C clients and S servers, in envelopes. A client has
// one operation in flight (its Put, then its Get), run by one coordinator in two phases. Phase 1
// sends S - 1 Queries, and the coordinator moves on at a majority of responses, its own included,
// so d = S - majority AckQueries arrive late. A late AckQuery is a no-op delivery (model.rs
// `is_no_op`), which the non-duplicating network never removes: it stays for the rest of the check.
// Phase 2 leaves d late AckRecords the same way. The network of one client peaks in phase 2 of its
// Get: 2d late replies of the Put, d late AckQueries of the Get, and the S - 1 Records (or their
// AckRecords) in flight, 3d + S - 1; it ends with 4d late replies, and it holds at least the
// client's own request or reply. The clients' envelopes are distinct (the request id is a multiple
// of the client's id), so the peaks add up. The CPU oracle attains the bound exactly on every full
// space measured: (1,3) 5, (1,4) 6, (1,5) 10, (3,2) 3, (4,2) 4 (tests/test_abd_wide_host.py pins
// the first, second and fourth).
constexpr int abd_net_bound(int C, int S) {
    const int d = S - (S / 2 + 1);
    const int a = 3 * d + S - 1, b = 4 * d;
    const int per_client = a > b ? (a > 1 ? a : 1) : (b > 1 ? b : 1);
    return C * per_client;
}

constexpr int ABD_MAX_CLIENTS = 6, ABD_MAX_SERVERS = 4, ABD_MAX_ACTORS = 8;

// The network slots of the encoding that checks ABD (C, S): 8 = AbdSys (actor.hpp, C <= 3, S <= 3
// and the bound within its 8 slots; those states and fingerprints are what they always were), 16 =
// AbdWideSysT<16>, 32 = AbdWideSysT<32>. SR_ABD_SLOTS=8|16|32 forces one (for tests: it may be
// below the bound, and the check then ends with the encoding error; 8 still needs C, S <= 3).
inline int abd_slots(int C, int S) {
    if (C < 1 || C > ABD_MAX_CLIENTS || S < 1 || S > ABD_MAX_SERVERS || C + S > ABD_MAX_ACTORS)
        throw Error(SR_ERR_UNSUPPORTED,
                    "abd: client_count in 1..=6, server_count in 1..=4, client_count + server_count <= 8");
    const int bound = abd_net_bound(C, S);
    int slots = C <= 3 && S <= 3 && bound <= 8 ? 8 : bound <= 16 ? 16 : 32;
    if (const char* e = std::getenv("SR_ABD_SLOTS")) {
        const int v = std::atoi(e);
        if (v != 8 && v != 16 && v != 32) throw Error(SR_ERR_ARG, "SR_ABD_SLOTS must be 8, 16 or 32");
        if (v == 8 && (C > 3 || S > 3))
            throw Error(SR_ERR_UNSUPPORTED, "SR_ABD_SLOTS=8: the 8-slot encoding holds client_count and server_count in 1..=3");
        slots = v;
    }
    return slots;
}

template <int KK>
struct AbdWideSysT {
    static constexpr int K = KK, AW = 6, NACT = 8, NPROPS = 2, NET = KK;
    static constexpr const char* NAME = "abd";
    static_assert(KK == 16 || KK == 32, "the oracle describes 16 envelopes; 32 slots hold every accepted (C, S)");
    static constexpr int SRV = 2, MAXS = ABD_MAX_SERVERS;
    static constexpr int RSP = 21, RW = 10;  // the phase-1 responses / the phase-2 acks mask
    enum Kind : u32 { PUT, GET, PUTOK, GETOK, QUERY, ACKQUERY, RECORD, ACKRECORD };
    u32 S = 2, C = 2;
    bool lossy = false, duplicating = false;

    static AbdWideSysT make(int clients, int servers) {
        (void)abd_slots(clients, servers);  // the limits
        AbdWideSysT m;
        m.C = (u32)clients;
        m.S = (u32)servers;
        return m;
    }
    static SR_HD u32 msg(u32 kind, u32 req, u32 clock, u32 id, u32 val) { return kind << 13 | req << 9 | clock << 6 | id << 3 | val; }
    static SR_HD u32 getf(u64 w, int off, int n) { return (u32)(w >> off & ((1ull << n) - 1)); }
    static SR_HD u64 setf(u64 w, int off, int n, u32 v) { return (w & ~(((1ull << n) - 1) << off)) | (u64)v << off; }
    static SR_HD u32 rsp(u32 clock, u32 id, u32 val) { return 1u | clock << 1 | id << 4 | val << 7; }
    SR_HD u32 majority() const { return S / 2 + 1; }
    SR_HD u32 nact() const { return S + C; }
    SR_HD PaxosHist hs() const {
        PaxosHist h;
        h.C = C;
        return h;
    }
    static SR_HD u64 hist_lo(const u64* s) { return s[1]; }
    static SR_HD u64 hist_hi(const u64* s) { return s[0] & 0xffffffffull; }
    static SR_HD void hist_set(u64* o, u64 lo, u64 hi) {
        o[1] = lo;
        o[0] = (o[0] & ~0xffffffffull) | hi;
    }
    // server id's word, by a compile-time index (a state word indexed at run time goes to scratch)
    static SR_HD u64 server(const u64* o, u32 id) {
        u64 w = 0;
#pragma unroll
        for (u32 i = 0; i < (u32)MAXS; ++i) w = i == id ? o[SRV + i] : w;
        return w;
    }
    static SR_HD void set_server(u64* o, u32 id, u64 w) {
#pragma unroll
        for (u32 i = 0; i < (u32)MAXS; ++i) o[SRV + i] = i == id ? w : o[SRV + i];
    }

    SR_HD void init_network(Out&, u32&) const {}
    SR_HD void on_start(u64* o, u32 id, Out& out) const {
        if (id < S) {  // AbdActor::on_start: seq (0, id), val '\0', phase None
            set_server(o, id, (u64)id << 3);
            return;
        }
        // RegisterActor::Client::on_start, put_count 1 (src/actor/register.rs:130-160): history phase 0
        if (id < S + C) out.send(id % S, msg(PUT, id, 0, 0, id - S + 1));  // Put(1 x id, 'A' + index)
    }
    SR_HD bool on_msg(u64* o, u32 id, u32 src, u32 m, Out& out) const {
        const u32 kind = m >> 13, req = m >> 9 & 15, mclock = m >> 6 & 7, mid = m >> 3 & 7, mval = m & 7;
        if (id >= S) {  // RegisterActor::Client::on_msg (register.rs:170-200): the phase is the awaited reply
            const u32 ph = hs().phase(hist_lo(o), hist_hi(o), id - S);
            if (ph == 0 && kind == PUTOK && req == id) {
                out.send((id + 1) % S, msg(GET, 2 * id, 0, 0, 0));  // Get((op_count + 1) x id) to (id + op_count) % S
                return true;
            }
            return ph == 1 && kind == GETOK && req == 2 * id;
        }
        // AbdActor::on_msg (examples/linearizable-register.rs:66-173)
        u64 w = server(o, id);
        const u32 clock = getf(w, 0, 3), sid = getf(w, 3, 3), val = getf(w, 6, 3), phase = getf(w, 9, 2);
        const u32 preq = getf(w, 11, 4), requester = getf(w, 15, 3), wr = getf(w, 18, 3);
        constexpr u64 LOW = (1ull << RSP) - 1;  // everything below the responses / acks
        switch (kind) {
            case PUT:
            case GET: {
                if (phase != 0) return false;
#pragma unroll
                for (u32 p = 0; p < (u32)MAXS; ++p)
                    if (p < S && p != id) out.send(p, msg(QUERY, req, 0, 0, 0));
                w = (w & 511) | 1ull << 9 | (u64)req << 11 | (u64)src << 15 | (u64)(kind == PUT ? mval + 1 : 0) << 18;
                w |= (u64)rsp(clock, sid, val) << (RSP + RW * (int)id);
                set_server(o, id, w);
                return true;
            }
            case QUERY:
                out.send(src, msg(ACKQUERY, req, clock, sid, val));
                return false;
            case ACKQUERY: {
                if (!(phase == 1 && preq == req)) return false;
                w = setf(w, RSP + RW * (int)src, RW, rsp(mclock, mid, mval));
                u32 count = 0, bclock = 0, bid = 0, bval = 0;
                bool first = true;
#pragma unroll
                for (u32 j = 0; j < (u32)MAXS; ++j) {
                    const u32 r = getf(w, RSP + RW * (int)j, RW);
                    if (j >= S || !(r & 1)) continue;
                    ++count;
                    const u32 rc = r >> 1 & 7, ri = r >> 4 & 7, rv = r >> 7 & 7;
                    if (first || rc > bclock || (rc == bclock && ri > bid)) bclock = rc, bid = ri, bval = rv;  // max seq
                    first = false;
                }
                if (count == majority()) {
                    u32 nclock = bclock, nid = bid, nval = bval, read = 0;
                    if (wr) {  // write: seq = (seq.0 + 1, id), the written value
                        nclock = bclock + 1;
                        nid = id;
                        nval = wr - 1;
                    } else {
                        read = bval + 1;
                    }
#pragma unroll
                    for (u32 p = 0; p < (u32)MAXS; ++p)
                        if (p < S && p != id) out.send(p, msg(RECORD, preq, nclock, nid, nval));
                    if (nclock > clock || (nclock == clock && nid > sid)) w = (w & ~511ull) | nclock | nid << 3 | nval << 6;  // self Record
                    w = setf(w, 9, 2, 2);
                    w = setf(w, 18, 3, read);
                    w = (w & LOW) | 1ull << (RSP + (int)id);  // the responses go; self AckRecord
                }
                set_server(o, id, w);
                return true;  // `state.to_mut()` before the quorum test
            }
            case RECORD:
                out.send(src, msg(ACKRECORD, req, 0, 0, 0));
                if (mclock > clock || (mclock == clock && mid > sid)) {
                    set_server(o, id, (w & ~511ull) | mclock | mid << 3 | mval << 6);
                    return true;
                }
                return false;
            case ACKRECORD: {
                const u32 acks = getf(w, RSP, MAXS);
                if (!(phase == 2 && preq == req && !(acks >> src & 1))) return false;
                const u32 nacks = acks | 1u << src;
                w = setf(w, RSP, MAXS, nacks);
                if ((u32)__builtin_popcount(nacks) == majority()) {
                    if (wr) out.send(requester, msg(GETOK, preq, 0, 0, wr - 1));
                    else out.send(requester, msg(PUTOK, preq, 0, 0, 0));
                    w &= 511;  // phase None
                }
                set_server(o, id, w);
                return true;
            }
            default:
                return false;
        }
    }
    SR_HD bool on_timeout(u64*, u32, Out&) const { return false; }
    // RegisterMsg::record_returns / record_invocations (src/actor/register.rs:37-87) on the history
    // field, as SingleCopySys: PutOk returns WriteOk and the client's Get invocation follows in the
    // same delivery; GetOk(v) returns ReadOk(v).
    SR_HD void record_in(u64* o, u32, u32 dst, u32 m) const {
        const u32 kind = m >> 13;
        if (dst < S || (kind != PUTOK && kind != GETOK)) return;
        const u32 c = dst - S;
        const PaxosHist h = hs();
        u64 lo = hist_lo(o), hi = hist_hi(o);
        const u32 ph = h.phase(lo, hi, c);
        if (kind == PUTOK) h.record_get(lo, hi, c);
        else PaxosHist::put(lo, hi, h.ret_off(c), 3, m & 7);
        PaxosHist::put(lo, hi, 2 * c, 2, ph + 1);
        hist_set(o, lo, hi);
    }
    SR_HD void record_out(u64*, u32, u32, u32) const {}  // the Puts at start: phase 0; Gets: in record_in
    SR_HD bool within_boundary(const u64*) const { return true; }
    SR_HD bool discovers(int p, const u64* s, const u32* net) const {
        if (p == 0) return !hs().linearizable(hist_lo(s), hist_hi(s));  // always "linearizable"
        bool any = false;                                                // sometimes "value chosen"
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const u32 e = net[k];
            any |= e != EMPTY && (e_msg(e) >> 13) == GETOK && (e & 7) != 0;
        }
        return any;
    }
    int expectation(int p) const { return p == 0 ? ALWAYS : SOMETIMES; }
    const char* prop_name(int p) const { return p == 0 ? "linearizable" : "value chosen"; }
    // the oracle's msg code: ((((req * 8 + clock) * 8 + id) * 8 + val) * 8 + kind)
    i64 msg_code(u32 m) const {
        const i64 kind = m >> 13, req = m >> 9 & 15, clock = m >> 6 & 7, id = m >> 3 & 7, val = m & 7;
        return (((req * 8 + clock) * 8 + id) * 8 + val) * 8 + kind;
    }
    u32 msg_decode(i64 code) const {
        return msg((u32)(code % 8), (u32)(code / 4096), (u32)(code / 512 % 8), (u32)(code / 64 % 8), (u32)(code / 8 % 8));
    }
    std::string format_msg(i64 code) const { return AbdSys{}.format_msg(code); }
    int actors_width() const { return (int)((S + C) * (8 + S)); }
    int history_width() const { return hs().width(); }
    // oracle/actor.hpp AbdSys::describe_actor, per actor (8 + S values), then the history
    int describe_fields(const u64* s, i64* d) const {
        int k = 0;
        const int width = 8 + (int)S;
        for (u32 id = 0; id < S + C; ++id) {
            const int base = k;
            if (id < S) {
                const u64 w = s[SRV + id];
                const u32 phase = getf(w, 9, 2), wr = getf(w, 18, 3);
                d[k++] = getf(w, 0, 3);
                d[k++] = getf(w, 3, 3);
                d[k++] = getf(w, 6, 3);
                d[k++] = phase;
                d[k++] = phase ? getf(w, 11, 4) : 0;
                d[k++] = phase ? getf(w, 15, 3) : 0;
                d[k++] = phase && wr ? (i64)wr - 1 : -1;
                for (u32 j = 0; j < S; ++j) {
                    const u32 r = getf(w, RSP + RW * (int)j, RW);
                    d[k++] = phase != 1 || !(r & 1) ? -1 : (i64)(r >> 1 & 7) * 64 + (i64)(r >> 4 & 7) * 8 + (r >> 7 & 7);
                }
                d[k++] = phase == 2 ? getf(w, RSP, MAXS) : 0;
            } else {
                const u32 ph = hs().phase(hist_lo(s), hist_hi(s), id - S);
                d[k++] = ph == 0 ? (i64)id : ph == 1 ? (i64)(2 * id) : -1;
                d[k++] = (i64)ph + 1;
            }
            while (k < base + width) d[k++] = 0;
        }
        hs().describe(hist_lo(s), hist_hi(s), d + k);
        return k + history_width();
    }
    int undescribe_fields(const i64* d, u64* s) const {
        int k = 0;
        const int width = 8 + (int)S;
        u32 phases[px::MAX_CLIENTS] = {};
        for (u32 id = 0; id < S + C; ++id, k += width) {
            if (id >= S) {
                phases[id - S] = (u32)(d[k + 1] - 1);
                continue;
            }
            const u32 phase = (u32)d[k + 3];
            u64 w = (u64)(d[k] & 7) | (u64)(d[k + 1] & 7) << 3 | (u64)(d[k + 2] & 7) << 6 | (u64)(phase & 3) << 9;
            if (phase) {
                w |= (u64)(d[k + 4] & 15) << 11 | (u64)(d[k + 5] & 7) << 15;
                if (d[k + 6] >= 0) w |= (u64)((d[k + 6] + 1) & 7) << 18;
            }
            if (phase == 1)
                for (u32 j = 0; j < S; ++j) {
                    const i64 r = d[k + 7 + (int)j];
                    if (r >= 0) w |= (u64)rsp((u32)(r / 64) & 7, (u32)(r / 8 % 8), (u32)(r % 8)) << (RSP + RW * (int)j);
                }
            if (phase == 2) w |= (u64)(d[k + 7 + (int)S] & 15) << RSP;
            s[SRV + id] = w;
        }
        u64 lo = 0, hi = 0;
        hs().undescribe(d + k, phases, lo, hi);
        hist_set(s, lo, hi);
        return k + history_width();
    }
};

}  // namespace act

using AbdRegisterWide16 = act::ActorGpu<act::AbdWideSysT<16>>;  // 14-word states
using AbdRegisterWide32 = act::ActorGpu<act::AbdWideSysT<32>>;  // 22-word states

// ABD (C, S) built with the encoding `abd_slots` picks, handed to f (device: the GPU whose history
// tables the 8-slot encoding reads, -1 for host use only).
template <class F>
auto with_abd_model(int C, int S, int device, F&& f) {
    const int slots = act::abd_slots(C, S);
    if (slots == 8) {
        AbdRegister m;
        static_cast<act::AbdSys&>(m) = act::AbdSys::make(C, S, device);
        return f(m);
    }
    if (slots == 16) {
        AbdRegisterWide16 m;
        static_cast<act::AbdWideSysT<16>&>(m) = act::AbdWideSysT<16>::make(C, S);
        return f(m);
    }
    AbdRegisterWide32 m;
    static_cast<act::AbdWideSysT<32>&>(m) = act::AbdWideSysT<32>::make(C, S);
    return f(m);
}

}  // namespace sr
