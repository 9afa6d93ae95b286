// MI355X breadth-first model-checking engine library: the compiled-in GpuModel registry and the
// C ABI (include/stateright_gpu.h). The engine itself is engine.hpp.
#include <unordered_set>
#include "registry.hpp"
#include "dgraph.hpp"
#include "paxos.hpp"
#include "abd_wide.hpp"
#include "dist_host.hpp"
#include "table_selftest.hpp"
#include "rehash_selftest.hpp"
#include "certify_selftest.hpp"

namespace sr {

static thread_local std::string g_last_error;
static void set_error(const std::string& e) { g_last_error = e; }

}  // namespace sr

namespace sr {

// The registry (registry.hpp): each family of models compiles in its own translation unit.
static std::unique_ptr<EngineBase> make_model_engine(const EngineArgs& a) {
    if (a.o->symmetry && a.model != SR_MODEL_2PC && a.model != SR_MODEL_2PC_STEP)
        throw Error(SR_ERR_UNSUPPORTED, "symmetry reduction: model " + std::to_string(a.model) + " has no canonical form");
    switch (a.model) {
        case SR_MODEL_LINEAR_EQUATION:
        case SR_MODEL_BINARY_CLOCK:
        case SR_MODEL_DGRAPH:
        case SR_MODEL_ACTOR_FIXTURE:
        case SR_MODEL_LADDER:
            return reg_basic(a);
        case SR_MODEL_2PC: return reg_two_phase(a);
        case SR_MODEL_INCREMENT: return reg_increment(a);
        case SR_MODEL_INCREMENT_LOCK: return reg_increment_lock(a);
        case SR_MODEL_PAXOS:
            a.need(1);
            if (a.p[0] < 1 || a.p[0] > px::MAX_CLIENTS) throw Error(SR_ERR_UNSUPPORTED, "paxos: client_count must be in 1..=6");
            return a.p[0] <= Paxos::max_clients() ? reg_paxos(a) : reg_paxos_wide(a);
        case SR_MODEL_PINGPONG: return reg_ping_pong(a);
        case SR_MODEL_ABD:
        case SR_MODEL_SINGLE_COPY:
            return reg_registers(a);
        case SR_MODEL_SPREAD:
        case SR_MODEL_LIVE_GRAPH:
            return reg_spread(a);
        case SR_MODEL_2PC_LIVE: return reg_two_phase_live(a);
        case SR_MODEL_SPIN_LOCK: return reg_spin_lock(a);
        case SR_MODEL_FAIR_RINGS: return reg_fair_rings(a);
        case SR_MODEL_LEADS_GRAPH:
        case SR_MODEL_LEADS_DGRAPH:
            return reg_leads(a);
        case SR_MODEL_REQ_LOCK:
            req_lock_threads(a.p, a.np);
            return a.p[0] <= 4 ? reg_req_lock(a) : reg_req_lock_wide(a);
        case SR_MODEL_STEP_GRAPH:
        case SR_MODEL_2PC_STEP:
        case SR_MODEL_STEP_DGRAPH:
            return reg_step(a);
    }
    throw Error(SR_ERR_ARG, "unknown model id " + std::to_string(a.model));
}

// The complete `eventually` check (sr_opts.liveness, live.hpp) runs on one GPU over a registered model.
static void refuse_liveness(const sr_opts& o, bool partitioned, bool plugin) {
    if (!o.liveness) return;
    if (partitioned) throw Error(SR_ERR_UNSUPPORTED, "liveness with a partitioned search: the fixpoint runs on one GPU's visited set and arena");
    if (plugin) throw Error(SR_ERR_UNSUPPORTED, "liveness with a plugin model: registered models only");
    if (o.symmetry) throw Error(SR_ERR_UNSUPPORTED, "liveness with symmetry: the fixpoint runs on concrete states, not on orbit representatives");
}

// The coverage pass (sr_opts.coverage, cover.hpp) runs on one GPU's arena, over states (Engine<M> refuses
// target_state_count and, for a plugin's canonical form too, symmetry).
static void refuse_coverage(const sr_opts& o, bool partitioned) {
    if (!o.coverage) return;
    if (partitioned) throw Error(SR_ERR_UNSUPPORTED, "coverage with a partitioned search: the pass counts over one GPU's arena");
    if (o.symmetry) throw Error(SR_ERR_UNSUPPORTED, "coverage with symmetry: the counts would be over orbit representatives, not over states");
    if (o.target_state_count)
        throw Error(SR_ERR_UNSUPPORTED, "coverage with target_state_count: the counts are over the whole reachable set");
}

static std::unique_ptr<EngineBase> make_engine(int model, const i64* p, int np, const sr_opts& o) {
    refuse_liveness(o, false, false);
    refuse_coverage(o, false);
    return make_model_engine(EngineArgs{model, p, np, &o, false, nullptr, 0});
}

}  // namespace sr

using namespace sr;

struct sr_bfs {
    std::unique_ptr<EngineBase> e;
    bool joined = false;
};

namespace sr {
// Driver threads of the checks, pooled: a check runs on an idle pooled thread, which after its
// job spins for up to ~2 ms for the next one before it sleeps, so back-to-back checks pay neither
// thread creation nor a wake-up (~20-50 us per check on a 2 ms check). Threads are never joined:
// the pool lives for the process.
class DriverPool {
    struct Worker {
        std::mutex mu;
        std::condition_variable cv;
        std::function<void()> job;
        std::atomic<bool> has_job{false};
        std::atomic<bool> idle{false};
    };

  public:
    static DriverPool& get() {
        static DriverPool* p = new DriverPool();  // never destroyed (its threads outlive main)
        return *p;
    }
    void submit(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (Worker* w : workers_) {
                bool t = true;
                if (w->idle.compare_exchange_strong(t, false)) {
                    hand(w, std::move(f));
                    return;
                }
            }
        }
        Worker* w = new Worker();
        hand(w, std::move(f));
        std::thread([w] { loop(w); }).detach();
        std::lock_guard<std::mutex> g(mu_);
        workers_.push_back(w);
    }

  private:
    static void hand(Worker* w, std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(w->mu);
            w->job = std::move(f);
            w->has_job.store(true, std::memory_order_release);
        }
        w->cv.notify_one();
    }
    static void loop(Worker* w) {
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            for (u32 spin = 1; !w->has_job.load(std::memory_order_acquire); ++spin) {
                _mm_pause();
                if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
                    std::unique_lock<std::mutex> g(w->mu);
                    w->cv.wait(g, [w] { return w->has_job.load(std::memory_order_acquire); });
                    break;
                }
            }
            std::function<void()> job;
            {
                std::lock_guard<std::mutex> g(w->mu);
                job.swap(w->job);
                w->has_job.store(false, std::memory_order_relaxed);
            }
            job();
            job = nullptr;
            w->idle.store(true, std::memory_order_release);
        }
    }
    std::mutex mu_;
    std::vector<Worker*> workers_;
};
}  // namespace sr

namespace sr {
// Host BFS over the reachable states of m: every slot self_loops() reports must be enabled and
// must return the state itself (the FAST expansion counts those slots without generating them).
template <class M>
static bool check_self_loops(const M& m, std::string& why) {
    constexpr int W = M::W, MW = M::MW;
    struct H {
        size_t operator()(const std::vector<u64>& v) const {
            u64 h = 0;
            for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
            return (size_t)h;
        }
    };
    std::unordered_set<std::vector<u64>, H> seen;
    const std::vector<u64> inits = init_states_of(m);
    const int k = (int)(inits.size() / W);
    std::vector<std::vector<u64>> queue;
    for (int i = 0; i < k; ++i) {
        std::vector<u64> st(inits.begin() + i * W, inits.begin() + (i + 1) * W);
        if (seen.insert(st).second) queue.push_back(st);
    }
    for (size_t q = 0; q < queue.size(); ++q) {
        const std::vector<u64> st = queue[q];
        u64 mk[MW], sl[MW], o[W];
        m.enabled(st.data(), mk);
        m.self_loops(st.data(), mk, sl);
        for (int w = 0; w < MW; ++w) {
            if (sl[w] & ~mk[w]) {
                why = "self_loops reports a slot that is not enabled";
                return false;
            }
            for (u64 bits = sl[w]; bits; bits &= bits - 1) {
                const int a = w * 64 + __builtin_ctzll(bits);
                if (!m.apply(st.data(), a, o) || !std::equal(o, o + W, st.data())) {
                    why = "self_loops reports slot " + std::to_string(a) + ", whose next state differs";
                    return false;
                }
            }
            for (u64 bits = mk[w]; bits; bits &= bits - 1) {
                const int a = w * 64 + __builtin_ctzll(bits);
                if (!m.apply(st.data(), a, o)) continue;
                std::vector<u64> nx(o, o + W);
                if (seen.insert(nx).second) queue.push_back(std::move(nx));
            }
        }
    }
    return true;
}

// The FAST expansion's optional hooks of a one-word model against its `enabled`, `self_loops` and
// `apply` (models.hpp has_action_masks, has_enabled_moves, SELF_LOOPS_EXACT), at one state:
// `action_masks` gives apply's state for every enabled slot, `enabled_moves` is
// enabled & ~self_loops with the self-loops' count, and every slot it leaves changes the state.
template <class M>
static bool check_action_masks_at(const M& m, u64 s, std::string& why) {
    static_assert(M::W == 1, "one-word models");
    constexpr int MW = M::MW;
    auto fail = [&](const std::string& what) {
        why = what + " at state " + std::to_string(s);
        return false;
    };
    u64 mk[MW], mv[MW], o[1];
    m.enabled(&s, mk);
    u32 loops = 0;
    for (int w = 0; w < MW; ++w) mv[w] = mk[w];
    if constexpr (has_self_loops<M>::value) {
        u64 sl[MW];
        m.self_loops(&s, mk, sl);
        for (int w = 0; w < MW; ++w) {
            loops += (u32)__builtin_popcountll(sl[w]);
            mv[w] &= ~sl[w];
        }
    }
    if constexpr (has_enabled_moves<M>::value) {
        u64 em[MW];
        const u32 r = m.enabled_moves(&s, em);
        for (int w = 0; w < MW; ++w)
            if (em[w] != mv[w]) return fail("enabled_moves differs from enabled & ~self_loops in word " + std::to_string(w));
        if (r != loops) return fail("enabled_moves returns " + std::to_string(r) + " self-loops, self_loops has " + std::to_string(loops));
    }
    for (int w = 0; w < MW; ++w)
        for (u64 bits = mk[w]; bits; bits &= bits - 1) {
            const int a = w * 64 + __builtin_ctzll(bits);
            if (!m.apply(&s, a, o)) return fail("apply refuses enabled slot " + std::to_string(a));
            if constexpr (has_action_masks<M>::value) {
                u64 clr, set;
                m.action_masks(a, &clr, &set);
                if (((s & ~clr) | set) != o[0]) return fail("action_masks of slot " + std::to_string(a) + " differs from apply");
            }
            if constexpr (self_loops_exact<M>::value) {
                if ((mv[w] >> (a & 63) & 1) && o[0] == s) return fail("slot " + std::to_string(a) + " is left enabled and returns the state itself");
            }
        }
    return true;
}
// Over every reachable state (walk) and `random` states of `bits` bits.
template <class M>
static bool check_action_masks(const M& m, int bits, bool walk, int random, std::string& why) {
    if (walk) {
        std::unordered_set<u64> seen;
        std::vector<u64> queue = init_states_of(m);
        for (u64 s : queue) seen.insert(s);
        for (size_t q = 0; q < queue.size(); ++q) {
            const u64 s = queue[q];
            if (!check_action_masks_at(m, s, why)) return false;
            for_each_successor(m, &s, [&](int, const u64* ns) {
                if (seen.insert(ns[0]).second) queue.push_back(ns[0]);
            });
        }
    }
    u64 x = 0x9E3779B97F4A7C15ull + (u64)bits;
    for (int i = 0; i < random; ++i) {
        x = fmix64(x + 0x632BE59BD9B4E019ull);
        if (!check_action_masks_at(m, x & ((1ull << bits) - 1), why)) return false;
    }
    return true;
}

}  // namespace sr

extern "C" {

void sr_opts_init(sr_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->struct_size = sizeof(sr_opts);
}

void sr_opts_init_sized(sr_opts* o, uint32_t size) {
    // a caller built against an older (shorter) sr_opts: only its own bytes are written, and the
    // engine reads only struct_size bytes back (normalized_opts), defaulting the rest
    const uint32_t n = size < (uint32_t)sizeof(sr_opts) ? size : (uint32_t)sizeof(sr_opts);
    if (!o || n < sizeof(uint32_t)) return;
    std::memset(o, 0, n);
    o->struct_size = n;
}

const char* sr_last_error(void) { return g_last_error.c_str(); }

int sr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

struct sr_dist {
    std::unique_ptr<Comm> c;
    hipStream_t stream = nullptr;  // for sr_dist_barrier / sr_dist_allreduce_f64
    hipStream_t get_stream() {
        if (!stream) {
            SR_HIP(hipSetDevice(c->device));
            SR_HIP(create_stream(&stream, c->device));
        }
        return stream;
    }
};

// Starts the driver thread of an engine (spawn returns at once, like the reference's spawn_bfs).
static sr_bfs* start(std::unique_ptr<EngineBase> engine) {
    auto b = std::make_unique<sr_bfs>();
    b->e = std::move(engine);
    EngineBase* e = b->e.get();
    DriverPool::get().submit([e] {
        try {
            e->run();
        } catch (const Error& x) {
            e->status = x.code;
            e->error = x.what();
        } catch (const std::exception& x) {
            e->status = SR_ERR_HIP;
            e->error = x.what();
        }
        e->finished.store(true, std::memory_order_release);  // the last access to the engine
    });
    return b.release();
}

sr_bfs* sr_gpu_bfs_spawn(int32_t model_id, const int64_t* params, int32_t nparams, const sr_opts* opts) {
    try {
        const sr_opts o = normalized_opts(opts);
        if (sr_device_count() <= 0) throw Error(SR_ERR_NO_DEVICE, "no HIP device visible");
        return start(make_engine(model_id, params, nparams, o));
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

static sr_bfs* spawn_plugin(const sr_plugin* pl, sr_dist* comm, int32_t vparts, const int64_t* params, int32_t nparams,
                            const sr_opts* opts) {
    try {
        if (!pl || !pl->create) throw Error(SR_ERR_ARG, "null plugin");
        if (pl->abi != SR_PLUGIN_ABI || pl->opts_size != sizeof(sr_opts))
            throw Error(SR_ERR_ARG, std::string("plugin ") + (pl->name ? pl->name : "?") + " was built against other headers (abi " +
                                        std::to_string(pl->abi) + ", engine " + std::to_string(SR_PLUGIN_ABI) + ")");
        sr_opts o = normalized_opts(opts);
        refuse_liveness(o, comm != nullptr || vparts > 1, true);
        refuse_coverage(o, comm != nullptr || vparts > 1);
        if (comm) o.device = comm->c->device;
        if (sr_device_count() <= 0) throw Error(SR_ERR_NO_DEVICE, "no HIP device visible");
        char err[512] = {0};
        void* e = pl->create(params, nparams, &o, comm ? comm->c.get() : nullptr, vparts, err, sizeof(err));
        if (!e) throw Error(SR_ERR_ARG, std::string("plugin ") + (pl->name ? pl->name : "?") + ": " + err);
        return start(std::unique_ptr<EngineBase>(static_cast<EngineBase*>(e)));
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

sr_bfs* sr_gpu_bfs_spawn_plugin(const sr_plugin* pl, const int64_t* params, int32_t nparams, const sr_opts* opts) {
    return spawn_plugin(pl, nullptr, 0, params, nparams, opts);
}

sr_bfs* sr_gpu_bfs_spawn_plugin_partitioned(const sr_plugin* pl, sr_dist* comm, int32_t vparts, const int64_t* params,
                                            int32_t nparams, const sr_opts* opts) {
    if (!comm && vparts < 1) {
        set_error("partitioned plugin spawn: a communicator or virtual_partitions >= 1");
        return nullptr;
    }
    return spawn_plugin(pl, comm, comm ? 0 : std::max(vparts, 2), params, nparams, opts);
}

}  // extern "C"

namespace sr {
// A registered model built for host use only (no device tables), handed to f: the models whose
// description determines the state (`undescribe`), for sr_model_fingerprint and the self-test.
template <class F>
static i64 with_host_model(int model, const i64* p, int np, F&& f) {
    auto need = [&](int k) {
        if (np < k) throw Error(SR_ERR_ARG, "model " + std::to_string(model) + " needs " + std::to_string(k) + " params");
    };
    switch (model) {
        case SR_MODEL_LINEAR_EQUATION:
            need(3);
            return f(LinearEquation{(u32)(p[0] & 0xff), (u32)(p[1] & 0xff), (u32)(p[2] & 0xff)});
        case SR_MODEL_BINARY_CLOCK: return f(BinaryClock{});
        case SR_MODEL_DGRAPH: return f(DGraph::make(p, np, -1));  // (host tables only)
        case SR_MODEL_2PC:
            need(1);
            if (p[0] < 1 || p[0] > 14) throw Error(SR_ERR_UNSUPPORTED, "2pc: rm_count must be in 1..=14");
            return f(TwoPhase{(int)p[0]});
        case SR_MODEL_INCREMENT:
            need(1);
            if (p[0] < 1 || p[0] > 15) throw Error(SR_ERR_UNSUPPORTED, "increment: threads must be in 1..=15");
            return p[0] <= 9 ? f(Increment<1>{(int)p[0]}) : f(Increment<2>{(int)p[0]});
        case SR_MODEL_INCREMENT_LOCK:
            need(1);
            if (p[0] < 1 || p[0] > 12) throw Error(SR_ERR_UNSUPPORTED, "increment_lock: threads must be in 1..=12");
            return p[0] <= 8 ? f(IncrementLock<1>{(int)p[0]}) : f(IncrementLock<2>{(int)p[0]});
        case SR_MODEL_PAXOS:
            need(1);
            if (p[0] < 1 || p[0] > px::MAX_CLIENTS) throw Error(SR_ERR_UNSUPPORTED, "paxos: client_count must be in 1..=6");
            return p[0] <= Paxos::max_clients() ? f(Paxos::make((int)p[0])) : f(PaxosWide::make((int)p[0]));
        case SR_MODEL_PINGPONG: {
            need(1);
            if (p[0] < 0 || p[0] > (i64)PingPongWide::MAX_NAT) throw Error(SR_ERR_UNSUPPORTED, "ping-pong: max_nat must be in 0..=14");
            auto fill = [&](auto& m) {
                m.max_nat = (u32)p[0];
                m.lossy = np > 1 && p[1] != 0;
                m.duplicating = np > 2 ? p[2] != 0 : true;
                m.maintains_history = np > 3 && p[3] != 0;
            };
            if (p[0] <= (i64)PingPong::MAX_NAT) {
                PingPong m;
                fill(m);
                return f(m);
            }
            PingPongWide m;
            fill(m);
            return f(m);
        }
        case SR_MODEL_ACTOR_FIXTURE: {
            need(1);
            ActorFixture m;
            m.kind = (int)p[0];
            return f(m);
        }
        case SR_MODEL_ABD: {
            need(1);
            return with_abd_model((int)p[0], np > 1 ? (int)p[1] : 2, -1, [&](const auto& m) -> i64 { return f(m); });
        }
        case SR_MODEL_SINGLE_COPY: {
            need(1);
            SingleCopyRegister m;
            static_cast<act::SingleCopySys&>(m) = act::SingleCopySys::make((int)p[0], np > 1 ? (int)p[1] : 1);
            return f(m);
        }
        case SR_MODEL_LADDER:
            need(2);
            if (p[0] < 1 || p[0] > 62 || p[1] < 0 || p[1] > 57) throw Error(SR_ERR_UNSUPPORTED, "ladder: rungs 1..=62, free bits 0..=57");
            return f(Ladder{(int)p[0], (int)p[1]});
        case SR_MODEL_SPREAD:
            return with_spread_model(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_LIVE_GRAPH:
            return with_live_graph(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_2PC_LIVE:
            return with_two_phase_live(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_SPIN_LOCK:
            return with_spin_lock(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_FAIR_RINGS:
            return with_fair_rings(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_LEADS_GRAPH:
            return with_leads_graph(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_LEADS_DGRAPH: return f(LeadsDGraph::make(p, np, -1));  // (host tables only)
        case SR_MODEL_REQ_LOCK:
            return with_req_lock(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_STEP_GRAPH:
            return with_step_graph(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_2PC_STEP:
            return with_two_phase_step(p, np, [&](const auto& m) -> i64 { return f(m); });
        case SR_MODEL_STEP_DGRAPH: return f(StepDGraph::make(p, np, -1));  // (host tables only)
        default:
            return SR_ERR_UNSUPPORTED;
    }
}

// Host BFS over up to max_states reachable states of m: every state's description must give the
// state back (undescribe) and so the engine's fingerprint of it. Returns the states checked.
template <class M>
static i64 describe_roundtrip(const M& m, i64 max_states, std::string& why) {
    if constexpr (!has_undescribe<M>::value) {
        why = "model has no state description inverse";
        return SR_ERR_UNSUPPORTED;
    } else {
        constexpr int W = M::W, MW = M::MW;
        struct H {
            size_t operator()(const std::vector<u64>& v) const {
                u64 h = 0;
                for (u64 x : v) h = fmix64(h ^ x) + 0x9E3779B97F4A7C15ull;
                return (size_t)h;
            }
        };
        std::unordered_set<std::vector<u64>, H> seen;
        std::vector<std::vector<u64>> queue;
        const std::vector<u64> inits = init_states_of(m);
        for (size_t i = 0; i + W <= inits.size(); i += W) {
            std::vector<u64> st(inits.begin() + (i64)i, inits.begin() + (i64)(i + W));
            if (seen.insert(st).second) queue.push_back(st);
        }
        std::vector<i64> d((size_t)m.describe_width());
        for (size_t q = 0; q < queue.size() && (i64)q < max_states; ++q) {
            const std::vector<u64> st = queue[q];
            m.describe(st.data(), d.data());
            u64 back[W];
            m.undescribe(d.data(), back);
            if (!std::equal(back, back + W, st.data())) {
                why = "state " + std::to_string(q) + " does not survive describe -> undescribe";
                return SR_ERR_ARG;
            }
            u64 fp = 0;
            if (described_fingerprint(m, d.data(), (int)d.size(), &fp) != SR_OK || fp != state_fp<M>(st.data())) {
                why = "state " + std::to_string(q) + ": sr_model_fingerprint differs from the engine's fingerprint";
                return SR_ERR_ARG;
            }
            u64 mk[MW], o[W];
            m.enabled(st.data(), mk);
            for (int w = 0; w < MW; ++w)
                for (u64 bits = mk[w]; bits; bits &= bits - 1) {
                    const int a = w * 64 + __builtin_ctzll(bits);
                    if (!m.apply(st.data(), a, o)) continue;
                    std::vector<u64> nx(o, o + W);
                    if (seen.insert(nx).second) queue.push_back(std::move(nx));
                }
        }
        return (i64)std::min<size_t>(queue.size(), (size_t)max_states);
    }
}

// Behind the three sr_liveness_host* entry points (`name`). args: nullptr, or what is wrong with the arguments;
// fairness: nullptr, or the mode ("weak fairness") that needs a FAIR_SLOTS model; form(m, moves) runs the host
// form (live.hpp) on a model with an `eventually` property and returns its LiveHost.
template <class Form>
static int64_t liveness_host_entry(const char* name, const char* args, const char* fairness, int32_t model, const int64_t* p, int32_t np,
                                   sr_live_result* out, int64_t* action_ids, int32_t cap, Form&& form) {
    try {
        if (args) throw Error(SR_ERR_ARG, args);
        // SR_LIVE_MOVES=0: the progress mode and the fair ones compare states even where the model's
        // `enabled_moves` names its self-loops (tests run both and compare; read per call)
        const char* e = std::getenv("SR_LIVE_MOVES");
        const bool moves = !e || std::atoi(e) != 0;
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            using M = std::decay_t<decltype(m)>;
            if constexpr (has_emask<M>::value) {
                const LiveHost h = form(m, moves);
                *out = h.r;
                for (int32_t i = 0; action_ids && i < cap && i < (int32_t)h.actions.size(); ++i) action_ids[i] = h.actions[i];
                return (i64)h.unique;
            } else {
                if (fairness && !fair_slots_model<M>)
                    throw Error(SR_ERR_UNSUPPORTED, std::string(fairness) + ": this model's slots are not fairness classes");
                throw Error(SR_ERR_ARG, "liveness: the model has no `eventually` property");
            }
        });
        if (r == SR_ERR_UNSUPPORTED) set_error(std::string(name) + ": model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

// A fair host form's LiveHostFair: the mode's counters go to *stats, the rest to liveness_host_entry.
template <class Stats>
static LiveHost live_host_split(LiveHostFair<Stats> f, Stats* stats) {
    *stats = f.s;
    return std::move(f.h);
}

// Behind sr_gpu_bfs_loop_fair and sr_gpu_bfs_loop_strongly_fair.
static int32_t loop_fair_entry(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t loop_start, bool strong) {
    if (!b || !b->e->finished.load(std::memory_order_acquire) || n < 0 || (n > 0 && !ids) || loop_start < 0 || loop_start > n) return -1;
    try {
        return b->e->loop_fair(init, ids, n, loop_start, strong);
    } catch (const std::exception& x) {  // (the host model's replay: nothing crosses the C ABI)
        set_error(x.what());
        return -1;
    }
}

}  // namespace sr

extern "C" {

int32_t sr_model_fingerprint(int32_t model, const int64_t* p, int32_t np, const int64_t* d, int32_t width, uint64_t* fp) {
    try {
        std::string why;
        const int r = (int)with_host_model(model, p, np, [&](const auto& m) { return (i64)described_fingerprint(m, d, width, fp, &why); });
        if (r != SR_OK) set_error(why);
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int64_t sr_selftest_describe(int32_t model, const int64_t* p, int32_t np, int64_t max_states) {
    try {
        std::string why;
        const i64 r = with_host_model(model, p, np, [&](const auto& m) { return (i64)describe_roundtrip(m, max_states, why); });
        if (r < 0) set_error(why);
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

void sr_sim_opts_init_sized(sr_sim_opts* o, uint32_t size) {
    const uint32_t n = size < (uint32_t)sizeof(sr_sim_opts) ? size : (uint32_t)sizeof(sr_sim_opts);
    if (!o || n < sizeof(uint32_t)) return;
    sr_sim_opts d;
    std::memset(&d, 0, sizeof(d));
    d.struct_size = n;
    d.max_depth = 4096;
    std::memcpy(o, &d, n);  // only the caller's own bytes
}

sr_bfs* sr_gpu_sim_spawn(int32_t model_id, const int64_t* params, int32_t nparams, const sr_sim_opts* opts) {
    try {
        const sr_sim_opts so = normalized_sim_opts(opts);
        if (sr_device_count() <= 0) throw Error(SR_ERR_NO_DEVICE, "no HIP device visible");
        sr_opts o = normalized_opts(nullptr);
        o.device = so.device;
        EngineArgs a{model_id, params, nparams, &o, false, nullptr, 0};
        a.sim = &so;
        return start(make_model_engine(a));
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

int64_t sr_gpu_sim_walk_records(const sr_bfs* b, uint32_t* steps, uint32_t* end_reason, uint64_t* final_fp, int64_t cap) {
    const SimEngineBase* e = b ? dynamic_cast<const SimEngineBase*>(b->e.get()) : nullptr;
    if (!e) {
        set_error("not a simulation handle");
        return SR_ERR_ARG;
    }
    return e->sim_records(steps, end_reason, final_fp, std::max<int64_t>(cap, 0));
}

int64_t sr_gpu_sim_walk_loop_starts(const sr_bfs* b, uint32_t* loop_start, int64_t cap) {
    const SimEngineBase* e = b ? dynamic_cast<const SimEngineBase*>(b->e.get()) : nullptr;
    if (!e) {
        set_error("not a simulation handle");
        return SR_ERR_ARG;
    }
    return e->sim_loop_starts(loop_start, std::max<int64_t>(cap, 0));
}

int32_t sr_gpu_sim_hit(const sr_bfs* b, int32_t prop, uint64_t* walk, uint32_t* step) {
    const SimEngineBase* e = b ? dynamic_cast<const SimEngineBase*>(b->e.get()) : nullptr;
    return e && e->sim_hit(prop, walk, step) ? 1 : 0;
}

int32_t sr_gpu_sim_unique(const sr_bfs* b, sr_sim_unique_result* out) {
    const SimEngineBase* e = b ? dynamic_cast<const SimEngineBase*>(b->e.get()) : nullptr;
    if (!e || !out || out->struct_size < sizeof(uint32_t) || !b->e->finished.load(std::memory_order_acquire)) {
        set_error("sr_gpu_sim_unique: a finished simulation handle and a sized result");
        return SR_ERR_ARG;
    }
    sr_sim_unique_result r = e->sim_unique();
    if (!r.on) r.batches = e->stats.levels;
    r.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(r));
    std::memcpy(out, &r, r.struct_size);  // only the caller's own bytes
    return SR_OK;
}

int64_t sr_gpu_sim_unique_fingerprints(sr_bfs* b, uint64_t* out, int64_t cap) {
    SimEngineBase* e = b ? dynamic_cast<SimEngineBase*>(b->e.get()) : nullptr;
    if (!e || !b->e->finished.load(std::memory_order_acquire)) {
        set_error("sr_gpu_sim_unique_fingerprints: not a finished simulation handle");
        return SR_ERR_ARG;
    }
    const int64_t n = e->sim_unique_fps(out, std::max<int64_t>(cap, 0));
    if (n < 0) {
        set_error("sr_gpu_sim_unique_fingerprints: the simulation ran without sr_sim_opts.unique");
        return SR_ERR_ARG;
    }
    return n;
}

int64_t sr_gpu_sim_batch_new(const sr_bfs* b, uint64_t* out, int64_t cap) {
    const SimEngineBase* e = b ? dynamic_cast<const SimEngineBase*>(b->e.get()) : nullptr;
    if (!e || !b->e->finished.load(std::memory_order_acquire)) {
        set_error("sr_gpu_sim_batch_new: not a finished simulation handle");
        return SR_ERR_ARG;
    }
    return e->sim_batch_new(out, std::max<int64_t>(cap, 0));
}

int64_t sr_sim_unique_host(int32_t model, const int64_t* p, int32_t np, uint64_t seed, uint64_t walk0, uint64_t nwalks,
                           uint32_t max_depth, int32_t loops, uint64_t* out, int64_t cap) {
    try {
        if (!max_depth || max_depth > SIM_MAX_DEPTH) throw Error(SR_ERR_ARG, "simulation: max_depth must be in 1..=2^20");
        if (walk0 >= SIM_MAX_WALKS || nwalks > SIM_MAX_WALKS - walk0) throw Error(SR_ERR_ARG, "simulation: walks must be below 2^40");
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            const std::vector<u64> fps = sim_unique_host(m, seed, walk0, nwalks, max_depth, loops != 0);
            for (int64_t i = 0; out && i < cap && i < (int64_t)fps.size(); ++i) out[i] = fps[(size_t)i];
            return (i64)fps.size();
        });
        if (r == SR_ERR_UNSUPPORTED) set_error("sr_sim_unique_host: model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int64_t sr_sim_walk(int32_t model, const int64_t* p, int32_t np, uint64_t seed, uint64_t walk, uint32_t max_depth,
                    int64_t* action_ids, int32_t cap, int32_t* end_reason, uint64_t* final_fp, int32_t* first_hit_step,
                    int32_t nprops, int32_t* attempts) {
    return sr_sim_walk_loops(model, p, np, seed, walk, max_depth, 0, action_ids, cap, end_reason, final_fp, first_hit_step, nprops,
                             attempts, nullptr);
}

int64_t sr_sim_walk_loops(int32_t model, const int64_t* p, int32_t np, uint64_t seed, uint64_t walk, uint32_t max_depth,
                          int32_t loops, int64_t* action_ids, int32_t cap, int32_t* end_reason, uint64_t* final_fp,
                          int32_t* first_hit_step, int32_t nprops, int32_t* attempts, int32_t* loop_start) {
    try {
        if (!max_depth || max_depth > SIM_MAX_DEPTH) throw Error(SR_ERR_ARG, "simulation: max_depth must be in 1..=2^20");
        if (walk >= SIM_MAX_WALKS) throw Error(SR_ERR_ARG, "simulation: walk must be below 2^40");
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            using M = std::decay_t<decltype(m)>;
            const SimHostWalk h = sim_host_walk(m, seed, walk, max_depth, loops != 0);
            for (int32_t i = 0; action_ids && i < cap && i < (int32_t)h.actions.size(); ++i) action_ids[i] = h.actions[i];
            if (end_reason) *end_reason = (int32_t)h.end;
            if (final_fp) *final_fp = h.final_fp;
            for (int32_t q = 0; first_hit_step && q < nprops; ++q) first_hit_step[q] = q < M::NPROPS ? h.first_hit[q] : -1;
            if (attempts) *attempts = (int32_t)h.redraws;
            if (loop_start) *loop_start = h.end == SIM_LOOP ? (int32_t)h.loop_start : -1;
            return (i64)h.steps;
        });
        if (r == SR_ERR_UNSUPPORTED) set_error("sr_sim_walk: model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int32_t sr_gpu_bfs_liveness(const sr_bfs* b, int32_t prop, sr_live_result* out) {
    if (!b || !out || !b->e->finished.load(std::memory_order_acquire) || !b->e->live_result(prop, out)) return SR_ERR_ARG;
    return SR_OK;
}

int64_t sr_liveness_host(int32_t model, const int64_t* p, int32_t np, int32_t prop, int64_t max_states, sr_live_result* out,
                         int64_t* action_ids, int32_t cap) {
    return sr_liveness_host_fair(model, p, np, prop, 0, max_states, out, action_ids, cap);
}

int32_t sr_gpu_bfs_sink_kind(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n) {
    if (!b || n < 0 || (n > 0 && !ids)) return -1;
    return b->e->sink_kind(init, ids, n);
}

int64_t sr_liveness_host_fair(int32_t model, const int64_t* p, int32_t np, int32_t prop, int32_t fairness, int64_t max_states,
                              sr_live_result* out, int64_t* action_ids, int32_t cap) {
    const char* args = !out || max_states < 1            ? "sr_liveness_host: out and max_states >= 1"
                       : fairness != 0 && fairness != 1 ? "sr_liveness_host_fair: fairness must be 0 (none) or 1 (progress)"
                                                        : nullptr;
    return liveness_host_entry("sr_liveness_host", args, nullptr, model, p, np, out, action_ids, cap, [&](const auto& m, bool moves) {
        return !fairness ? live_host(m, prop, (u64)max_states)
               : moves   ? live_host<true, true>(m, prop, (u64)max_states)
                         : live_host<true, false>(m, prop, (u64)max_states);
    });
}

int32_t sr_gpu_bfs_liveness_weak(const sr_bfs* b, int32_t prop, sr_live_weak* out) {
    if (!b || !out || !b->e->finished.load(std::memory_order_acquire) || !b->e->live_weak_result(prop, out)) return SR_ERR_ARG;
    return SR_OK;
}

int32_t sr_gpu_bfs_loop_fair(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t loop_start) {
    return loop_fair_entry(b, init, ids, n, loop_start, false);
}

int64_t sr_liveness_host_weak(int32_t model, const int64_t* p, int32_t np, int32_t prop, int64_t max_states, sr_live_result* out,
                              sr_live_weak* weak, int64_t* action_ids, int32_t cap) {
    const char* args = !out || !weak || max_states < 1 ? "sr_liveness_host_weak: out, weak and max_states >= 1" : nullptr;
    return liveness_host_entry("sr_liveness_host_weak", args, "weak fairness", model, p, np, out, action_ids, cap, [&](const auto& m, bool moves) {
        return live_host_split(moves ? live_host_weak<true>(m, prop, (u64)max_states) : live_host_weak<false>(m, prop, (u64)max_states), weak);
    });
}

int32_t sr_gpu_bfs_liveness_leads(const sr_bfs* b, int32_t prop, sr_live_leads* out) {
    if (!b || !out || !b->e->finished.load(std::memory_order_acquire) || !b->e->live_leads_result(prop, out)) return SR_ERR_ARG;
    return SR_OK;
}

int32_t sr_gpu_bfs_replay_triggers(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t prop, int32_t* out, int32_t cap) {
    if (!b || n < 0 || (n > 0 && !ids) || !out || cap < n + 1) return -1;
    try {
        std::vector<int> t;
        const int r = b->e->triggers(init, ids, n, prop, t);
        for (int i = 0; r > 0 && i < r; ++i) out[i] = t[i];
        return r;
    } catch (const std::exception& x) {  // (the host model's replay: nothing crosses the C ABI)
        set_error(x.what());
        return -1;
    }
}

int64_t sr_liveness_host_leads(int32_t model, const int64_t* p, int32_t np, int32_t prop, int32_t fairness, int64_t max_states,
                               sr_live_result* out, sr_live_leads* leads, int64_t* action_ids, int32_t cap) {
    const char* args = !out || !leads || max_states < 1 ? "sr_liveness_host_leads: out, leads and max_states >= 1"
                       : fairness < 0 || fairness > 3  ? "sr_liveness_host_leads: fairness must be 0 (none), 1 (progress), 2 (weak) or 3 (strong)"
                                                       : nullptr;
    if (leads) *leads = live_leads_none();
    const char* mode = fairness == 2 ? "weak fairness" : fairness == 3 ? "strong fairness" : nullptr;
    return liveness_host_entry("sr_liveness_host_leads", args, mode, model, p, np, out, action_ids, cap, [&](const auto& m, bool moves) -> LiveHost {
        using M = std::decay_t<decltype(m)>;
        if constexpr (!has_lmask<M>::value) {
            throw Error(SR_ERR_ARG, "liveness: the model has no leads-to property");
        } else {
            const LiveLeadsStart start{prop, *leads};
            const u64 cap_states = (u64)max_states;
            sr_live_weak wk;
            sr_live_strong sg;
            switch (fairness) {
                case 0: return live_host<false, true>(m, prop, cap_states, start);
                case 1: return moves ? live_host<true, true>(m, prop, cap_states, start) : live_host<true, false>(m, prop, cap_states, start);
                case 2: return live_host_split(moves ? live_host_weak<true>(m, prop, cap_states, start) : live_host_weak<false>(m, prop, cap_states, start), &wk);
                default: return live_host_split(moves ? live_host_strong<true>(m, prop, cap_states, start) : live_host_strong<false>(m, prop, cap_states, start), &sg);
            }
        }
    });
}

int32_t sr_gpu_bfs_liveness_strong(const sr_bfs* b, int32_t prop, sr_live_strong* out) {
    if (!b || !out || !b->e->finished.load(std::memory_order_acquire) || !b->e->live_strong_result(prop, out)) return SR_ERR_ARG;
    return SR_OK;
}

int32_t sr_gpu_bfs_loop_strongly_fair(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t loop_start) {
    return loop_fair_entry(b, init, ids, n, loop_start, true);
}

int64_t sr_liveness_host_strong(int32_t model, const int64_t* p, int32_t np, int32_t prop, int64_t max_states, sr_live_result* out,
                                sr_live_strong* strong, int64_t* action_ids, int32_t cap) {
    const char* args = !out || !strong || max_states < 1 ? "sr_liveness_host_strong: out, strong and max_states >= 1" : nullptr;
    return liveness_host_entry("sr_liveness_host_strong", args, "strong fairness", model, p, np, out, action_ids, cap, [&](const auto& m, bool moves) {
        return live_host_split(moves ? live_host_strong<true>(m, prop, (u64)max_states) : live_host_strong<false>(m, prop, (u64)max_states), strong);
    });
}

// Copies the fixed part of a pass' figures into the caller's mirror (at most its struct_size bytes).
static void cover_copy_out(const sr_coverage& c, sr_coverage* out) {
    sr_coverage r = c;
    r.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(r));
    std::memcpy(out, &r, r.struct_size);  // only the caller's own bytes
}

int32_t sr_gpu_bfs_coverage(const sr_bfs* b, sr_coverage* out) {
    if (!b || !out || out->struct_size < 2 * sizeof(uint32_t) || !b->e->finished.load(std::memory_order_acquire)) {
        set_error("sr_gpu_bfs_coverage: a finished check and a sized result struct");
        return SR_ERR_ARG;
    }
    cover_copy_out(b->e->cover.c, out);
    if (!b->e->cover.c.ran) set_error("coverage: the pass did not run (the option is off, or the search did not explore everything)");
    return SR_OK;
}

int32_t sr_gpu_bfs_coverage_classes(const sr_bfs* b, uint64_t* enabled, uint64_t* taken, uint64_t* moved, int32_t cap) {
    if (!b || !b->e->finished.load(std::memory_order_acquire)) return SR_ERR_ARG;
    const CoverFigures& f = b->e->cover;
    if (!f.c.ran) return 0;
    for (int32_t c = 0; c < cap && c < f.c.classes; ++c) {
        if (enabled) enabled[c] = f.enabled[(size_t)c];
        if (taken) taken[c] = f.taken[(size_t)c];
        if (moved) moved[c] = f.moved[(size_t)c];
    }
    return f.c.classes;
}

int32_t sr_gpu_bfs_coverage_props(const sr_bfs* b, uint64_t* holds, int32_t cap) {
    if (!b || !b->e->finished.load(std::memory_order_acquire)) return SR_ERR_ARG;
    const CoverFigures& f = b->e->cover;
    if (!f.c.ran) return 0;
    for (int32_t p = 0; holds && p < cap && p < f.c.nprops; ++p) holds[p] = f.holds[(size_t)p];
    return f.c.nprops;
}

int32_t sr_gpu_bfs_coverage_class_name(const sr_bfs* b, int32_t c, char* name, int32_t cap) {
    if (!b || !b->e->finished.load(std::memory_order_acquire) || c < 0 || c >= (int32_t)b->e->cover.names.size()) return SR_ERR_ARG;
    const std::string& s = b->e->cover.names[(size_t)c];
    if (name && cap > 0) std::snprintf(name, (size_t)cap, "%s", s.c_str());
    return (int32_t)s.size();
}

int64_t sr_coverage_host(int32_t model, const int64_t* p, int32_t np, int64_t max_states, sr_coverage* out, uint64_t* enabled,
                         uint64_t* taken, uint64_t* moved, int32_t class_cap, uint64_t* holds, int32_t prop_cap, char* names,
                         int32_t names_cap) {
    try {
        if (!out || out->struct_size < 2 * sizeof(uint32_t) || max_states < 1)
            throw Error(SR_ERR_ARG, "sr_coverage_host: a sized result struct and max_states >= 1");
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            const CoverFigures f = cover_host(m, (u64)max_states);
            cover_copy_out(f.c, out);
            for (int32_t c = 0; c < class_cap && c < f.c.classes; ++c) {
                if (enabled) enabled[c] = f.enabled[(size_t)c];
                if (taken) taken[c] = f.taken[(size_t)c];
                if (moved) moved[c] = f.moved[(size_t)c];
            }
            for (int32_t q = 0; holds && q < prop_cap && q < f.c.nprops; ++q) holds[q] = f.holds[(size_t)q];
            if (names && names_cap > 0) {
                std::string all;
                for (const std::string& s : f.names) all += s + "\n";
                std::snprintf(names, (size_t)names_cap, "%s", all.c_str());
            }
            return (i64)f.c.states;
        });
        if (r == SR_ERR_UNSUPPORTED) set_error("sr_coverage_host: model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

// Copies a step result into the caller's mirror (at most its struct_size bytes).
static void step_copy_out(const sr_step_result& s, sr_step_result* out) {
    sr_step_result r = s;
    r.struct_size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(r));
    std::memcpy(out, &r, r.struct_size);  // only the caller's own bytes
}

int32_t sr_gpu_bfs_step(const sr_bfs* b, int32_t prop, sr_step_result* out) {
    sr_step_result r;
    if (!b || !out || out->struct_size < 2 * sizeof(uint32_t) || !b->e->finished.load(std::memory_order_acquire) ||
        !b->e->step_result(prop, &r)) {
        set_error("sr_gpu_bfs_step: a finished check, one of its properties and a sized result struct");
        return SR_ERR_ARG;
    }
    step_copy_out(r, out);
    return SR_OK;
}

int32_t sr_gpu_bfs_replay_step(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t prop) {
    if (!b || n < 1 || !ids) return -1;
    try {
        return b->e->step_replay(init, ids, n, prop);
    } catch (const std::exception& x) {  // (the host model's replay: nothing crosses the C ABI)
        set_error(x.what());
        return -1;
    }
}

int64_t sr_step_host(int32_t model, const int64_t* p, int32_t np, int32_t prop, int64_t max_states, sr_step_result* out,
                     int64_t* action_ids, int32_t cap) {
    try {
        if (!out || out->struct_size < 2 * sizeof(uint32_t) || max_states < 1 || (cap > 0 && !action_ids))
            throw Error(SR_ERR_ARG, "sr_step_host: a sized result struct, max_states >= 1 and a buffer of cap");
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            using M = std::decay_t<decltype(m)>;
            if constexpr (!has_smask<M>::value) {
                throw Error(SR_ERR_ARG, "step pass: the model has no step property");
            } else {
                const StepHost h = step_host(m, prop, (u64)max_states);
                step_copy_out(h.r, out);
                for (size_t i = 0; i < h.actions.size() && (int64_t)i < cap; ++i) action_ids[i] = h.actions[i];
                return (i64)h.unique;
            }
        });
        if (r == SR_ERR_UNSUPPORTED) set_error("sr_step_host: model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int64_t sr_host_graph(int32_t model, const int64_t* p, int32_t np, int64_t max_states, int64_t* out, int64_t cap) {
    try {
        if (max_states < 1 || (cap > 0 && !out)) throw Error(SR_ERR_ARG, "sr_host_graph: max_states >= 1 and a buffer of cap");
        const i64 r = with_host_model(model, p, np, [&](const auto& m) -> i64 {
            using M = std::decay_t<decltype(m)>;
            constexpr int W = M::W;
            std::map<std::vector<u64>, i64> index;
            std::vector<std::vector<u64>> st;
            auto add = [&](const u64* s) {
                std::vector<u64> v(s, s + W);
                auto it = index.find(v);
                if (it != index.end()) return it->second;
                if ((i64)st.size() >= max_states)
                    throw Error(SR_ERR_CAPACITY, "sr_host_graph: more than " + std::to_string(max_states) + " reachable states (max_states)");
                index.emplace(v, (i64)st.size());
                st.push_back(std::move(v));
                return (i64)st.size() - 1;
            };
            std::vector<i64> dump{0, 0, M::NPROPS};
            const std::vector<u64> inits = init_states_of(m);
            for (size_t i = 0; i + W <= inits.size(); i += W) dump.push_back(add(&inits[i]));
            dump[1] = (i64)dump.size() - 3;
            for (size_t q = 0; q < st.size(); ++q) {
                const std::vector<u64> s = st[q];  // (a copy: add() grows st)
                i64 conds = 0;
                for (int pr = 0; pr < M::NPROPS; ++pr)
                    if ((m.expectation(pr) == ALWAYS) != m.discovers(pr, s.data())) conds |= (i64)1 << pr;
                dump.push_back(conds);
                const size_t at = dump.size();
                dump.push_back(0);
                for_each_successor(m, s.data(), [&](int a, const u64* ns) {
                    dump.push_back(m.action_id(s.data(), a));
                    dump.push_back(add(ns));
                    dump[at] += 1;
                });
            }
            dump[0] = (i64)st.size();
            std::copy(dump.begin(), dump.begin() + (size_t)std::min<i64>(std::max<i64>(cap, 0), (i64)dump.size()), out);
            return (i64)dump.size();
        });
        if (r == SR_ERR_UNSUPPORTED) set_error("sr_host_graph: model " + std::to_string(model) + " has no host form");
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

// Until the check's driver job has finished: a spin for the first ~20 ms (a short check's end is
// seen at once), then polls every 50 us.
static void wait_finished(sr_bfs* b) {
    const auto t0 = std::chrono::steady_clock::now();
    for (u32 spin = 1; !b->e->finished.load(std::memory_order_acquire); ++spin) {
        if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        else
            _mm_pause();
    }
}

int32_t sr_gpu_bfs_join(sr_bfs* b) {
    if (!b) return SR_ERR_ARG;
    if (!b->joined) {
        wait_finished(b);
        b->joined = true;
    }
    if (b->e->status != SR_OK) set_error(b->e->error);
    return b->e->status;
}

int32_t sr_gpu_bfs_is_done(const sr_bfs* b) { return b && b->e->finished && b->e->reference_done ? 1 : 0; }
int32_t sr_gpu_bfs_is_running(const sr_bfs* b) { return b && !b->e->finished ? 1 : 0; }
uint64_t sr_gpu_bfs_state_count(const sr_bfs* b) { return b ? b->e->state_count.load() : 0; }
uint64_t sr_gpu_bfs_unique_state_count(const sr_bfs* b) { return b ? b->e->unique.load() : 0; }
uint32_t sr_gpu_bfs_max_depth(const sr_bfs* b) { return b ? b->e->max_depth.load() : 0; }

int32_t sr_gpu_bfs_stats(const sr_bfs* b, sr_stats* out) {
    if (!b || !out) return SR_ERR_ARG;
    *out = b->e->stats;
    return SR_OK;
}

int32_t sr_gpu_bfs_stats_sized(const sr_bfs* b, sr_stats* out, uint32_t size) {
    if (!b || (!out && size)) return SR_ERR_ARG;
    if (out) std::memcpy(out, &b->e->stats, std::min<size_t>(size, sizeof(sr_stats)));
    return (int32_t)sizeof(sr_stats);
}

int64_t sr_gpu_bfs_launch_profile(const sr_bfs* b, double* kernel_ms, uint64_t* frontier, int64_t cap) {
    if (!b) return SR_ERR_ARG;
    const auto& ms = b->e->launch_ms;
    const auto& fr = b->e->launch_frontier;
    const int64_t n = (int64_t)ms.size();
    for (int64_t i = 0; i < std::min(n, cap); ++i) {
        if (kernel_ms) kernel_ms[i] = ms[i];
        if (frontier) frontier[i] = i < (int64_t)fr.size() ? fr[i] : 0;
    }
    return n;
}

int64_t sr_gpu_bfs_launch_counters(const sr_bfs* b, uint64_t* probes, uint64_t* cas, int64_t cap) {
    if (!b) return SR_ERR_ARG;
    const auto& pr = b->e->launch_probes;
    const auto& cs = b->e->launch_cas;
    const int64_t n = (int64_t)pr.size();
    for (int64_t i = 0; i < std::min(n, cap); ++i) {
        if (probes) probes[i] = pr[i];
        if (cas) cas[i] = i < (int64_t)cs.size() ? cs[i] : 0;
    }
    return n;
}

int32_t sr_gpu_bfs_property_count(const sr_bfs* b) { return b ? b->e->nprops() : 0; }

int32_t sr_gpu_bfs_property(const sr_bfs* b, int32_t p, char* name, int32_t cap, int32_t* expectation) {
    if (!b || p < 0 || p >= b->e->nprops()) return SR_ERR_ARG;
    const char* n = b->e->prop_name(p);
    if (name && cap > 0) std::snprintf(name, (size_t)cap, "%s", n);
    if (expectation) *expectation = b->e->expectation(p);
    return (int32_t)std::strlen(n);
}

int32_t sr_gpu_bfs_discovery(const sr_bfs* b, int32_t p, uint64_t* fp_chain, uint32_t cap) {
    try {
        if (!b) return SR_ERR_ARG;
        std::vector<u64> c;
        b->e->chain(p, c);
        if (fp_chain) std::memcpy(fp_chain, c.data(), std::min<size_t>(cap, c.size()) * sizeof(u64));
        return (int32_t)c.size();
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int32_t sr_gpu_bfs_discovery_path(const sr_bfs* b, int32_t p, int64_t* action_ids, int32_t cap_actions,
                                  int64_t* states, int64_t cap_states) {
    try {
        if (!b) return SR_ERR_ARG;
        std::vector<i64> a, s;
        int n = b->e->path(p, a, s);
        if (n < 0) return -1;
        if (action_ids) std::memcpy(action_ids, a.data(), std::min<size_t>((size_t)cap_actions, a.size()) * sizeof(i64));
        if (states) std::memcpy(states, s.data(), std::min<size_t>((size_t)cap_states, s.size()) * sizeof(i64));
        return n;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int32_t sr_gpu_bfs_describe_width(const sr_bfs* b) { return b ? b->e->width() : 0; }

int32_t sr_gpu_bfs_action_name(const sr_bfs* b, int64_t id, char* buf, int32_t cap) {
    if (!b) return SR_ERR_ARG;
    std::string s = b->e->action_name(id);
    if (buf && cap > 0) std::snprintf(buf, (size_t)cap, "%s", s.c_str());
    return (int32_t)s.size();
}

int64_t sr_gpu_bfs_visits(const sr_bfs* b, int64_t* out, int64_t cap) {
    if (!b) return SR_ERR_ARG;
    auto v = b->e->visits();
    if (out) std::memcpy(out, v.data(), (size_t)std::min<int64_t>(cap, (int64_t)v.size()) * sizeof(int64_t));
    return (int64_t)v.size();
}

int64_t sr_gpu_bfs_visit_tree(const sr_bfs* b, int64_t* parent, int64_t* action, int64_t cap) {
    try {
        if (!b) return SR_ERR_ARG;
        std::vector<i64> p, a;
        if (!b->e->visit_tree(p, a)) {
            set_error("this check kept no visit record (sr_opts.record_visits = 0)");
            return SR_ERR_UNSUPPORTED;
        }
        const size_t n = std::min<size_t>((size_t)std::max<int64_t>(cap, 0), p.size());
        if (parent) std::memcpy(parent, p.data(), n * sizeof(i64));
        if (action) std::memcpy(action, a.data(), n * sizeof(i64));
        return (int64_t)p.size();
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int64_t sr_gpu_bfs_action_id_bound(const sr_bfs* b) { return b ? b->e->action_id_bound() : 0; }
int32_t sr_gpu_bfs_init_count(const sr_bfs* b) { return b ? b->e->init_count() : 0; }

int32_t sr_gpu_bfs_replay_trace(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int32_t* conditions,
                                int64_t cap, int32_t* terminal) {
    if (!b) return SR_ERR_ARG;
    std::vector<i64> s;
    std::vector<int> c, all;
    int term = 0;
    int r = b->e->replay(init, ids, n, s, c, &all, &term);
    if (r < 0) return -1;
    for (int64_t i = 0; i < (int64_t)all.size() && i < cap; ++i) conditions[i] = all[i];
    if (terminal) *terminal = term;
    return r;
}

int32_t sr_gpu_bfs_explore(const sr_bfs* b, const uint64_t* fps, int32_t n, int64_t* action_ids, int32_t* has_state,
                           uint64_t* fp_out, int64_t* states, int32_t cap) {
    try {
        if (!b || (n > 0 && !fps)) return SR_ERR_ARG;
        std::vector<i64> a, st;
        std::vector<int> h;
        std::vector<u64> f;
        const int v = b->e->explore(fps, n, a, h, f, st);
        if (v < 0) {
            set_error("Unable to find state following fingerprints");
            return -1;
        }
        const int wd = b->e->width();
        for (int i = 0; i < v && i < cap; ++i) {
            if (action_ids) action_ids[i] = a[i];
            if (has_state) has_state[i] = h[i];
            if (fp_out) fp_out[i] = f[i];
            if (states) std::memcpy(states + (size_t)i * wd, st.data() + (size_t)i * wd, wd * sizeof(i64));
        }
        return v;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int32_t sr_gpu_bfs_replay(const sr_bfs* b, int32_t init, const int64_t* ids, int32_t n, int64_t* states, int64_t cap_states,
                          int32_t* conds, int32_t cap_conds) {
    if (!b) return SR_ERR_ARG;
    std::vector<i64> s;
    std::vector<int> c;
    int r = b->e->replay(init, ids, n, s, c);
    if (r < 0) return -1;
    if (states) std::memcpy(states, s.data(), (size_t)std::min<int64_t>(cap_states, (int64_t)s.size()) * sizeof(int64_t));
    for (int i = 0; i < (int)c.size() && i < cap_conds; ++i) conds[i] = c[i];
    return r;
}


int32_t sr_dist_unique_id(uint8_t* out) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) {
        set_error("ncclGetUniqueId failed");
        return SR_ERR_HIP;
    }
    static_assert(sizeof(ncclUniqueId) == SR_DIST_ID_BYTES, "RCCL unique id size");
    std::memcpy(out, &id, sizeof(id));
    return SR_OK;
}

sr_dist* sr_dist_init(int32_t rank, int32_t world, const uint8_t* idb, int32_t device) {
    try {
        if (world < 1 || rank < 0 || rank >= world) throw Error(SR_ERR_ARG, "bad rank/world");
        SR_HIP(hipSetDevice(device));
        auto c = std::make_unique<RcclComm>();
        c->rank = rank;
        c->world = world;
        c->device = device;
        ncclUniqueId id;
        std::memcpy(&id, idb, sizeof(id));
        SR_NCCL(ncclCommInitRank(&c->nccl, world, id, rank));
        auto d = std::make_unique<sr_dist>();
        d->c = std::move(c);
        return d.release();
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

int32_t sr_dist_local_group(int32_t world, const int32_t* devices, sr_dist** out) {
    try {
        if (world < 1 || !out) throw Error(SR_ERR_ARG, "bad world/out");
        auto g = std::make_shared<LocalGroup>(world);
        for (int r = 0; r < world; ++r) {
            auto c = std::make_unique<LocalComm>();
            c->rank = r;
            c->world = world;
            c->device = devices ? devices[r] : 0;
            c->g = g;
            g->devices[r] = c->device;
            auto d = std::make_unique<sr_dist>();
            d->c = std::move(c);
            out[r] = d.release();
        }
        return SR_OK;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

sr_dist* sr_dist_shm_init(int32_t rank, int32_t world, const char* name, int32_t device, int64_t slot_bytes,
                          int32_t devices_distinct) {
    try {
        if (world < 1 || rank < 0 || rank >= world || !name || slot_bytes < 4096) throw Error(SR_ERR_ARG, "bad shm communicator");
        SR_HIP(hipSetDevice(device));
        auto d = std::make_unique<sr_dist>();
        d->c = std::make_unique<ShmComm>(rank, world, std::string(name), device, (size_t)slot_bytes, devices_distinct != 0);
        return d.release();
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

int32_t sr_dist_host_protocol(const char* name, int32_t rank, int32_t world, const sr_dist_host_opts* opts,
                              sr_dist_host_result* out) {
    try {
        if (world < 1 || rank < 0 || rank >= world || !name || !opts || !out) throw Error(SR_ERR_ARG, "bad host protocol run");
        sr_dist_host_opts o;
        std::memset(&o, 0, sizeof(o));
        std::memcpy(&o, opts, std::min<size_t>(sizeof(o), opts->struct_size ? opts->struct_size : sizeof(o)));
        if (o.rm_count < 1 || o.rm_count > 7) throw Error(SR_ERR_UNSUPPORTED, "host protocol run: rm_count must be in 1..=7");
        ShmComm c(rank, world, std::string(name), -1, (size_t)1 << 24, false);
        c.host_only = true;
        DistHostRun run(c, o);
        const int r = run.run();
        *out = run.r;
        return r;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int32_t sr_dist_rank(const sr_dist* d) { return d ? d->c->rank : SR_ERR_ARG; }
int32_t sr_dist_world(const sr_dist* d) { return d ? d->c->world : SR_ERR_ARG; }
int32_t sr_dist_nranks(const sr_dist* d) { return d ? d->c->nranks() : SR_ERR_ARG; }
int32_t sr_dist_kind(const sr_dist* d, char* buf, int32_t cap) {
    if (!d) return SR_ERR_ARG;
    const char* k = d->c->kind();
    if (buf && cap > 0) std::snprintf(buf, (size_t)cap, "%s", k);
    return (int32_t)std::strlen(k);
}

int32_t sr_dist_barrier(sr_dist* d) {
    try {
        if (!d) return SR_ERR_ARG;
        SR_HIP(hipSetDevice(d->c->device));
        SR_HIP(hipDeviceSynchronize());
        d->c->barrier(d->get_stream());
        return SR_OK;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

int32_t sr_dist_allreduce_f64(sr_dist* d, double* values, int32_t n, int32_t op) {
    try {
        if (!d || !values || n < 1 || op < 0 || op > 2) return SR_ERR_ARG;
        // doubles travel as order-preserving u64 keys, so min and max are exact (no sum)
        if (op == 2) throw Error(SR_ERR_ARG, "sr_dist_allreduce_f64: only min (0) and max (1)");
        std::vector<u64> k(n);
        for (int i = 0; i < n; ++i) {
            u64 b;
            std::memcpy(&b, &values[i], 8);
            k[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
        }
        SR_HIP(hipSetDevice(d->c->device));
        hipStream_t s = d->get_stream();
        DBuf<u64> buf;
        buf.alloc(d->c->device, n);
        SR_HIP(hipMemcpyAsync(buf.p, k.data(), n * 8, hipMemcpyHostToDevice, s));
        d->c->all_reduce(buf.p, n, op == 0 ? RedOp::Min : RedOp::Max, s);
        SR_HIP(hipMemcpyAsync(k.data(), buf.p, n * 8, hipMemcpyDeviceToHost, s));
        SR_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) {
            const u64 b = (k[i] >> 63) ? (k[i] & 0x7fffffffffffffffull) : ~k[i];
            std::memcpy(&values[i], &b, 8);
        }
        return SR_OK;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    }
}

void sr_dist_free(sr_dist* d) {
    if (!d) return;
    if (d->stream && hipStreamDestroy(d->stream) == hipSuccess) StreamCensus::get().destroyed(d->c->device);
    delete d;
}

int32_t sr_rccl_version(int32_t* runtime, int32_t* compiled) {
    int v = 0;
    if (ncclGetVersion(&v) != ncclSuccess) return SR_ERR_HIP;
    if (runtime) *runtime = v;
    if (compiled) *compiled = NCCL_VERSION_CODE;
    return SR_OK;
}

#ifndef SR_BUILD_DIGEST
#define SR_BUILD_DIGEST "unstamped"
#endif
const char* sr_build_digest(void) { return SR_BUILD_DIGEST; }

int32_t sr_hip_runtime_version(int32_t* runtime, int32_t* compiled) {
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) return SR_ERR_HIP;
    if (runtime) *runtime = v;
    if (compiled) *compiled = HIP_VERSION;
    return SR_OK;
}

int32_t sr_selftest_tables(void) {
    // qperm is a bijection on B bits (exhaustive for small B)
    for (u32 B = 1; B <= 18; ++B) {
        std::vector<u8> seen(1u << B, 0);
        for (u64 x = 0; x < (1ull << B); ++x) {
            const u64 y = (u64)qperm(x, B);
            if (y >> B || seen[y]) {
                set_error("qperm is not a bijection on " + std::to_string(B) + " bits");
                return SR_ERR_ARG;
            }
            seen[y] = 1;
        }
    }
    // qmix (one-word keys) is a bijection on B bits
    for (u32 B = 2; B <= 20; ++B) {
        std::vector<u8> seen(1u << B, 0);
        for (u64 x = 0; x < (1ull << B); ++x) {
            const u64 y = qmix(x, B);
            if (y >> B || seen[y]) {
                set_error("qmix is not a bijection on " + std::to_string(B) + " bits");
                return SR_ERR_ARG;
            }
            seen[y] = 1;
        }
    }
    // narrow (32-bit) quotient slots: 2pc N=9..12 keys in their tables, and a table larger than
    // the key space (remainder 1 bit); the filter key gives the permuted key back
    const u32 ncases[][2] = {{40, 25}, {40, 22}, {44, 27}, {48, 29}, {52, 31}, {16, 22}, {62, 40}};
    u64 rn = 0x452821E638D01377ull;
    for (auto& c : ncases) {
        const u32 q = c[0] > c[1] ? c[0] - c[1] : 1u;
        TableView t{nullptr, nullptr, (1ull << c[1]) - 1, q, 32 - q, c[0]};
        t.s32 = 1;
        if (q + SLOT32_DMIN > 32) {
            t.s32 = 0;
            t.dbits = 64 - q;
        }
        for (int i = 0; i < 100000; ++i) {
            rn = fmix64(rn + 0x9E3779B97F4A7C15ull);
            const u64 key = rn & ((1ull << c[0]) - 1);
            const u64 h = qmix(key, c[0]);
            const ProbeKey pk = quot_probe(t, h);
            const u64 d = (rn >> 40) % 500;
            const u64 slotv = pk.tag + d;
            if ((t.s32 && slotv >> 32) || quot_decode(t, (pk.home + d) & t.mask, slotv) != h || pk.home > t.mask ||
                filter_key(t, pk) != h + 1) {
                set_error("narrow quotient slot encode/decode mismatch at B=" + std::to_string(c[0]));
                return SR_ERR_ARG;
            }
        }
    }
    // quotient slot values decode to the key at every displacement (B = 89, k = 33: increment_lock
    // N=12's table; B = 68, k = 20)
    const u32 cases[][2] = {{89, 33}, {68, 20}, {82, 26}, {120, 64}};
    u64 r = 0x243F6A8885A308D3ull;
    for (auto& c : cases) {
        TableView t{nullptr, nullptr, (c[1] >= 64 ? ~0ull : (1ull << c[1]) - 1), c[0] - c[1], 64 - (c[0] - c[1]), c[0]};
        for (int i = 0; i < 100000; ++i) {
            r = fmix64(r + 0x9E3779B97F4A7C15ull);
            const u64 r2 = fmix64(r ^ 0xABCDEFull);
            const u128 key = ((u128)r2 << 64 | r) & (((u128)1 << c[0]) - 1);
            const u128 h = qperm(key, c[0]);
            const ProbeKey pk = quot_probe(t, h);
            const u64 d = r2 % 200;
            if (quot_decode(t, (pk.home + d) & t.mask, pk.tag + d) != h || pk.home > t.mask || (pk.tag & ((1ull << t.dbits) - 1)) != 1) {
                set_error("quotient slot encode/decode mismatch at B=" + std::to_string(c[0]));
                return SR_ERR_ARG;
            }
        }
    }
    return SR_OK;
}

int32_t sr_selftest_table_growth(void) {
    try {
        std::string why;
        if (!table_growth_selftest(why)) {
            set_error(why);
            return SR_ERR_ARG;
        }
        return SR_OK;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int32_t sr_selftest_rehash_gpu(int32_t device) {
    try {
        std::string why;
        if (!rehash_test::run_all(device, why, device < 0)) {
            set_error(why);
            return SR_ERR_ARG;
        }
        return SR_OK;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int32_t sr_selftest_certify_gpu(int32_t device) {
    try {
        std::string why;
        if (!cert_test::run_all(device, why, device < 0)) {
            set_error(why);
            return SR_ERR_ARG;
        }
        return SR_OK;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

int32_t sr_gpu_bfs_certificate(const sr_bfs* b, sr_certificate* out, uint32_t size) {
    if (!b || (!out && size) || !b->e->finished.load(std::memory_order_acquire)) return SR_ERR_ARG;
    if (out) std::memcpy(out, &b->e->cert, std::min<size_t>(size, sizeof(sr_certificate)));
    return (int32_t)sizeof(sr_certificate);
}

int32_t sr_gpu_bfs_table_audit(const sr_bfs* b, sr_table_audit* out, uint32_t size) {
    if (!b || (!out && size)) return SR_ERR_ARG;
    if (out) std::memcpy(out, &b->e->audit, std::min<size_t>(size, sizeof(sr_table_audit)));
    return (int32_t)sizeof(sr_table_audit);
}

int32_t sr_table_encoding(int32_t words, int32_t key_bits, uint64_t slots, uint32_t* out) {
    try {
        if (!out || key_bits < 2 || (words != 1 && words != 2 && words != 4) || key_bits > std::min(64 * words, 128) ||
            !slots || (slots & (slots - 1)))
            throw Error(SR_ERR_ARG, "sr_table_encoding: words 1, 2 or 4, 2 <= key_bits <= min(64 words, 128), slots a power of two");
        const TableEncoding e = words == 1   ? table_encoding_of<1>(key_bits, slots)
                                : words == 2 ? table_encoding_of<2>(key_bits, slots)
                                             : table_encoding_of<4>(key_bits, slots);
        const u32 v[8] = {e.qbits, e.dbits, e.bbits, e.plimit, e.s32, e.filter, e.filter_log2, e.min_cap_log2};
        std::copy(v, v + 8, out);
        return SR_OK;
    } catch (const Error& x) {
        set_error(x.what());
        return x.code;
    } catch (const std::exception& x) {
        set_error(x.what());
        return SR_ERR_ARG;
    }
}

// expand_fast's level geometry (kernels.hpp LevelGeom / level_geometry) walked on the host the way
// the kernel walks it: workgroup b from first_chunk in steps of stride while the chunk starts below
// hi, wave wid's lanes l < pw at wave_first + l below chunk_end. A wave's ranks are an interval, so
// the walk records intervals: they must tile [lo, hi) (every parent exactly once, none outside).
// Also pw <= cap, cw <= wpb cap, workgroup shares within one chunk width of each other, and with
// the switch off the waves of the shift formula the kernel used before.
static bool check_level_geometry(u32 nblk, std::vector<u32>& stamp, std::vector<u32>& end, u32& gen,
                                 const std::vector<u32>& ns, std::string& why) {
    for (u32 wpb : {4u, 8u})
        for (u32 cap_log2 = 2; cap_log2 <= 6; ++cap_log2)
            for (int balanced = 0; balanced < 2; ++balanced)
                for (u32 n : ns) {
                    const u32 cap = 1u << cap_log2, lo = n & 1 ? 77u : 0u, hi = lo + n;
                    const LevelGeom g = level_geometry(n, nblk, wpb, cap, balanced != 0);
                    auto fail = [&](const char* what) {
                        why = std::string("level geometry: ") + what + " at n=" + std::to_string(n) + " nblk=" +
                              std::to_string(nblk) + " cap=" + std::to_string(cap) + " wpb=" + std::to_string(wpb) +
                              (balanced ? " balanced" : " fixed");
                        return false;
                    };
                    if (g.pw == 0 || g.pw > cap || g.cw == 0 || g.cw > wpb * cap) return fail("pw or cw out of range");
                    if (!balanced && (g.pw != cap || g.cw != wpb * cap)) return fail("fixed geometry changed");
                    ++gen;
                    u64 intervals = 0, share_min = ~0ull, share_max = 0;
                    for (u32 b = 0; b < nblk; ++b) {
                        u64 share = 0;
                        u64 j = 0;  // the workgroup's j-th chunk
                        for (u64 c0 = g.first_chunk(lo, b); c0 < hi; c0 += g.stride(nblk), ++j) {
                            const u32 lim = g.chunk_end(c0, hi);
                            for (u32 wid = 0; wid < wpb; ++wid) {
                                const u64 w0 = g.wave_first(c0, wid);
                                const u64 w1 = std::min<u64>(w0 + g.pw, lim);  // lanes l < pw with w0 + l < lim
                                if (!balanced) {  // the shift formula: lanes l < 2^cap_log2 with rank < hi
                                    const u64 o0 = lo + (((u64)b + j * nblk) * wpb << cap_log2) + ((u64)wid << cap_log2);
                                    const u64 o1 = std::min<u64>(o0 + cap, hi);
                                    if (o0 < o1 ? o0 != w0 || o1 != w1 : w0 < w1) return fail("differs from the shift formula");
                                }
                                if (w1 <= w0) continue;
                                if (w0 < lo || w1 > hi) return fail("a parent outside the frontier");
                                if (stamp[w0 - lo] == gen) return fail("a parent taken twice");
                                stamp[w0 - lo] = gen;
                                end[w0 - lo] = (u32)(w1 - lo);
                                share += w1 - w0;
                                ++intervals;
                            }
                        }
                        share_min = std::min(share_min, share);
                        share_max = std::max(share_max, share);
                    }
                    u64 followed = 0;
                    u32 pos = 0;
                    while (pos < n) {
                        if (stamp[pos] != gen) return fail("a parent not taken");
                        pos = end[pos];
                        ++followed;
                    }
                    if (pos != n || followed != intervals) return fail("waves overlap");
                    if (share_max - share_min > g.cw) return fail("workgroup shares differ by more than one chunk");
                }
    return true;
}

int32_t sr_selftest_level_geometry(void) {
    std::vector<u32> ns;
    for (u32 n = 0; n <= 2048; ++n) ns.push_back(n);
    for (u32 k = 12; k <= 21; ++k)
        for (u32 n : {(1u << k) - 1, 1u << k, (1u << k) + 1}) ns.push_back(n);
    std::vector<u32> nblks;
    for (u32 b = 1; b <= 48; ++b) nblks.push_back(b);
    for (u32 b : {1535u, 1536u, 1537u}) nblks.push_back(b);
    // (one worker per slice of the workgroup counts: ~10^9 wave intervals in all)
    const u32 workers = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::string> why(workers);
    std::vector<std::thread> pool;
    for (u32 w = 0; w < workers; ++w)
        pool.emplace_back([&, w] {
            std::vector<u32> stamp((1u << 21) + 2, 0), end((1u << 21) + 2, 0);
            u32 gen = 0;
            for (size_t i = w; i < nblks.size() && why[w].empty(); i += workers)
                check_level_geometry(nblks[i], stamp, end, gen, ns, why[w]);
        });
    for (auto& t : pool) t.join();
    for (auto& s : why)
        if (!s.empty()) {
            set_error(s);
            return SR_ERR_ARG;
        }
    return SR_OK;
}

// PaxosHist::linearizable (the cluster-graph test) against PaxosHist::linearizable_search (the
// tester's serialization search) on random histories of the register clients' protocol (every
// client: Write invoked at init; on its completion the Read is invoked, recording how many ops every
// other client had completed; the Read completes with any value): all client counts 1..6.
static bool check_linearizability(std::string& why) {
    u64 x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { return x = fmix64(x + 0x632BE59BD9B4E019ull); };
    for (u32 C = 1; C <= px::MAX_CLIENTS; ++C) {
        PaxosHist h;
        h.C = C;
        u32 nonlin = 0;
        for (int it = 0; it < 40000; ++it) {
            u64 lo = 0, hi = 0;
            const u32 steps = (u32)(rnd() % (2 * C + 1));
            for (u32 k = 0; k < steps; ++k) {
                const u32 t = (u32)(rnd() % C), ph = h.phase(lo, hi, t);
                if (ph == 0) {
                    for (u32 u = 0; u < C; ++u)
                        if (u != t) PaxosHist::put(lo, hi, h.last_off(t, u), 2, h.phase(lo, hi, u));
                } else if (ph == 1) {
                    PaxosHist::put(lo, hi, h.ret_off(t), 3, rnd() % (C + 1));
                } else {
                    continue;
                }
                PaxosHist::put(lo, hi, 2 * t, 2, ph + 1);
            }
            const bool a = h.linearizable(lo, hi), b = h.linearizable_search(lo, hi);
            nonlin += !b;
            if (a != b) {
                why = "linearizability: C=" + std::to_string(C) + " history " + std::to_string(lo) + "/" + std::to_string(hi) +
                      ": cluster test " + std::to_string(a) + ", search " + std::to_string(b);
                return false;
            }
        }
        if (C >= 2 && nonlin == 0) {
            why = "linearizability: no non-linearizable history drawn at C=" + std::to_string(C);
            return false;
        }
    }
    return true;
}

int32_t sr_selftest_models(void) {
    std::string why;
    if (!check_linearizability(why)) {
        set_error(why);
        return SR_ERR_ARG;
    }
    for (int n = 1; n <= 7; ++n) {
        TwoPhase m;
        m.n = n;
        if (!sr::check_self_loops(m, why)) {
            set_error("2pc n=" + std::to_string(n) + ": " + why);
            return SR_ERR_ARG;
        }
        if (n <= 6 && !sr::check_self_loops(Canon<TwoPhase>(m), why)) {
            set_error("2pc n=" + std::to_string(n) + " (canonical): " + why);
            return SR_ERR_ARG;
        }
    }
    return SR_OK;
}

int32_t sr_selftest_action_masks(void) {
    std::string why;
    auto bad = [&](const std::string& who) {
        set_error(who + ": " + why);
        return (int32_t)SR_ERR_ARG;
    };
    for (int n = 1; n <= 14; ++n) {
        TwoPhase m;
        m.n = n;
        if (!sr::check_action_masks(m, 4 * n + 4, n <= 4, 10000, why)) return bad("2pc n=" + std::to_string(n));
    }
    if (!sr::check_action_masks(TwoPhaseT<9>{9}, 40, false, 10000, why)) return bad("2pc n=9 (compiled in)");
    if (!sr::check_action_masks(TwoPhaseT<10>{10}, 44, false, 10000, why)) return bad("2pc n=10 (compiled in)");
    if (!sr::check_action_masks(TwoPhaseT<11>{11}, 48, false, 10000, why)) return bad("2pc n=11 (compiled in)");
    if (!sr::check_action_masks(Ladder{5, 3}, 9, true, 512, why)) return bad("ladder 5+3");
    if (!sr::check_action_masks(Ladder{58, 8}, 14, false, 10000, why)) return bad("ladder 58+8");
    return SR_OK;
}

int32_t sr_device_synchronize(int32_t device) {
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        set_error("hipDeviceSynchronize failed");
        return SR_ERR_HIP;
    }
    return SR_OK;
}

sr_bfs* sr_gpu_bfs_spawn_partitioned(sr_dist* comm, int32_t virtual_parts, int32_t model_id, const int64_t* params,
                                     int32_t nparams, const sr_opts* opts) {
    try {
        sr_opts o = normalized_opts(opts);
        refuse_liveness(o, true, false);
        refuse_coverage(o, true);
        if (comm) o.device = comm->c->device;
        if (sr_device_count() <= 0) throw Error(SR_ERR_NO_DEVICE, "no HIP device visible");
        return start(make_model_engine(EngineArgs{model_id, params, nparams, &o, true, comm ? comm->c.get() : nullptr, (int)virtual_parts}));
    } catch (const std::exception& x) {
        set_error(x.what());
        return nullptr;
    }
}

void sr_gpu_bfs_free(sr_bfs* b) {
    if (!b) return;
    if (!b->joined) wait_finished(b);  // the pooled driver thread must be done with the engine
    delete b;
}

}  // extern "C"

#if SR_TIMELINE
// ---- diagnostic build only (SR_TIMELINE=1): expand_fast's per-workgroup timeline ----
static u64* g_timeline_host_ptr = nullptr;
extern "C" int64_t sr_timeline_reset(int32_t device) {
    const size_t words = (size_t)TL_LAUNCHES * TL_BLOCKS * TL_STAMPS;
    if (hipSetDevice(device) != hipSuccess) return SR_ERR_HIP;
    if (!g_timeline_host_ptr) {
        if (hipMalloc(&g_timeline_host_ptr, words * 8) != hipSuccess) return SR_ERR_HIP;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &g_timeline_host_ptr, sizeof(u64*)) != hipSuccess) return SR_ERR_HIP;
    }
    if (hipMemset(g_timeline_host_ptr, 0, words * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SR_ERR_HIP;
    return (int64_t)words;
}
extern "C" int64_t sr_timeline_fetch(int32_t device, uint64_t* out, int64_t cap) {
    const size_t words = (size_t)TL_LAUNCHES * TL_BLOCKS * TL_STAMPS;
    if (!g_timeline_host_ptr || hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SR_ERR_HIP;
    if (out && hipMemcpy(out, g_timeline_host_ptr, std::min<size_t>(words, (size_t)cap) * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return SR_ERR_HIP;
    return (int64_t)words;
}
#endif

#ifdef SR_ONE_TU
// One translation unit (diagnostic builds, scripts/build_timeline.sh): the registry families too.
#include "reg_basic.hip"
#include "reg_two_phase.hip"
#include "reg_increment.hip"
#include "reg_increment_lock.hip"
#include "reg_paxos.hip"
#include "reg_paxos_wide.hip"
#include "reg_ping_pong.hip"
#include "reg_registers.hip"
#include "reg_registers_wide.hip"
#include "reg_spread.hip"
#endif
