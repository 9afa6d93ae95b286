/*
 * stateright_gpu.h — C ABI of the MI355X breadth-first model-checking engine.
 *
 * This is the drop-in boundary for Stateright's `CheckerBuilder::spawn_bfs` path. Each entry point
 * replaces one piece of the reference's Rust interface (crate `stateright` 0.28.0, paths relative to
 * the reference repository):
 *
 *   sr_gpu_bfs_spawn              <- CheckerBuilder::spawn_bfs        src/checker.rs:124-129
 *                                    BfsChecker::spawn                src/checker/bfs.rs:36-163
 *                                    (builder options threads/target_state_count/visitor:
 *                                     src/checker.rs:35-51,162-177, mirrored by sr_opts)
 *   sr_gpu_bfs_join               <- Checker::join                    src/checker/bfs.rs:300-305
 *   sr_gpu_bfs_is_done            <- Checker::is_done                 src/checker/bfs.rs:307-311
 *   sr_gpu_bfs_state_count        <- Checker::state_count             src/checker/bfs.rs:283-285
 *   sr_gpu_bfs_unique_state_count <- Checker::unique_state_count      src/checker/bfs.rs:287
 *   sr_gpu_bfs_max_depth          <- (new: BFS depth metric, SURVEY.md §5 "no depth metric")
 *   sr_gpu_bfs_property_*         <- Model::properties / Property     src/lib.rs:214-300
 *   sr_gpu_bfs_discovery          <- discoveries() + reconstruct_path src/checker/bfs.rs:289-298,314-342
 *   sr_gpu_bfs_discovery_path     <- Path::from_fingerprints          src/checker/path.rs:20-86
 *   sr_gpu_bfs_replay             <- Path::from_actions (assert_discovery) src/checker/path.rs:90-112,
 *                                                                     src/checker.rs:292-337
 *   sr_gpu_bfs_visits             <- StateRecorder visitor            src/checker/visitor.rs:70-99
 *   sr_gpu_bfs_visit_tree         <- PathRecorder / Fn(Path) visitors src/checker/visitor.rs:19-66,
 *                                                                     src/checker/bfs.rs:187-189
 *   sr_gpu_bfs_free               <- Drop of the checker (join(self) consumes it in Rust)
 *   sr_last_error                 <- the reference panics; see "Errors" below
 *   sr_gpu_sim_spawn / sr_sim_walk <- new: the random-walk simulation checker (upstream's
 *                                    `spawn_simulation`, added after 0.28); see its section below
 *   sr_dist_* / sr_gpu_bfs_spawn_partitioned <- new: the visited set partitioned over GPUs
 *
 * Models: device code cannot call host function pointers, so `impl Model` becomes a registry of
 * compiled-in GpuModel encodings selected by `model_id` + integer parameters (SR_MODEL_*). Each
 * encoding packs one state into fixed-width 64-bit words and enumerates the reference's
 * `actions()` in order as action slots.
 *
 * Errors: the reference panics (zero fingerprint src/lib.rs:310, path nondeterminism
 * src/checker/path.rs:35-79, worker panics src/checker/bfs.rs:302). Here every call returns a
 * status (SR_OK or a negative SR_ERR_*) and sr_last_error() describes the last failure on the
 * calling thread. A check whose model reaches a state that its encoding cannot hold (the device's
 * ERR_MODEL bit: an actor network past its slots) ends with SR_ERR_UNSUPPORTED, "<model>: a state
 * exceeded its encoding (network slots)", without a capacity restart; its counts are not results.
 *
 * Threading: spawn returns immediately; the level loop runs on a host driver thread bound to one
 * HIP device. Counters are readable while it runs (like the reference's atomics).
 */
#ifndef STATERIGHT_GPU_H
#define STATERIGHT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Model registry (params in parentheses). */
enum sr_model_id {
    SR_MODEL_LINEAR_EQUATION = 1, /* (a, b, c)      src/test_util.rs:140-188            */
    SR_MODEL_BINARY_CLOCK = 2,    /* ()             src/test_util.rs:4-45               */
    SR_MODEL_2PC = 3,             /* (rm_count<=14) examples/2pc.rs:10-121              */
    SR_MODEL_INCREMENT = 4,       /* (threads<=15)  examples/increment.rs:109-197       */
    SR_MODEL_INCREMENT_LOCK = 5,  /* (threads<=12)  examples/increment_lock.rs:3-107    */
    SR_MODEL_DGRAPH = 6,          /* (expectation, len, v.., len, v..) src/test_util.rs:47-116 */
    SR_MODEL_PAXOS = 7,           /* (client_count<=6) examples/paxos.rs:93-263 + src/actor/model.rs */
    /* ActorModel fixtures (src/actor/model.rs:176-327 over stateright_amd/csrc/actor.hpp): */
    SR_MODEL_PINGPONG = 9,        /* (max_nat<=14, lossy, duplicating, maintains_history)
                                     src/actor/actor_test_util.rs:4-96                     */
    SR_MODEL_ACTOR_FIXTURE = 10,  /* (kind: 0 undeliverable envelope, 1 timer) src/actor/model.rs:697-733 */
    SR_MODEL_ABD = 11,            /* (client_count<=6, server_count<=4; <=8 actors) examples/linearizable-register.rs.
                                     The network of (C, S) holds at most B = C * max(1, 3d + S - 1, 4d)
                                     envelopes, d = S - majority: 8 slots when C, S <= 3 and B <= 8, else
                                     16 (B <= 16), else 32 (states then describe 32 envelopes) */
    SR_MODEL_SINGLE_COPY = 12,    /* (client_count<=6, server_count; <=8 actors) examples/single-copy-register.rs */
    SR_MODEL_LADDER = 13,         /* (rungs<=62, free_bits<=57) test fixture: rungs + free_bits action slots,
                                     (rungs + 1) * 2^free_bits states (stateright_amd/csrc/models.hpp Ladder) */
    SR_MODEL_SPREAD = 14,         /* (words: 1, 2 or 4; key_bits: free_bits < key_bits <= min(64 words, 128);
                                     free_bits<=24; loops<=4; mark < 2^free_bits) test fixture: the subsets of
                                     free_bits bits packed into a pseudo-random key of key_bits bits, so the
                                     visited set's slot encoding is a parameter; 2^free_bits states, `loops`
                                     unreported self-loops per state (stateright_amd/csrc/models.hpp Spread).
                                     Optionally followed by (roots, dup): the init states are the subsets
                                     0 .. roots-1, then 0 .. dup-1 again; 1 <= roots <= 2^free_bits,
                                     dup <= roots, roots + dup <= 512 (default 1, 0) */
    SR_MODEL_LIVE_GRAPH = 15,     /* (n_bits<=24, degree 1..4, seed, p_mod, t_mod, roots 1..512[, words[, dup]]) test fixture with
                                     cycles: states v < 2^n_bits; r(v, k) = fmix64(fmix64(seed ^ v) + k) (murmur3's
                                     finalizer); v has no actions iff t_mod > 0 and r(v, degree) % t_mod == 0, else
                                     slot k < degree leads to r(v, k) mod 2^n_bits (action id k); one `eventually`
                                     property "marked": p_mod > 0 and r(v, degree + 1) % p_mod == 0; init states
                                     0 .. roots-1; words = 1 (default), 2 or 4 pads the state with words that are
                                     functions of v; dup (default 0, <= roots, roots + dup <= 512) repeats the init
                                     states 0 .. dup-1 after the roots (stateright_amd/csrc/models.hpp LiveGraph) */
    SR_MODEL_2PC_LIVE = 16,       /* (rm_count<=14) SR_MODEL_2PC (same states, action slots and counts) with two
                                     `eventually` properties after its three: 3 "every RM decides" (every rm is
                                     Committed or Aborted), 4 "every RM commits". No reference counterpart: 2pc
                                     has no terminal state (once Commit or Abort is sent, RmRcvCommitMsg /
                                     RmRcvAbortMsg stay enabled as self-loops), so it is the model of the complete
                                     `eventually` check's progress mode (SR_LIVENESS_PROGRESS) */
    SR_MODEL_SPIN_LOCK = 17,      /* (threads 1..20) n threads take a lock in turn while a clock ticks; one word:
                                     holder (0 free, i + 1) in bits [0,5), served (n bits) from bit 5, tick above.
                                     Slot i < n Acquire(i) (the lock is free), n + i Release(i) (thread i holds it:
                                     serves i and frees the lock), 2n Tick (always: flips tick); (n + 1) 2^n 2 states.
                                     Two `eventually` properties: 0 "some thread served", 1 "every thread served".
                                     No reference counterpart: the model of the complete `eventually` check's
                                     weak-fairness mode (SR_LIVENESS_WEAK) */
    SR_MODEL_FAIR_RINGS = 18,     /* (d 1..28, w 4..64, core 0..2, lanes 1..512) nested rings; one word: position x
                                     in bits [0,6), ring k in [6,11), lane j in [11,20), done in bit 20. Lane j has
                                     the rings 0 .. d_j, d_j = 1 + (j mod d); its core is on iff core == 1, or
                                     core == 2 and j is odd. Slot 0 Step (x + 1 mod w); 1 + k Out(k), enabled at
                                     (k, 0): to `done` for k = 0, else to (k - 1, 0), and with the core on and
                                     k = d_j also at (k, 2), to (k, 0); d + 2 + k In(k), enabled at (k, 1) iff
                                     k < d_j: to (k + 1, 1). One `eventually` property "done"; init states
                                     (j, 0, 0). No reference counterpart and no oracle counterpart: the fixture of
                                     the complete `eventually` check's strong-fairness mode (SR_LIVENESS_STRONG),
                                     whose fair sets lie d_j levels deep inside unfair components */
    SR_MODEL_LEADS_GRAPH = 19,    /* (n_bits<=24, degree 1..4, seed, p_mod, t_mod, roots 1..512, q_mod[, words[, dup]])
                                     SR_MODEL_LIVE_GRAPH's graph, key and description with three properties:
                                     0 eventually "marked" (as there); 1 leads-to "armed ~> marked", whose trigger
                                     is q_mod > 0 and r(v, degree + 2) % q_mod == 0; 2 leads-to "always eventually
                                     marked", whose trigger is true. The fixture of the leads-to check */
    SR_MODEL_REQ_LOCK = 20,       /* (threads 1..8) a lock whose threads first ask for it, while a clock ticks; one
                                     word: holder (0 free, i + 1) in bits [0,5), waiting (n bits) from bit 5, tick
                                     above. Slot i < n Request(i) (i neither waits nor holds: sets waiting(i)), n + i
                                     Acquire(i) (the lock is free and i waits: i holds, waiting(i) cleared), 2n + i
                                     Release(i) (i holds: frees the lock), 3n Tick (always: flips tick);
                                     (2^n + n 2^(n-1)) 2 states. Properties p < n: leads-to "thread p waiting ~>
                                     thread p holds"; property n: eventually "some thread holds". The model of the
                                     leads-to check: refuted with no, progress and (n >= 2) weak fairness, proved
                                     under strong fairness */
    SR_MODEL_LEADS_DGRAPH = 21,   /* (n_trig, t.., len, v.., len, v..) SR_MODEL_DGRAPH's adjacency from paths, with
                                     an explicit list of trigger nodes; one leads-to property "trigger ~> odd" */
    SR_MODEL_STEP_GRAPH = 22,     /* (n_bits<=24, degree 1..4, seed, f_mod, t_mod, roots 1..512[, words[, dup]])
                                     SR_MODEL_LIVE_GRAPH's graph, key and description with two STEP properties and no
                                     other: 0 "no forbidden step", where the step (v, slot k) is forbidden iff
                                     f_mod > 0 and r(v, degree + 3 + k) % f_mod == 0 (f_mod: any non-negative int64);
                                     1 "never down", violated iff the successor is below v. The fixture of the step
                                     pass */
    SR_MODEL_2PC_STEP = 23,       /* (rm_count<=14) SR_MODEL_2PC (same states, action slots and counts) with two
                                     STEP properties after its three: 3 "a decided RM stays decided" (holds),
                                     4 "the TM never aborts once an RM is prepared" (refuted by RmPrepare, TmAbort) */
    SR_MODEL_STEP_DGRAPH = 24     /* (n_pairs<=16, src, dst, .., len, v.., len, v..) SR_MODEL_DGRAPH's adjacency from
                                     paths, with an explicit list of forbidden (src, dst) pairs; one step property
                                     "no forbidden step" */
};

/* Visit order inside a BFS level. */
enum sr_order {
    SR_ORDER_AUTO = 0, /* FAST; rerun as FIFO if an early exit makes counts order-dependent */
    SR_ORDER_FIFO = 1, /* exactly the single-threaded reference order (pop_back/push_front)   */
    SR_ORDER_FAST = 2  /* any order inside a level: wave-aggregated append, no ordering pass  */
};

/* sr_opts.liveness: the complete `eventually` check (see sr_gpu_bfs_liveness below). Every value but 0,
 * SR_LIVENESS_PROGRESS, SR_LIVENESS_WEAK and SR_LIVENESS_STRONG is read as SR_LIVENESS_COMPLETE. */
enum sr_liveness_mode {
    SR_LIVENESS_OFF = 0,
    SR_LIVENESS_COMPLETE = 1, /* no fairness: a self-loop on a state where the property does not hold refutes it */
    SR_LIVENESS_PROGRESS = 2, /* progress fairness: a successor equal to its state is no successor */
    SR_LIVENESS_WEAK = 3,     /* weak fairness per action slot (see sr_gpu_bfs_liveness_weak below). Until this
                                 value was given its meaning, 3 was one of the "other values" read as
                                 SR_LIVENESS_COMPLETE */
    SR_LIVENESS_STRONG = 4    /* strong fairness per action slot (see sr_gpu_bfs_liveness_strong below). Until
                                 this value was given its meaning, 4 was one of the "other values" read as
                                 SR_LIVENESS_COMPLETE; the values from 5 up still are */
};
/* sr_live_result.end_kind: how the witness ends (both modes). */
enum sr_live_end { SR_LIVE_END_NONE = 0, SR_LIVE_END_TERMINAL = 1, SR_LIVE_END_LOOP = 2, SR_LIVE_END_STUTTER = 3 };

/* SR_LEADS_TO has no reference counterpart: "whenever the property's trigger holds, its condition holds then
 * or later" (TLA+'s P ~> Q; always-eventually where the trigger is true). Only the complete liveness check
 * decides it (see sr_gpu_bfs_liveness_leads below); the search itself never discovers it. */
enum sr_expectation { SR_ALWAYS = 0, SR_EVENTUALLY = 1, SR_SOMETIMES = 2, SR_LEADS_TO = 3, SR_ALWAYS_STEP = 4 }; /* src/lib.rs:293-300 */
/* SR_ALWAYS_STEP has no reference counterpart either: an invariant over STEPS (TLA+'s [][A]_v), decided by the
 * step pass alone (see sr_gpu_bfs_step below); the search itself never discovers it. */

enum sr_status {
    SR_OK = 0,
    SR_ERR_ARG = -1,
    SR_ERR_HIP = -2,
    SR_ERR_CAPACITY = -3,
    SR_ERR_UNSUPPORTED = -4,
    SR_ERR_NO_DEVICE = -5,
    SR_ERR_NONDETERMINISM = -6
};

typedef struct sr_opts {
    uint32_t struct_size;        /* sizeof(sr_opts)                                              */
    int32_t device;              /* HIP device ordinal                                           */
    uint64_t target_state_count; /* 0 = None; `CheckerBuilder::target_state_count` checker.rs:164 */
    int32_t order;               /* enum sr_order                                                */
    int32_t record_visits;       /* keep every visited state (a StateRecorder visitor)           */
    uint64_t capacity_hint;      /* expected unique states; 0 = grow the visited table on demand */
    int32_t profile;             /* time every expand launch with HIP events                     */
    int32_t verbose;             /* per-level log lines on stderr                                */
    int32_t counters;            /* count visited-set probes and CAS attempts (sr_stats.probes/cas)
                                    with a counting variant of the expand kernel (slower)        */
    int32_t defer_paths;         /* partitioned search: 0 = at join, every rank gathers the states
                                    of every discovery path (collectively), so sr_gpu_bfs_discovery*
                                    work on any single rank afterwards; 1 = skip that at join and
                                    reconstruct on demand (then collective: every rank must call
                                    sr_gpu_bfs_discovery* for the same property in the same order).
                                    The reference's join reconstructs nothing either
                                    (src/checker/bfs.rs:289-298 builds paths in discoveries()). */
    int32_t symmetry;            /* 1 = canonical symmetry reduction (models with a canonical form:
                                    2pc, plugins with `canonical`): one state per orbit, order-
                                    independent counts; NOT the reference's DFS count, whose
                                    representatives are not canonical (src/checker/dfs.rs:258-283) */
    int32_t reserved0;           /* what were 4 bytes of tail padding; never read                  */
    int32_t liveness;            /* 1 = the complete `eventually` check (see sr_gpu_bfs_liveness below); 2 = the
                                    same under progress fairness, 3 = under weak fairness per action
                                    slot, 4 = under strong fairness (enum sr_liveness_mode); 0 = off,
                                    and then nothing changes. The struct grew from 56 to 64 bytes for it: a
                                    caller whose struct_size is 56 is read as liveness = 0, whatever its
                                    padding holds                                                   */
    int32_t coverage;            /* 1 = the coverage pass behind a check that explored everything (see
                                    sr_gpu_bfs_coverage below); 0 = off, and then nothing changes. What was
                                    `reserved1`: the size and every offset are unchanged, and a caller
                                    whose struct_size is 56 is read as coverage = 0                  */
    int32_t certify;             /* 1 = the certificate pass behind a one-GPU check (see sr_gpu_bfs_certificate
                                    below); 0 = off, and then nothing changes. The search launches the
                                    kernels it launches without it; the visited set is only kept until the
                                    pass has run. The struct grew from 64 to 72 bytes for it: a caller
                                    whose struct_size is 64 is read as certify = 0                   */
    int32_t reserved1;           /* tail padding made explicit; never read                           */
} sr_opts;

/* Timing/throughput counters of a finished run (sr_gpu_bfs_stats / sr_gpu_bfs_stats_sized).
 * Layout of SR_PLUGIN_ABI 4 (ABI 3 plus exchange_fallbacks and owner_key). */
typedef struct sr_stats {
    double level_loop_sec;       /* first expand launch .. last level synchronised              */
    double total_sec;            /* spawn .. done, excluding one-time device allocation          */
    double expand_kernel_ms;     /* sum of expand-kernel HIP-event durations (profile=1)         */
    uint64_t expand_launches;
    uint64_t levels;
    uint64_t table_capacity;     /* visited-set slots                                            */
    uint64_t rehashes;
    uint64_t algorithmic_bytes;  /* 8 B per successor probe + 16 B per insert +
                                    8*W B frontier write + 8*W B frontier read per state         */
    uint64_t successors;         /* == state_count - init states                                 */
    uint32_t words_per_state;
    uint32_t order_used;         /* enum sr_order actually used for the reported counts          */
    uint32_t restarts;           /* capacity restarts of this check (larger buffers / synchronous) */
    uint32_t pipelined;          /* partitioned search: 1 = levels pipelined, no host wait inside;
                                    2 = pipelined with the direct exchange (records stored into the
                                    owners' buffers through peer pointers, device flags per level) */
    uint64_t records_routed;     /* partitioned search: successor records sent between partitions (all ranks) */
    uint64_t head_levels;        /* partitioned search: levels run replicated before partitioning */
    uint64_t probes;             /* visited-set slots loaded by the expand kernels (first probe + linear steps) */
    uint64_t cas;                /* 64-bit atomicCAS claims attempted on the visited set */
    uint64_t max_displacement;   /* longest linear-probe displacement (slots past home) of any entry
                                    of the final visited set; measured with counters=1, else 0    */
    uint32_t displacement_limit; /* probe limit of the final table's slot encoding (quotient mode:
                                    2^dbits - 2; fingerprint mode: 65536)                          */
    uint32_t table_doublings;    /* quotient mode: in-check doublings after a level overflowed the
                                    probe limit (the level is finished on the larger table)       */
    uint32_t exchange_fallbacks; /* partitioned search: checks redone on the collective exchange after
                                    the direct exchange failed its per-slot sequence tag / checksum
                                    or a peer's flag timed out (the result is then still exact)    */
    uint32_t owner_key;          /* partitioned search: 1 = states are owned by the model's owner key
                                    (a projection most actions keep), 0 = by fingerprint          */
    uint32_t balanced_levels;    /* FAST order: expand launches that cut their level into equal
                                    workgroup shares from the real frontier size (SR_BALANCE=0: 0) */
    uint32_t table_encoding;     /* the final visited set's slot encoding and the duplicate filter the
                                    check ran with: bits 0-7 remainder bits (0: fingerprint mode),
                                    bit 8 4-byte slots, bits 16-23 log2 of the filter's entries (0: no
                                    filter), bit 24 compact (4-byte) filter entries (this field was
                                    reserved0 and always 0 before)                                 */
    uint32_t root_path;          /* how the init states entered the check (enum sr_root_path)      */
    uint32_t reserved1;
} sr_stats;

/* sr_stats.root_path: the code path that put the init states into the visited set and level 0. */
enum sr_root_path {
    SR_ROOTS_INLINE = 1,   /* one launch, the states in the kernel arguments (at most 32 words of them);
                              simulation: the walks read them from the kernel arguments            */
    SR_ROOTS_FUSED = 2,    /* a host copy, then one workgroup (more than 32 words, at most 256 states) */
    SR_ROOTS_LAUNCHES = 3, /* a host copy, then insert, evaluate and publish launches (more than 256) */
    SR_ROOTS_HEAD = 4,     /* partitioned search: into the replicated head                         */
    SR_ROOTS_PARTS = 5,    /* partitioned search: each partition takes the states it owns          */
    SR_ROOTS_BUFFER = 6    /* simulation: the walks read them from device memory (more than 32 words) */
};

typedef struct sr_bfs sr_bfs;

void sr_opts_init(sr_opts* opts);
/* The same for a caller whose sr_opts mirror has `size` bytes (a binding written against an older
 * header): writes at most `size` bytes and sets struct_size to what it wrote. Bindings in other
 * languages should call this with their own struct size rather than sr_opts_init. */
void sr_opts_init_sized(sr_opts* opts, uint32_t size);
const char* sr_last_error(void);
int sr_device_count(void);

/* Spawns the checker; returns NULL on error (see sr_last_error). Non-blocking. */
sr_bfs* sr_gpu_bfs_spawn(int32_t model_id, const int64_t* params, int32_t nparams, const sr_opts* opts);
int32_t sr_gpu_bfs_join(sr_bfs* bfs);
int32_t sr_gpu_bfs_is_done(const sr_bfs* bfs);
/* 1 while the driver thread is still searching (for `report`'s polling loop, src/checker.rs:223). */
int32_t sr_gpu_bfs_is_running(const sr_bfs* bfs);
uint64_t sr_gpu_bfs_state_count(const sr_bfs* bfs);
uint64_t sr_gpu_bfs_unique_state_count(const sr_bfs* bfs);
uint32_t sr_gpu_bfs_max_depth(const sr_bfs* bfs);
int32_t sr_gpu_bfs_stats(const sr_bfs* bfs, sr_stats* out);
/* The same for a caller whose sr_stats mirror has `size` bytes (a binding written against another
 * header): copies at most `size` bytes; returns the engine's sizeof(sr_stats). */
int32_t sr_gpu_bfs_stats_sized(const sr_bfs* bfs, sr_stats* out, uint32_t size);
/* profile=1: HIP-event duration (ms) of every expand launch in launch order and the frontier size
 * it expanded (0 if unknown); returns the number of launches (FAST pipelined order: launch i
 * expands level i, a last launch past the end expands nothing). */
int64_t sr_gpu_bfs_launch_profile(const sr_bfs* bfs, double* kernel_ms, uint64_t* frontier, int64_t cap);
/* Visited-set probes and CAS claims of every expand launch of the pipelined FAST loop, in launch
 * order (sr_opts.counters = 1; zeros otherwise). Returns the number of launches. */
int64_t sr_gpu_bfs_launch_counters(const sr_bfs* bfs, uint64_t* probes, uint64_t* cas, int64_t cap);

int32_t sr_gpu_bfs_property_count(const sr_bfs* bfs);
/* Copies the property name (NUL-terminated) and its expectation; returns the name length. */
int32_t sr_gpu_bfs_property(const sr_bfs* bfs, int32_t prop, char* name, int32_t cap, int32_t* expectation);

/* Discovery of property `prop`: writes the fingerprint chain init..discovered state (the
 * reference's `reconstruct_path` input) and returns its length; 0 = no discovery. */
int32_t sr_gpu_bfs_discovery(const sr_bfs* bfs, int32_t prop, uint64_t* fp_chain, uint32_t cap);
/* Replays that chain on the host model (`Path::from_fingerprints`): canonical action ids
 * (len = chain-1) and states (chain * describe_width int64s). Returns the number of actions,
 * -1 if no discovery, or a negative SR_ERR_*. */
int32_t sr_gpu_bfs_discovery_path(const sr_bfs* bfs, int32_t prop, int64_t* action_ids, int32_t cap_actions,
                                  int64_t* states, int64_t cap_states);
int32_t sr_gpu_bfs_describe_width(const sr_bfs* bfs);
/* Reference `Debug` text of a canonical action id (e.g. "RmPrepare(3)"). */
int32_t sr_gpu_bfs_action_name(const sr_bfs* bfs, int64_t action_id, char* buf, int32_t cap);
/* Upper bound (exclusive) on canonical action ids of the model, for name lookups. */
int64_t sr_gpu_bfs_action_id_bound(const sr_bfs* bfs);
/* Number of init states (`Model::init_states`, src/lib.rs:163). */
int32_t sr_gpu_bfs_init_count(const sr_bfs* bfs);
/* `Path::from_actions` (src/checker/path.rs:90-112) from init state `init_index` on the host copy
 * of the model: writes the states (describe_width int64s each) and, per property, whether its
 * CONDITION holds on the last state. Returns the number of actions applied, or -1 if an action is
 * not enabled along the way (the reference returns None). */
int32_t sr_gpu_bfs_replay(const sr_bfs* bfs, int32_t init_index, const int64_t* action_ids, int32_t n_actions,
                          int64_t* states, int64_t cap_states, int32_t* conditions, int32_t cap_conditions);
/* `Path::from_actions` as above, reporting each property's condition on EVERY state of the path
 * (conditions[i * property_count + p], i = 0..n) and whether the last state is terminal (its
 * `actions()` list is empty): what `assert_discovery` needs for an `eventually` property
 * (src/checker.rs:306-323). Returns n, or -1 if an action is not enabled along the way. */
int32_t sr_gpu_bfs_replay_trace(const sr_bfs* bfs, int32_t init_index, const int64_t* action_ids, int32_t n_actions,
                                int32_t* conditions, int64_t cap, int32_t* terminal);
/* Explorer's `states` route (src/checker/explorer.rs:159-240), host-only: n == 0 lists the init
 * states (action -1); otherwise the state reached by the fingerprint path (`Path::final_state`,
 * src/checker/path.rs:115-136) and, per action its `actions()` lists (in order), the canonical
 * action id, whether `next_state` is Some (has_state), the next state's fingerprint and its
 * description (describe_width int64s per view). Returns the number of views (at most cap are
 * written), or -1 if no state follows the fingerprints. */
int32_t sr_gpu_bfs_explore(const sr_bfs* bfs, const uint64_t* fingerprints, int32_t n, int64_t* action_ids,
                           int32_t* has_state, uint64_t* fingerprints_out, int64_t* states, int32_t cap);
/* Visited states in visit order (record_visits=1), describe_width int64s each; returns count*width. */
int64_t sr_gpu_bfs_visits(const sr_bfs* bfs, int64_t* out, int64_t cap);
/* The visitor's paths (`CheckerVisitor::visit` gets `Path::from_fingerprints` of every popped
 * state, src/checker/bfs.rs:187-189, src/checker/visitor.rs:19-66): per visit, in the order of
 * sr_gpu_bfs_visits, the visit index of its BFS-tree parent and the canonical id of the first
 * action leading from that parent to it (-1 and -1 for init states). Returns the visit count,
 * or SR_ERR_UNSUPPORTED when the check kept no visit record (record_visits=0). The partitioned
 * search gathers every rank's records at join, so its tree is global on every rank. */
int64_t sr_gpu_bfs_visit_tree(const sr_bfs* bfs, int64_t* parent, int64_t* action, int64_t cap);
void sr_gpu_bfs_free(sr_bfs* bfs);

/* ---- The complete `eventually` check (sr_opts.liveness = 1; stateright_amd/csrc/live.hpp has the
 * definition, for host and device from one source) ----
 * The search refutes an `eventually` property only at a terminal state reached with the property's
 * bit still set, and the bits are not part of the visited key, so it reports "holds" for a state
 * that is reached first along a path on which the property held and later along one on which it did
 * not, and for a path round a cycle on which it never holds (the reference's FIXMEs,
 * src/checker/bfs.rs:239-256, pinned in src/checker.rs:400-413). With liveness = 1 a search that
 * ended having explored everything is followed, per `eventually` property p still without a
 * discovery, by a backward fixpoint over the reachable set: N_p = the reachable states where p's
 * condition does not hold; F_p = the greatest subset of N_p in which every state is terminal (no
 * action yields a next state within the boundary) or has a successor in F_p. p has a counterexample
 * iff an init state is in F_p, and then the discovery of p is the deterministic witness: from the
 * init state of lowest index in F_p, always through the lowest action slot whose next state is in
 * F_p, to a terminal state (loop_start -1) or to the first state equal to an earlier one of the path
 * (a lasso: the path's LAST state EQUALS its state at index loop_start; the two are compared word
 * for word before the path is returned). sr_gpu_bfs_discovery / _discovery_path serve it like any
 * other discovery. After the pass, no discovery of an `eventually` property means it holds on every
 * maximal path. A property the search itself discovered keeps that discovery.
 * Not covered: no fairness is assumed, so any self-loop on a state where p does not hold refutes p;
 * the witness is not the shortest counterexample; one GPU and registered models only. Refused at
 * spawn with SR_ERR_UNSUPPORTED: target_state_count (a partial set makes the fixpoint unsound), the
 * partitioned spawns, symmetry, plugins, a capacity_hint beyond 2^32 - 1 states (a check that reaches
 * more fails at the pass). A successor the visited set does not hold fails the check with
 * SR_ERR_NONDETERMINISM.
 * PROGRESS FAIRNESS (liveness = SR_LIVENESS_PROGRESS = 2, off by default): the same rule over
 * succ'(s) = succ(s) \ {s}: a successor whose words all equal those of s is no successor, and a state
 * is a sink if it is terminal or a STUTTER END (it has successors and every one is the state
 * itself). F_p' is the greatest subset of N_p in which every state is such a sink or has a successor
 * other than itself in F_p'; the witness steps over succ' only and ends at a terminal state, at a
 * stutter end (end_kind 3, loop_start -1) or at the first repeated state, so a closed loop has at
 * least two distinct states. No discovery then means: the property holds on every maximal path that
 * does not stay forever in one state that has a successor other than itself. This is NOT per-action
 * weak fairness: a cycle through two or more distinct states still refutes the property, and that is
 * not repaired in this mode (SR_LIVENESS_WEAK below is). The refusals above apply unchanged; the simulation checker's loop detection
 * (sr_sim_opts.loops) is not affected: there a self-loop still closes a lasso. */
typedef struct sr_live_result {
    int32_t ran;            /* 1 = the pass ran for this property                                  */
    int32_t init_index;     /* the init state (order of init_states) the witness starts at; -1 = no
                               init state is in F_p: the property holds                            */
    uint64_t not_p_states;  /* |N_p|                                                               */
    uint64_t surviving;     /* |F_p|                                                               */
    uint64_t examined;      /* worklist entries examined over all rounds                           */
    uint32_t rounds;        /* rounds until one removed nothing (an implementation detail: states
                               are removed in place, so it depends on the order; never compare it) */
    uint32_t end_kind;      /* enum sr_live_end: 0 no witness, 1 it ends at a terminal state, 2 it closes a
                               loop, 3 (progress fairness only) it ends at a stutter end. What was
                               `reserved0`: the size and every offset are unchanged                 */
    int64_t witness_len;    /* steps of the witness; -1 without one                                */
    int64_t loop_start;     /* index of the path's state that its last state repeats; -1 = none, or
                               the witness ends at a terminal state                                */
    double pass_ms;         /* wall time of the pass for this property                             */
} sr_live_result;
/* The pass' outcome for property `prop` of a joined check (ran = 0: liveness off, neither an `eventually`
 * nor a leads-to property, discovered by the search itself, or the search did not explore everything). */
int32_t sr_gpu_bfs_liveness(const sr_bfs* bfs, int32_t prop, sr_live_result* out);
/* Host-only (no device needed): a host search of a registered model over at most max_states states
 * (SR_ERR_CAPACITY beyond), then the fixpoint and the witness for its `eventually` property `prop`.
 * Writes the witness' canonical action ids (at most cap). Returns the model's unique state count,
 * or a negative SR_ERR_*. */
int64_t sr_liveness_host(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int64_t max_states,
                         sr_live_result* out, int64_t* action_ids, int32_t cap);
/* The same with the mode as an argument: fairness 0 = none (sr_liveness_host is this call), 1 = progress
 * fairness (SR_ERR_ARG for any other value). */
int64_t sr_liveness_host_fair(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int32_t fairness,
                              int64_t max_states, sr_live_result* out, int64_t* action_ids, int32_t cap);
/* Host-only: the sink kind of the state reached by the canonical action ids from init state `init` of
 * a joined check's model: -1 the actions cannot be replayed, 0 the state has a successor other than
 * itself, 1 it is terminal, 3 it is a stutter end (what `assert_discovery` asks in the progress mode). */
int32_t sr_gpu_bfs_sink_kind(const sr_bfs* bfs, int32_t init, const int64_t* action_ids, int32_t n);

/* ---- WEAK FAIRNESS (liveness = SR_LIVENESS_WEAK = 3, off by default; live.hpp and DESIGN.md section 12
 * have the definition) ----
 * An action SLOT is a fairness class, for the models that say their slots are actions (DGraph, LiveGraph,
 * 2pc and 2pc-live, SpinLock); every other model is refused at spawn with SR_ERR_UNSUPPORTED, as is
 * everything the other modes refuse. me(s, a): slot a is enabled at s, yields a state, and that state
 * differs from s. Over F_p' (progress fairness above) and its edges between distinct states, a strongly
 * connected component of two or more states is FAIR iff for every slot a some member has not me(., a), or
 * some member's a-step stays inside the component. goal = the sinks of F_p' (terminal states and stutter
 * ends) and the members of fair components; FairF = the states of F_p' from which goal is reachable. The
 * property has a counterexample iff an init state is in FairF; no discovery means it holds on every maximal
 * run that is weakly fair to every slot (which subsumes progress fairness). The witness is deterministic:
 * from the init state of lowest index in FairF along the lowest slot that lowers the distance to goal; at
 * a sink it ends (end_kind 1 or 3, loop_start -1); otherwise a closed walk inside the fair component
 * follows, which for every slot in order either passes a state where the slot is not moving-enabled or
 * takes it (end_kind 2; the path's last state equals its state at loop_start = stem_len; the loop may pass
 * a state more than once). sr_live_result keeps its meanings: not_p_states |N_p|, surviving |F_p'|,
 * witness_len = stem_len + loop_len. Not strong fairness: a slot that is disabled again and again on a
 * loop is not protected. */
typedef struct sr_live_weak {
    int32_t ran;              /* 1 = the pass ran for this property in this mode                      */
    int32_t reserved0;
    uint64_t cyclic_states;   /* F_p' without its sinks, trimmed to the states with a successor in it  */
    uint64_t components;      /* strongly connected components of two or more states                  */
    uint64_t fair_components;
    uint64_t goal_states;     /* sinks of F_p' and members of fair components                         */
    uint64_t fair_states;     /* |FairF|                                                              */
    int64_t stem_len;         /* steps from the init state to the sink or into the fair component; -1 */
    int64_t loop_len;         /* steps of the closed walk; 0 where the witness ends at a sink; -1      */
    uint32_t scc_rounds;      /* implementation details (kernel rounds of the component search, of the  */
    uint32_t reach_rounds;    /* rank fixpoints, and rank fixpoints run for the loop): never compare    */
    uint32_t segments;        /* them                                                                   */
    uint32_t reserved1;
    double pass_ms;           /* wall time of what this mode adds to the pass for this property        */
} sr_live_weak;
/* The weak-fairness figures for property `prop` of a joined check (ran = 0: the check ran in another mode,
 * or sr_gpu_bfs_liveness would say ran = 0). */
int32_t sr_gpu_bfs_liveness_weak(const sr_bfs* bfs, int32_t prop, sr_live_weak* out);
/* Host-only (no device needed): sr_liveness_host under weak fairness, by other algorithms than the
 * device's (Tarjan's components, breadth-first ranks over predecessor lists). SR_ERR_UNSUPPORTED for a
 * model whose slots are not fairness classes. */
int64_t sr_liveness_host_weak(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int64_t max_states,
                              sr_live_result* out, sr_live_weak* weak, int64_t* action_ids, int32_t cap);
/* Host-only: whether the loop of a lasso is weakly fair. The canonical action ids are replayed from init
 * state `init` of a joined check's model; the loop is the states from index loop_start to the last, which
 * must equal the state at loop_start. 1: every slot is not moving-enabled at some state of the loop or
 * taken by one of its steps; 0: it is not, or the loop is not closed or has no step; -1: the actions
 * cannot be replayed, or the model's slots are not fairness classes. */
int32_t sr_gpu_bfs_loop_fair(const sr_bfs* bfs, int32_t init, const int64_t* action_ids, int32_t n, int32_t loop_start);

/* ---- STRONG FAIRNESS (liveness = SR_LIVENESS_STRONG = 4, off by default; live.hpp and DESIGN.md section 12
 * have the definition) ----
 * Slots, me(s, a), F_p', its sinks and its graph G' are those of the weak mode, and the same models take it
 * (every other is refused at spawn with SR_ERR_UNSUPPORTED, as is everything the other modes refuse). A set S
 * of two or more states of F_p', strongly connected in G'[S], is STRONGLY FAIR iff for every slot a no member
 * has me(., a), or some member has me(., a) and its a-step stays in S. Such a set may lie inside a component
 * that is not fair (a larger set may enable a slot the smaller never enables), so the components are
 * DECOMPOSED: for a component C of G'[X], bad(C) is the set of slots that are moving-enabled somewhere in C
 * and whose steps all leave C; with bad(C) empty, C is a FAIR NODE; otherwise the components of C without the
 * states that enable a bad slot are decomposed in the same way, starting from X = F_p' at depth 1. goal = the
 * sinks of F_p' and the members of fair nodes; FairF = the states of F_p' from which goal is reachable. The
 * property has a counterexample iff an init state is in FairF; no discovery means it holds on every maximal
 * run that is strongly fair to every slot (a slot moving-enabled again and again is taken again and again),
 * which subsumes weak fairness. The witness is deterministic: the weak mode's stem; at a sink it ends
 * (end_kind 1 or 3, loop_start -1); otherwise a closed walk inside the fair node follows, which takes, for the
 * slots in order, every slot that some member moves on and no step of the loop so far took, from the nearest
 * member whose step stays inside, and then goes home (end_kind 2, loop_start = stem_len). It is not the
 * shortest counterexample. One GPU, registered models only; levels and rounds are reported, not bounded. */
typedef struct sr_live_strong {
    int32_t ran;              /* 1 = the pass ran for this property in this mode                      */
    uint32_t levels;          /* depth of the decomposition tree; 0 without a component               */
    uint64_t cyclic_states;   /* F_p' without its sinks, trimmed to the states with a successor in it  */
    uint64_t components;      /* nodes of the tree: components of two or more states, at every depth   */
    uint64_t fair_components; /* fair nodes (pairwise disjoint)                                        */
    uint64_t goal_states;     /* sinks of F_p' and members of fair nodes                               */
    uint64_t fair_states;     /* |FairF|                                                              */
    int64_t stem_len;         /* steps from the init state to the sink or into the fair node; -1       */
    int64_t loop_len;         /* steps of the closed walk; 0 where the witness ends at a sink; -1      */
    uint32_t scc_rounds;      /* implementation details (kernel rounds of the component searches, of   */
    uint32_t reach_rounds;    /* the rank fixpoints, and rank fixpoints run for the loop): never        */
    uint32_t segments;        /* compare them                                                           */
    uint32_t reserved1;
    double pass_ms;           /* wall time of what this mode adds to the pass for this property        */
} sr_live_strong;
/* The strong-fairness figures for property `prop` of a joined check (ran = 0: the check ran in another mode,
 * or sr_gpu_bfs_liveness would say ran = 0). */
int32_t sr_gpu_bfs_liveness_strong(const sr_bfs* bfs, int32_t prop, sr_live_strong* out);
/* Host-only (no device needed): sr_liveness_host under strong fairness, by other algorithms than the
 * device's (the decomposition tree by recursion with Tarjan's components, breadth-first ranks over
 * predecessor lists). SR_ERR_UNSUPPORTED for a model whose slots are not fairness classes. */
int64_t sr_liveness_host_strong(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int64_t max_states,
                                sr_live_result* out, sr_live_strong* strong, int64_t* action_ids, int32_t cap);
/* Host-only: whether the loop of a lasso is strongly fair; replayed as sr_gpu_bfs_loop_fair replays it. 1:
 * every slot that is moving-enabled at some state of the loop is taken by one of its steps; 0: it is not, or
 * the loop is not closed or has no step; -1: the actions cannot be replayed, or the model's slots are not
 * fairness classes. */
int32_t sr_gpu_bfs_loop_strongly_fair(const sr_bfs* bfs, int32_t init, const int64_t* action_ids, int32_t n,
                                      int32_t loop_start);
/* ---- LEADS-TO properties (expectation SR_LEADS_TO; live.hpp and DESIGN.md section 14 have the definition) ----
 * A leads-to property p has a TRIGGER P and a TARGET condition Q (the property's condition). In every mode of
 * the complete check, X_Q is the mode's set for Q exactly as for an `eventually` property with that condition:
 * F_p (no fairness), F_p' (progress) or FairF (weak, strong): the reachable states from which a (fair) maximal
 * run exists on which Q never holds. p has a counterexample iff some REACHABLE state where P holds is in X_Q.
 * The seed is the violating state of lowest depth (breadth-first distance from the init states), among those
 * the lowest compared word by word from word 0, unsigned. The witness is the search's own tree path from an
 * init state to the seed (its length is the seed's depth; Q may hold on it), followed by the mode's witness
 * started at the seed. sr_live_result keeps its meanings, over the whole path: witness_len counts all steps,
 * init_index is the init state the prefix starts at (the lowest index of an equal init state), loop_start is
 * an index into the whole path and never below trigger_index; sr_live_weak / sr_live_strong stem_len counts
 * from the seed, so loop_start = trigger_index + stem_len. With liveness off the property is not checked, and
 * the search stops as if it were absent; with liveness on an undiscovered leads-to property makes the search
 * explore everything. One seed only; the witness is not the shortest beyond its prefix. */
typedef struct sr_live_leads {
    int32_t ran;            /* 1 = the pass ran for this property and it is a leads-to property            */
    int32_t reserved0;
    uint64_t triggered;     /* reachable states where the trigger holds                                    */
    uint64_t pending;       /* ... where the trigger holds and the target condition does not               */
    uint64_t violating;     /* ... where the trigger holds and that are in X_Q (each state counted once,
                               whatever number of runs from it avoid Q)                                   */
    int64_t trigger_index;  /* index of the seed on the witness = length of the prefix; -1 without one     */
    int64_t trigger_depth;  /* the seed's depth; equals trigger_index; -1 without a witness                */
    double seed_ms;         /* wall time of the seed stage (counts, seed, tie-break)                       */
} sr_live_leads;
/* The leads-to figures for property `prop` of a joined check (ran = 0: not a leads-to property, or
 * sr_gpu_bfs_liveness would say ran = 0). */
int32_t sr_gpu_bfs_liveness_leads(const sr_bfs* bfs, int32_t prop, sr_live_leads* out);
/* Host-only: the trigger of the leads-to property `prop` on every state of the path that the canonical action
 * ids describe from init state `init` of a joined check's model (what `assert_discovery` asks for a leads-to
 * property): writes n + 1 entries (0 / 1) and returns n + 1; -1: the actions cannot be replayed, `prop` is no
 * leads-to property, or cap < n + 1. */
int32_t sr_gpu_bfs_replay_triggers(const sr_bfs* bfs, int32_t init, const int64_t* action_ids, int32_t n, int32_t prop,
                                   int32_t* out, int32_t cap);
/* Host-only (no device needed): the leads-to check of property `prop` of a registered model in the mode
 * `fairness` (0 none, 1 progress, 2 weak, 3 strong), built from the host forms above with the seed rule above;
 * the prefix is the tree path of the reference's FIFO order. Writes the whole witness' canonical action ids
 * (at most cap). Returns the model's unique state count, or a negative SR_ERR_*. */
int64_t sr_liveness_host_leads(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int32_t fairness,
                               int64_t max_states, sr_live_result* out, sr_live_leads* leads, int64_t* action_ids, int32_t cap);
/* ---- The coverage pass (sr_opts.coverage = 1, off by default; stateright_amd/csrc/cover.hpp has the
 * definition, for host and device from one source) ----
 * "No discovery over N states" is only worth something if the model did what its author believes: an
 * action that is never enabled, or is enabled but always cut by the boundary, makes every `always`
 * property hold vacuously, and so does a property whose condition holds nowhere or everywhere. With
 * coverage = 1 a one-GPU search that ended having explored everything is followed by one more expansion
 * of every reachable state, on the GPU and without the visited set, that counts: per ACTION CLASS c
 * (the class of slot a at state s is a itself, or what the model's optional `cover_class` hook says:
 * include/stateright_gpu_model.hpp) enabled[c] (slots of enabled(s)), taken[c] (those for which apply
 * yields a state within the boundary) and moved[c] (those whose state differs from s); per state, with
 * deg its taken and mdeg its moved slots, terminal (deg = 0), stutter_ends (deg > 0, mdeg = 0),
 * out_degree[min(deg, 63)] and max_out_degree; per property, the states where its CONDITION holds. Every
 * distinct reachable state counts once (a repeated init state too). The search itself is unchanged: the
 * pass reads the arena behind it, and with the option off no kernel, count or allocation differs.
 * ran = 0: the option is off or the search did not explore everything (it stopped with every property
 * discovered). Refused at spawn with SR_ERR_UNSUPPORTED: the partitioned spawns, symmetry (the counts
 * would be over orbit representatives), target_state_count, a model of more than 1024 classes. Plugin
 * models take it; the simulation checker ignores it. What the figures do not say: which action FOUND a
 * state first (that depends on the visit order), anything per depth, anything about simulation traces. */
typedef struct sr_coverage {
    uint32_t struct_size;     /* sizeof this struct in the caller's build (set before the call)          */
    int32_t ran;              /* 1 = the pass ran; with 0 every field below is 0                          */
    uint64_t states;          /* |R|: equals unique_state_count                                           */
    uint64_t terminal;        /* states without a taken slot                                              */
    uint64_t stutter_ends;    /* states with taken slots, every one of them the state itself              */
    uint32_t max_out_degree;  /* the most taken slots of one state (not clamped)                          */
    int32_t classes;          /* action classes, at most 1024                                             */
    int32_t nprops;           /* properties                                                               */
    int32_t reserved0;
    double pass_ms;           /* wall time of the pass                                                    */
    uint64_t out_degree[64];  /* states by taken slots; the last bucket holds 63 and more                 */
} sr_coverage;
/* Fills *out (at most out->struct_size bytes) for a joined check. SR_ERR_ARG for a handle that still runs. */
int32_t sr_gpu_bfs_coverage(const sr_bfs* bfs, sr_coverage* out);
/* The per-class counts (each array may be NULL; at most cap entries are written). Returns the number of
 * classes, 0 if the pass did not run. */
int32_t sr_gpu_bfs_coverage_classes(const sr_bfs* bfs, uint64_t* enabled, uint64_t* taken, uint64_t* moved, int32_t cap);
/* Per property, the states where its condition holds. Returns the number of properties, 0 if the pass did
 * not run. */
int32_t sr_gpu_bfs_coverage_props(const sr_bfs* bfs, uint64_t* holds, int32_t cap);
/* Copies the name of class c (NUL-terminated); returns its length, or SR_ERR_ARG. */
int32_t sr_gpu_bfs_coverage_class_name(const sr_bfs* bfs, int32_t c, char* name, int32_t cap);
/* Host-only (no device needed): the same figures by a host search of a registered model over at most
 * max_states states (SR_ERR_CAPACITY beyond) and the same per-state rule. enabled, taken, moved take at most
 * class_cap entries and holds at most prop_cap (each may be NULL); names (may be NULL) receives the class
 * names, each followed by a newline, cut at names_cap - 1 bytes and NUL-terminated. Returns the model's
 * unique state count, or a negative SR_ERR_*. */
int64_t sr_coverage_host(int32_t model_id, const int64_t* params, int32_t nparams, int64_t max_states, sr_coverage* out,
                         uint64_t* enabled, uint64_t* taken, uint64_t* moved, int32_t class_cap, uint64_t* holds,
                         int32_t prop_cap, char* names, int32_t names_cap);

/* ---- STEP properties (expectation SR_ALWAYS_STEP; stateright_amd/csrc/step.hpp has the definition, for host
 * and device from one source) ----
 * A step property is an invariant over the steps of the model: the model's `step_holds(p, s, a, t)` hook says
 * whether the step from s through action slot a to t is allowed. An EDGE is a pair (s, a) with s a distinct
 * reachable state, a in enabled(s) and apply(s, a) yielding a state within the boundary (the coverage pass'
 * "taken"; a step back to s itself is an edge like any other). With no option at all, a one-GPU search that
 * ended having explored everything is followed by one more expansion of every reachable state, on the GPU and
 * without the visited set, that counts per step property: edges (the same for every property), violations (the
 * edges where the hook is false) and sources (the states with a violating edge). The property has a
 * counterexample iff violations > 0. The SEED is the violating edge whose source has the lowest depth, then the
 * source lowest compared word by word from word 0, unsigned, then the lowest slot; the witness is the search's
 * own tree path from an init state to the seed's source followed by the seed's action: step_index + 1 actions,
 * the last state the seed's successor. It is the property's discovery (sr_gpu_bfs_discovery*). An undiscovered
 * step property makes the search explore everything. ran = 0 (the property is NOT CHECKED, never refused at
 * spawn, and the search stops as if it were absent): the partitioned spawns, symmetry, target_state_count, the
 * simulation checker, a search that stopped early. One seed only; no early exit. */
typedef struct sr_step_result {
    uint32_t struct_size;  /* sizeof this struct in the caller's build (set before the call)               */
    int32_t ran;           /* 1 = the pass ran and `prop` is a step property; with 0 the counts are 0       */
    uint64_t edges;        /* edges of the reachable graph                                                  */
    uint64_t violations;   /* edges on which the property does not hold                                     */
    uint64_t sources;      /* states with at least one such edge                                            */
    int64_t step_index;    /* index of the violating step on the witness = the seed's depth; -1 without one */
    int64_t step_action;   /* the canonical id of the seed's action; -1 without a witness                   */
    int32_t init_index;    /* the init state the witness starts at (the lowest index of an equal one); -1   */
    int32_t reserved0;
    int64_t witness_len;   /* actions of the witness = step_index + 1; -1 without one                       */
    double scan_ms;        /* wall time of the counting launch and its read-back (shared by the properties) */
    double min_ms;         /* wall time of this property's seed tie-break and witness                       */
} sr_step_result;
/* Fills *out (at most out->struct_size bytes) for property `prop` of a joined check. SR_ERR_ARG for a handle
 * that still runs or a `prop` that is no property. */
int32_t sr_gpu_bfs_step(const sr_bfs* bfs, int32_t prop, sr_step_result* out);
/* Host-only: whether the LAST step of the path that the canonical action ids describe from init state `init`
 * of a joined check's model holds for the step property `prop` (what `assert_discovery` asks): 1 it holds, 0 it
 * violates it; -1: the actions cannot be replayed, n < 1, or `prop` is no step property. */
int32_t sr_gpu_bfs_replay_step(const sr_bfs* bfs, int32_t init, const int64_t* action_ids, int32_t n, int32_t prop);
/* Host-only (no device needed): the same rule by a host search of a registered model in the reference's FIFO
 * order over at most max_states states (SR_ERR_CAPACITY beyond); the witness follows that search's tree. Writes
 * the witness' canonical action ids (at most cap). Returns the model's unique state count, or a negative
 * SR_ERR_*. */
int64_t sr_step_host(int32_t model_id, const int64_t* params, int32_t nparams, int32_t prop, int64_t max_states,
                     sr_step_result* out, int64_t* action_ids, int32_t cap);

/* Host-only (no device needed): the reachable graph of a registered model, by a host search over at
 * most max_states states (SR_ERR_CAPACITY beyond), states numbered in the order the search finds
 * them. The dump is int64s: [states, init states, properties, the init states' numbers..., then per
 * state in number order: a bit mask of the properties whose CONDITION holds there, its successor
 * count, and per successor within the boundary, in `actions()` order, (canonical action id, number)].
 * Writes at most cap of them; returns the length of the whole dump, or a negative SR_ERR_*. What the
 * tests of the complete `eventually` check run their own fixpoint over. */
int64_t sr_host_graph(int32_t model_id, const int64_t* params, int32_t nparams, int64_t max_states, int64_t* out,
                      int64_t cap);

/* ---- Random-walk simulation checker (the counterpart of the simulation checker Stateright gained
 * after 0.28; stateright_amd/csrc/sim.hpp defines the walk, for host and device from one source) ----
 * `walks` independent random traces run from the init states, one GPU lane per trace; the properties
 * are evaluated on every state of a trace and NO visited set is kept, so a model whose reachable set
 * fits no card still gets discoveries. What it does not prove: a run WITHOUT a discovery proves
 * nothing (sr_gpu_bfs_is_done is 1 only when every property was discovered).
 *
 * Determinism: trace w is a pure function of (model, seed, w, max_depth, loops): a counter-based generator
 * r(seed, w, t, k) (two rounds of murmur3's fmix64 over the seed, the trace index, the step t and
 * the attempt k) draws the init state and, per step, one of the enabled action slots; a slot whose
 * next state is None or outside the boundary is cleared and another is drawn; a state where none is
 * left is terminal. A trace ends there (reason 1), at max_depth steps (2) or at a state past its
 * model's encoding (3, the check then fails with SR_ERR_UNSUPPORTED as a BFS check does). The
 * traces run in batches of consecutive indices and the check stops after the first whole batch at
 * whose end every property is discovered, state_count >= target_state_count, or `walks` traces
 * have run: a check is a deterministic function of (model, seed, walks, max_depth, batch size).
 * Per property the discovery is the hit of the fewest steps, ties to the lowest trace index; an
 * `eventually` property is hit only at a terminal state of a trace on which it never held.
 *
 * Loop detection (sr_sim_opts.loops = 1; off by default, and with it off nothing changes). A trace
 * that returns to a state it has visited is a lasso, a prefix followed by a cycle that can repeat
 * forever, so an `eventually` property that held nowhere on it is refuted without a terminal state
 * (no fairness assumption, as the reference defines `eventually`). A trace keeps the fingerprints of
 * its last 8 states and one checkpoint (taken at step 0 and at every power of two); at a state
 * whose fingerprint equals one of them it ends with reason 4, its loop start being the index of that
 * earlier state, and every `eventually` property that never held on it is hit there. Cycles of at
 * most 8 states are found at their first closure; longer ones once the trace returns to a
 * checkpoint. The trace with loops on is the trace with loops off, cut at its first detection
 * (stateright_amd/csrc/sim.hpp has the full rule). The discovery path of such a hit is a lasso: its
 * LAST state EQUALS its state at index loop start (both sides compare 64-bit fingerprints to end a
 * trace, but a path is returned only after the two states were compared in full; a collision fails
 * the call with SR_ERR_NONDETERMINISM and a message that says so).
 *
 * Distinct-state count (sr_sim_opts.unique = 1; off by default, and with it off nothing changes: no
 * kernel, count, record, hit or allocation). For a check that ran the traces 0 .. n-1,
 *   U = { fingerprint(s_t) : 0 <= w < n, 0 <= t <= steps(w) }:
 * every state a trace visits, its init state and its last state included, exactly the states
 * state_count counts. Every visit inserts the state's 64-bit fingerprint into a table in device
 * memory that all traces share and that lives across the batches of the check; unique_state_count is
 * then |U|, sr_gpu_sim_unique_fingerprints returns U and sr_gpu_sim_batch_new how many fingerprints
 * each batch added. The mode feeds nothing back: trace w, its record, its hits and the check's stop
 * point are the same with it on or off. U is a union, so |U|, the set and the per-batch counts are
 * functions of (model, seed, traces run, max_depth, loops, batch size) and of nothing else (not of
 * the kernel's form, the grid or the order of launches). Fingerprints are compared, not states:
 * exact for models whose state is one packed word (their fingerprint is a bijection), a 64-bit hash
 * for wider states, where n distinct states lose one to a collision with probability ~n^2 / 2^65.
 * What it is: a measure of how much ground the traces covered and of whether more traces still
 * reach anything new (the per-batch counts decay as coverage saturates). What it is not: a proof.
 * States no trace reached are not in it, |U| below the reachable count says nothing about the rest,
 * and a run stopped by stale_batches has still proved nothing: sr_gpu_bfs_is_done keeps meaning
 * "every property discovered". The table has the smallest power of two >= 2 * unique_capacity slots
 * of 8 bytes (open addressing, at most min(slots, 1024) probes per insert). An insert whose probes
 * run out is dropped and sets `overflow`: |U| is then a lower bound (with at most 1024 slots the
 * table is then full and |U| equals its slots). Without an overflow the count and the set are
 * exact up to fingerprint collisions. The table is allocated when the check starts and released
 * when it ends; U leaves the device compacted, |U| * 8 bytes of host memory.
 *
 * Every sr_gpu_bfs_* accessor works on the handle. unique_state_count is SET EQUAL to state_count
 * (states visited, repeats included: there is no visited set) unless sr_sim_opts.unique is set (then
 * it is |U| above), max_depth is the longest trace in
 * steps, sr_stats.levels the number of batches, expand_launches the launches and successors =
 * state_count - traces started; visits are empty and the visit tree is unsupported. Registered
 * models only (no plugins, no partitions, no symmetry reduction). */
typedef struct sr_sim_opts {
    uint32_t struct_size;        /* sizeof this struct in the caller's build                      */
    int32_t device;              /* HIP device ordinal                                           */
    uint64_t seed;
    uint64_t walks;              /* total traces, < 2^40; 0 = run until every property is discovered
                                    or the target is reached                                     */
    uint32_t max_depth;          /* steps per trace, 1 .. 2^20; 0 = the default 4096             */
    int32_t record_walks;        /* keep one record per trace (sr_gpu_sim_walk_records)          */
    uint64_t target_state_count; /* 0 = none; at least one of walks and target_state_count is required
                                    (SR_ERR_ARG otherwise: a property may never be discovered)   */
    int32_t verbose;             /* one log line per batch on stderr                             */
    int32_t profile;             /* time every launch with HIP events                            */
    int32_t loops;               /* 1 = loop detection (end reason 4, lasso discoveries); 0 = off */
    int32_t reserved0;           /* the tail padding of the 56-byte struct: never read            */
    /* (the struct grew from 56 to 72 bytes here: a caller whose struct_size is 56 is read as all
     * three below being zero, whatever its padding holds)                                         */
    int32_t unique;              /* 1 = count distinct states (see above); 0 = off               */
    uint32_t stale_batches;      /* k > 0: also stop after the first whole batch that ends a run of k
                                    consecutive batches with no new fingerprint; needs unique = 1
                                    (SR_ERR_ARG otherwise) and counts as a bound: walks = 0 without a
                                    target_state_count is then accepted. An overflow of the table
                                    fails such a check with SR_ERR_CAPACITY                       */
    uint64_t unique_capacity;    /* distinct fingerprints the table is sized for (slots: the smallest
                                    power of two >= twice that); 0 = min(walks * (max_depth + 1),
                                    2^28), or 2^28 when walks is 0                                */
} sr_sim_opts;
/* Zeroes the caller's mirror of `size` bytes (at most the library's own size) and sets struct_size
 * to what it wrote and max_depth to 4096. */
void sr_sim_opts_init_sized(sr_sim_opts* opts, uint32_t size);
/* The distinct-state count of a simulation (sr_sim_opts.unique). */
typedef struct sr_sim_unique_result {
    uint32_t struct_size;   /* sizeof this struct in the caller's build (set before the call)     */
    int32_t on;             /* the mode was on; with 0 every field below but batches is 0          */
    uint64_t unique;        /* |U|: distinct fingerprints in the table (a lower bound if overflow) */
    int32_t overflow;       /* an insert was dropped: its probe limit ran out                      */
    int32_t stopped_stale;  /* the check stopped by stale_batches                                  */
    uint64_t slots;         /* the table's slots                                                   */
    uint64_t capacity;      /* the capacity the table was sized for                                */
    uint64_t batches;       /* batches run                                                         */
} sr_sim_unique_result;
/* Fills *out (at most out->struct_size bytes) for a finished simulation. SR_ERR_ARG for a handle
 * that is no simulation or still runs. */
int32_t sr_gpu_sim_unique(const sr_bfs* sim, sr_sim_unique_result* out);
/* The fingerprints of U, sorted ascending (sorted once, at the first call). Writes at most cap of
 * them; returns |U| as counted in the table, or a negative SR_ERR_* (SR_ERR_ARG: no simulation, still
 * running, or the mode was off). */
int64_t sr_gpu_sim_unique_fingerprints(sr_bfs* sim, uint64_t* out, int64_t cap);
/* Per batch, in order, the number of fingerprints it added to U; their sum is |U|. Returns the
 * number of batches (at most cap are written); 0 with the mode off (nothing is recorded then). */
int64_t sr_gpu_sim_batch_new(const sr_bfs* sim, uint64_t* out, int64_t cap);
/* Host-only (no device needed): U of the traces walk0 .. walk0 + nwalks - 1 of a registered model,
 * by the same definition. Writes the distinct fingerprints sorted ascending (at most cap); returns
 * their number, or a negative SR_ERR_*. */
int64_t sr_sim_unique_host(int32_t model_id, const int64_t* params, int32_t nparams, uint64_t seed, uint64_t walk0,
                           uint64_t nwalks, uint32_t max_depth, int32_t loops, uint64_t* out, int64_t cap);
/* Spawns the simulation; returns NULL on error (see sr_last_error). Non-blocking. */
sr_bfs* sr_gpu_sim_spawn(int32_t model_id, const int64_t* params, int32_t nparams, const sr_sim_opts* opts);
/* record_walks = 1: per trace, by trace index, its steps, end reason (1 terminal, 2 depth, 3 fault,
 * 4 loop: only with sr_sim_opts.loops) and the engine's fingerprint of its last state. Returns the number of traces run (at most cap are
 * written), or SR_ERR_ARG for a handle that is no simulation. */
int64_t sr_gpu_sim_walk_records(const sr_bfs* sim, uint32_t* steps, uint32_t* end_reason, uint64_t* final_fp, int64_t cap);
/* record_walks = 1: per trace, by trace index, its loop start: the index (< its steps) of the earlier
 * state a trace of end reason 4 returned to, 0xFFFFFFFF for every other trace. Returns as above. */
int64_t sr_gpu_sim_walk_loop_starts(const sr_bfs* sim, uint32_t* loop_start, int64_t cap);
/* The discovery of property `prop`: the trace index and the step of its hit. Returns 1, or 0 if the
 * property has no discovery (or the handle is no simulation). */
int32_t sr_gpu_sim_hit(const sr_bfs* sim, int32_t prop, uint64_t* walk, uint32_t* step);
/* Host-only (no device needed): trace `walk` of a registered model as the device runs it. Writes its
 * canonical action ids (at most cap), end reason, the fingerprint of its last state and, per
 * property p < nprops, the step of the trace's hit of p (-1 = none). attempts (may be NULL) receives
 * the number of drawn slots whose next state was refused. Returns the steps, or a negative SR_ERR_*. */
int64_t sr_sim_walk(int32_t model_id, const int64_t* params, int32_t nparams, uint64_t seed, uint64_t walk,
                    uint32_t max_depth, int64_t* action_ids, int32_t cap, int32_t* end_reason, uint64_t* final_fp,
                    int32_t* first_hit_step, int32_t nprops, int32_t* attempts);
/* sr_sim_walk with the loops flag of sr_sim_opts: loop_start (may be NULL) receives the trace's loop
 * start, -1 unless its end reason is 4. */
int64_t sr_sim_walk_loops(int32_t model_id, const int64_t* params, int32_t nparams, uint64_t seed, uint64_t walk,
                          uint32_t max_depth, int32_t loops, int64_t* action_ids, int32_t cap, int32_t* end_reason,
                          uint64_t* final_fp, int32_t* first_hit_step, int32_t nprops, int32_t* attempts,
                          int32_t* loop_start);

/* ---- Partitioned search over several GPUs (no counterpart in the reference,
 * which is single-process shared-memory: src/checker/bfs.rs:70-152) ----
 * One process per GPU. Rank 0 creates a unique id, every rank receives it out of band (e.g. a
 * torch.distributed broadcast) and calls sr_dist_init with its rank. The first small levels run
 * replicated on every rank with no collective. After them every level is exchanged DIRECTLY: each
 * rank's expand kernel stores its successor records (8*W bytes each) into the owners' receive
 * buffers through peer pointers (IPC handles across processes, shared once through the
 * communicator) and raises a device flag per level in every owner; owners wait for the flags on
 * the device. No collective and no host step runs inside a level. If a one-off
 * collective probe finds the peer path unusable on any rank (or SR_DIRECT=0), RCCL instead carries
 * ONE all-to-all of fixed-capacity buckets per level, every rank's row in the bucket headers.
 * Counts reported by every rank are global. Discovery paths are gathered on every rank at join
 * (sr_opts.defer_paths = 0, the default), so any rank may ask for them alone. */
#define SR_DIST_ID_BYTES 128
typedef struct sr_dist sr_dist;
int32_t sr_dist_unique_id(uint8_t* id_out);
/* An RCCL communicator (one process per GPU). */
sr_dist* sr_dist_init(int32_t rank, int32_t world, const uint8_t* id, int32_t device);
/* `world` communicators whose ranks are threads of THIS process (rank r on devices[r], or device 0
 * when devices is NULL): the same stream-ordered collectives as RCCL, carried by device copies
 * across the ranks' streams, with a host rendezvous per call that rejects ranks issuing different
 * collectives, and the direct exchange through raw device pointers. Runs the partitioned engine's
 * multi-rank code path on one GPU (tests). Ranks that share a device each need a hardware queue of
 * their own for the direct exchange's device-side waits (GPU_MAX_HW_QUEUES >= world + 2). */
int32_t sr_dist_local_group(int32_t world, const int32_t* devices, sr_dist** comms_out);
/* `world` PROCESSES of one host whose host-side transport is the POSIX shared-memory segment `name`
 * (created by the first rank to open it; rank 0 unlinks it when freed): synchronous staged
 * collectives through per-rank slots of slot_bytes, a barrier in the segment, and the direct
 * exchange through IPC handles. Lets the one-process-per-GPU code path run as separate processes on
 * ONE GPU, where RCCL refuses two ranks on one device (tests, bench rehearsals).
 * devices_distinct = 1 when every rank has its own GPU. */
sr_dist* sr_dist_shm_init(int32_t rank, int32_t world, const char* name, int32_t device, int64_t slot_bytes,
                          int32_t devices_distinct);
int32_t sr_dist_rank(const sr_dist* comm);
int32_t sr_dist_world(const sr_dist* comm);
/* Ranks the transport reports (RCCL: ncclCommCount). */
int32_t sr_dist_nranks(const sr_dist* comm);
/* "rccl", "local" or "shm". */
int32_t sr_dist_kind(const sr_dist* comm, char* buf, int32_t cap);
/* Device synchronisation of this rank, then a collective barrier (bench timing brackets). */
int32_t sr_dist_barrier(sr_dist* comm);
/* Element-wise min (op 0) or max (op 1) of n doubles over the ranks, in place. */
int32_t sr_dist_allreduce_f64(sr_dist* comm, double* values, int32_t n, int32_t op);
void sr_dist_free(sr_dist* comm);

/* The partitioned search's HOST protocol without a GPU (tests): `world` processes on the
 * shared-memory segment `name` (as sr_dist_shm_init, host buffers only) run a 2pc check whose
 * device side is a CPU stand-in (expansion, routing by part_of, the direct exchange's per-slot
 * checksum, one row per partition and level), while the level rows, their error precedence, the
 * pipelined bucket plan and the outcome vote are the engine's own code (dist.hpp). Faults are
 * injected where the device would raise them. Returns SR_OK with *out filled, or the error every
 * rank agreed to fail with (sr_last_error). */
typedef struct sr_dist_host_opts {
    uint32_t struct_size;
    int32_t rm_count;               /* 2pc resource managers (1..=7) */
    uint64_t cmin;                  /* minimum planned bucket capacity (records per pair) */
    int32_t corrupt_level;          /* >= 0: a record this rank receives at that level is altered after
                                       its source checksummed it (once); -1: none */
    int32_t capacity_fail_at_end;   /* this rank alone fails with a capacity error at the end (once) */
    int32_t fail_at_end;            /* this rank alone fails with another error at the end (once) */
    int32_t plan_div;               /* > 1: the planned capacities divided by it (an under-estimate) */
} sr_dist_host_opts;
typedef struct sr_dist_host_result {
    uint64_t unique, state_count, local_unique;  /* global counts; states this rank's partition holds */
    uint32_t max_depth, levels;
    uint32_t attempts, restarts, fallbacks, disagreements;
    uint32_t overflow_level;        /* first level with a bucket over its planned capacity (~0: none) */
    uint32_t first_outcome;         /* this rank's outcome of the first attempt: 0 ok, 1 capacity,
                                       2 exchange, 3 other error (dist.hpp Outcome) */
    uint64_t plan_digest;           /* hash of the planned bucket capacities (equal on every rank) */
} sr_dist_host_result;
int32_t sr_dist_host_protocol(const char* name, int32_t rank, int32_t world, const sr_dist_host_opts* opts,
                              sr_dist_host_result* out);

/* Versions: runtime = what the loaded library reports, compiled = the headers the engine was built
 * against (RCCL: NCCL_VERSION_CODE; HIP: HIP_VERSION). A mismatch means another process-wide copy
 * of the runtime (e.g. one bundled with a Python framework) was loaded first. */
int32_t sr_rccl_version(int32_t* runtime, int32_t* compiled);
int32_t sr_hip_runtime_version(int32_t* runtime, int32_t* compiled);
int32_t sr_device_synchronize(int32_t device);
/* The source digest this library was compiled from (16 hex digits: sha256 over the engine's sources
 * and headers, stateright_amd/build.py `source_digest`). The Python loader refuses a library whose
 * digest differs from the sources beside it, so a stale binary never tests or benches old code. */
const char* sr_build_digest(void);
/* Host-only self-test of the visited set's quotient encoding (kernels.hpp): the key permutation is
 * a bijection and slot values decode to their keys. SR_OK or SR_ERR_ARG (sr_last_error). */
int32_t sr_selftest_tables(void);
/* Host-only self-test of the FAST expansion's level geometry (kernels.hpp level_geometry): the
 * workgroup / chunk / wave / lane shares of a level, fixed and balanced, take every parent of the
 * frontier exactly once over a range of frontier sizes, grids, parents-per-wave caps and waves per
 * workgroup; balanced shares are equal to within one chunk. SR_OK or SR_ERR_ARG (sr_last_error). */
int32_t sr_selftest_level_geometry(void);
/* Host-only self-check of the compiled-in model encodings: every slot a model's optional
 * `self_loops` reports (counted by the FAST expansion without being generated) is enabled and
 * returns the state itself, over every reachable state of 2pc N=1..7 (and its canonical form);
 * and the register clients' linearizability test (paxos, single-copy register) agrees with the
 * tester's serialization search on random histories of 1..6 clients.
 * SR_OK or SR_ERR_ARG (sr_last_error says where). */
int32_t sr_selftest_models(void);
/* Host-only self-check of 2pc's optional FAST-expansion hooks (models.hpp), N = 1..14 in the
 * runtime-n form and the compiled-in 9, 10 and 11, over every reachable state for N <= 4 and 10 000
 * random states per N: `action_masks` gives `apply`'s state for every enabled slot, `enabled_moves`
 * equals `enabled & ~self_loops` and returns the self-loops' count, every slot it leaves changes the
 * state (SELF_LOOPS_EXACT); and the same hooks of the Ladder fixture. SR_OK or SR_ERR_ARG. */
int32_t sr_selftest_action_masks(void);
/* Host-only self-test of the visited set's encodings as the engine chooses them (kernels.hpp
 * make_table_view), through growth: for models of 1, 2 and 4 words and every key width, the views of
 * the tables from the model's smallest (at least 2^10 slots) up to 2^40. Per view, over some thousands of random keys:
 * the home slot is inside the table, the slot value at the first and the last displacement fits the
 * slot and decodes to the permuted key, and the duplicate filter's key is injective where the filter
 * is on. Per growth by 2, 8 and 64: the rehashed slot of every key is the slot a fresh probe finds,
 * the range-by-range rehash is chosen only where new home >> lg is the old home, and the mode
 * (quotient or fingerprint) does not change. Allocates nothing. SR_OK or SR_ERR_ARG (sr_last_error). */
int32_t sr_selftest_table_growth(void);
/* Host-only: the encoding the engine gives a model of `words` (1, 2 or 4) words with a packed key of
 * `key_bits` bits in a table of `slots` (a power of two) slots. out[8]: remainder bits (0:
 * fingerprint mode), displacement bits, key bits, probe limit, 1 for 4-byte slots, duplicate filter
 * (0 none, 1 8-byte entries, 2 compact 4-byte entries), log2 of its entries, log2 of the model's
 * smallest table. SR_ERR_ARG for a table below the model's smallest. */
int32_t sr_table_encoding(int32_t words, int32_t key_bits, uint64_t slots, uint32_t* out);
/* comm == NULL: `virtual_partitions` partitions in this process on opts->device (same protocol;
 * the partitions store into each other's receive buffers). FAST order only. */
sr_bfs* sr_gpu_bfs_spawn_partitioned(sr_dist* comm, int32_t virtual_partitions, int32_t model_id,
                                     const int64_t* params, int32_t nparams, const sr_opts* opts);

/* ---- GpuModel plugins: `impl Model` outside the registry (src/lib.rs:155-237) ----
 * A user writes a GpuModel (the encoding concept of stateright_amd/csrc/models.hpp) and builds it
 * with hipcc into its own shared library, instantiating the engine from
 * include/stateright_gpu_model.hpp; the macro SR_GPU_PLUGIN(name, Model, make) there exports
 * `const sr_plugin* sr_plugin_<name>(void)`. The engine library then runs it like a registered
 * model. The plugin must be built from the same headers (abi). */
#define SR_PLUGIN_ABI 4
typedef struct sr_plugin {
    uint32_t abi;         /* SR_PLUGIN_ABI of the headers the plugin was built with */
    uint32_t opts_size;   /* sizeof(sr_opts) in that build */
    const char* name;
    /* Creates an engine object (comm = NULL and virtual_parts <= 1: one GPU; else partitioned). */
    void* (*create)(const int64_t* params, int32_t nparams, const sr_opts* opts, void* comm, int32_t virtual_parts,
                    char* err, int32_t errcap);
    /* Fingerprint of a state given by its canonical description (needs the model's `undescribe`). */
    int32_t (*fingerprint)(const int64_t* params, int32_t nparams, const int64_t* described, int32_t width,
                           uint64_t* fp_out);
} sr_plugin;

sr_bfs* sr_gpu_bfs_spawn_plugin(const sr_plugin* plugin, const int64_t* params, int32_t nparams, const sr_opts* opts);
sr_bfs* sr_gpu_bfs_spawn_plugin_partitioned(const sr_plugin* plugin, sr_dist* comm, int32_t virtual_partitions,
                                            const int64_t* params, int32_t nparams, const sr_opts* opts);

/* The engine's fingerprint of a state of a registered model, given by its canonical description
 * (the integers sr_gpu_bfs_discovery_path / sr_gpu_bfs_visits return, describe_width of them):
 * what a host-side `Path::from_fingerprints` (src/checker/path.rs:20-86) compares with the chain of
 * sr_gpu_bfs_discovery. Host-only (no device needed). Every registered model but DGraph: the
 * register models (paxos, ABD, single-copy) describe their LinearizabilityTester history
 * canonically (per client the Get's returned value and its real-time predecessors), so their
 * description determines the state. SR_ERR_UNSUPPORTED for DGraph. */
int32_t sr_model_fingerprint(int32_t model_id, const int64_t* params, int32_t nparams, const int64_t* described,
                             int32_t width, uint64_t* fp_out);
/* Host-only self-test of sr_model_fingerprint: a host BFS over up to max_states reachable states of
 * the model; every state's description must give the state back and the engine's fingerprint of
 * it. Returns the states checked, or SR_ERR_* (sr_last_error says which state failed). */
int64_t sr_selftest_describe(int32_t model_id, const int64_t* params, int32_t nparams, int64_t max_states);

/* ---- the visited-set audit (csrc/kernels_audit.hpp) ----
 * A check run with sr_opts.counters audits its final visited set against its arena, which lists
 * every visited state, after the level loop: one pass over the slots and one over the arena's
 * states (a partitioned check: every partition's table against that partition's states, summed over
 * partitions and ranks). 72 bytes.
 * Clean: misplaced, duplicates, arena_missing, arena_shared and meta_wrong are all 0, and
 * occupied == arena_states == unique_state_count when the check explored everything. After an early
 * exit (every property discovered inside a level) or a target stop, the level being expanded at the
 * stop, or a speculative one enqueued past it, has claimed slots for states no arena level lists:
 * then only occupied >= arena_states holds. Init states the model lists twice are two arena states
 * of one slot and count in arena_shared. The audit proves that table and arena are equal as sets
 * (and in FIFO order that meta names each state's level and parent); it says nothing about states
 * that were never claimed. */
typedef struct sr_table_audit {
    uint32_t ran;            /* 1: the audit ran (sr_opts.counters); else every field is 0           */
    uint32_t fifo;           /* 1: FIFO order, meta was audited                                      */
    uint64_t slots;          /* slots of the final table(s)                                          */
    uint64_t occupied;       /* non-zero slots                                                       */
    uint64_t misplaced;      /* occupied slots whose stored displacement is at or past the probe limit,
                                whose key cannot have that home, or with a vacant slot between their
                                home and themselves                                                   */
    uint64_t duplicates;     /* occupied slots whose key another slot in [home, slot) holds too       */
    uint64_t arena_states;   /* states in the arena (every level the check accounted for)            */
    uint64_t arena_missing;  /* ... that a lookup does not find in the table                          */
    uint64_t arena_shared;   /* ... that resolve to a slot another arena state resolved to before     */
    uint64_t meta_wrong;     /* FIFO order: ... whose slot's meta is not (own level, parent's rank);
                                level 0 carries 0                                                    */
} sr_table_audit;
/* Copies at most `size` bytes of the finished check's audit; returns the engine's
 * sizeof(sr_table_audit), or SR_ERR_ARG. */
int32_t sr_gpu_bfs_table_audit(const sr_bfs* bfs, sr_table_audit* out, uint32_t size);
/* GPU self-test of the visited set's growth kernels (rehash, rehash_ranges<u32|u64>, rehash_spill,
 * remap_slots; csrc/rehash_selftest.hpp) on synthetic tables built on the host, grown through the
 * engines' own launch routine and compared slot by slot with a sequential host rebuild. SR_OK, or
 * SR_ERR_ARG with the first failing case in sr_last_error (SR_ERR_HIP: a runtime error).
 * device < 0: host only, nothing is launched: every case is built and its expectations checked
 * against the host model (the random fill must spill, the long run must extend its window twice). */
int32_t sr_selftest_rehash_gpu(int32_t device);

/* ---- The certificate of a finished check (sr_opts.certify; stateright_amd/csrc/certify.hpp has the exact
 * definitions) ----
 * After the search, GPU passes re-derive from the arena, its level offsets, the parent ranks and the final
 * visited set that the arena lists exactly the reachable set, level by level, with a valid BFS tree, and in
 * FIFO order in the reference's visit order. A clean certificate has every error counter at 0. One GPU only:
 * a partitioned check leaves ran = 0. The closure counters are filled only when the search explored everything
 * (explored_all); after an early exit or a target stop the roots, map, tree, order and property figures hold.
 * The first `inits` arena states are the init states in REVERSE order, as the reference visits them. */
typedef struct sr_certificate {
    uint32_t ran;              /* 1: the pass ran; else every counter is 0                                    */
    uint32_t fifo;             /* 1: FIFO order, the tags (meta) were checked                                 */
    uint32_t explored_all;     /* 1: the search explored everything, the closure pass ran                     */
    uint32_t skipped;          /* 1: the level map (4 bytes per slot) could not be allocated; ran = 0         */
    uint64_t states;           /* arena states (every level the check accounted for)                          */
    uint64_t levels;           /* arena levels                                                                */
    uint64_t inits;            /* init states, as the model lists them                                        */
    uint64_t repeated_inits;   /* ... that repeat an earlier one                                              */
    uint64_t roots_wrong;      /* level 0: indices that do not hold their init state                          */
    uint64_t map_missing;      /* states the table does not hold                                              */
    uint64_t tree_range;       /* parent ranks at or past the previous level's size (counted, never loaded)   */
    uint64_t tree_edge;        /* states that no enabled slot of their parent produces                        */
    uint64_t tree_slot;        /* FIFO: states whose tag is not parent rank * max_actions + first such slot   */
    uint64_t edges;            /* (state, enabled slot) pairs whose apply succeeds, repeated init states aside */
    uint64_t repeated_edges;   /* ... of the repeated init states: inits + edges + repeated_edges is the
                                  search's state_count                                                        */
    uint64_t closure_missing;  /* successors the table does not hold                                          */
    uint64_t closure_unlisted; /* successors in a slot that no arena state maps to                            */
    uint64_t closure_late;     /* successors listed more than one level below their generator                 */
    uint64_t fifo_not_first;   /* FIFO: successors one level down with an earlier generator than the recorded */
    uint64_t fifo_order;       /* FIFO: neighbours of a level whose tags do not strictly increase             */
    uint32_t nprops;           /* the model's properties                                                      */
    uint32_t pmask;            /* the ones counted below: those outside emask() | lmask() | smask()           */
    uint64_t holds[32];        /* per property: states where `discovers` holds                                */
    uint64_t first_index[32];  /* ... the lowest such arena index (all ones: none)                            */
    uint64_t disc_index[32];   /* ... the engine's own discovery, lstart[level] + rank (all ones: none)       */
    uint64_t disc_wrong[32];   /* ... 1: `discovers` is false there                                           */
    uint32_t first_level[32];  /* ... the level of first_index (all ones: none)                               */
    uint32_t disc_level[32];   /* ... the level of disc_index (all ones: none, or past the arena)             */
    double pass_ms;            /* host time of the pass                                                       */
} sr_certificate;
/* Copies at most `size` bytes of the finished check's certificate; returns the engine's
 * sizeof(sr_certificate), or SR_ERR_ARG. */
int32_t sr_gpu_bfs_certificate(const sr_bfs* bfs, sr_certificate* out, uint32_t size);
/* Self-test of the certificate kernels (csrc/certify_selftest.hpp): arenas and tables built on the host by a
 * sequential search of small models, clean and with planted errors (a wrong parent, an out-of-range parent
 * rank, a missing or unowned table entry, a late or unreachable state, swapped neighbours, a later generator's
 * tag, a replaced init state); every counter of every case must equal the host evaluation of the definitions.
 * SR_OK, or SR_ERR_ARG with the first failing case in sr_last_error (SR_ERR_HIP: a runtime error).
 * device < 0: host only, nothing is launched: the cases are built, evaluated and cross-checked (a clean arena
 * gives zeros, every planted error moves the counter it was planted for). */
int32_t sr_selftest_certify_gpu(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* STATERIGHT_GPU_H */
