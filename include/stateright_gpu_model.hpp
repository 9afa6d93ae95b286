/*
 * stateright_gpu_model.hpp — write a GpuModel and build it into a plugin for the MI355X engine.
 *
 * The reference checks any `impl Model` (src/lib.rs:155-237). Device code cannot call host
 * closures, so a model for the GPU engine is a C++ struct, the GpuModel concept, compiled with
 * hipcc together with the engine templates this header brings in; the result is a shared library
 * that the engine library (include/stateright_gpu.h, sr_gpu_bfs_spawn_plugin) runs like a
 * registered model. A GpuModel M provides (models in stateright_amd/csrc/models.hpp):
 *
 *   static constexpr int W, MW, NPROPS;      words per state, 64-bit words of the action mask, properties
 *   int max_actions(), max_out_degree();     action slots (`actions()` positions), max successors
 *   SR_HD void enabled(const u64* s, u64* m);           bit a: slot a is listed by `actions(s)`
 *   SR_HD bool apply(const u64* s, int a, u64* out);    `next_state(s, a)` is Some and within boundary
 *   SR_HD bool discovers(int p, const u64* s);           always: !condition; sometimes/eventually: condition
 *   host: init_states(u64*) -> count, expectation(p), prop_name(p), describe_width(), describe(s, i64*),
 *         action_id(s, a), action_name(id), action_id_bound()
 *         init_states writes at most 256 states (sr::MAX_INIT_STATES) unless the model reports its
 *         count with init_count(); the engine checks the count once at spawn (SR_ERR_ARG)
 *   optional: init_count()                    the number of init states (any count; the engine sizes
 *                                             its host buffers from it)
 *             undescribe(const i64*, u64*)    (sr_plugin.fingerprint)
 *             emask()                         (the mask of `eventually` properties)
 *             SR_HD u32 lmask()               the mask of LEADS-TO properties (expectation(p) == LEADS_TO = 3:
 *                                             "whenever the trigger holds, the condition holds then or later"),
 *                                             disjoint from emask(); with it comes
 *                                             SR_HD bool leads_from(int p, const u64* s), the TRIGGER of such a
 *                                             property, while discovers(p, s) is its condition, as for
 *                                             `eventually`. Only the complete liveness check decides such a
 *                                             property, and it refuses plugins, so a plugin's leads-to
 *                                             properties are left unchecked by every checker (the plugin ABI
 *                                             version is unchanged); a model without lmask() has none
 *             u32 smask()                     the mask of STEP properties (expectation(p) == ALWAYS_STEP = 4: an
 *                                             invariant over steps, TLA+'s [][A]_v), disjoint from emask() and
 *                                             lmask(); with it comes the hook
 *                                             SR_HD bool step_holds(int p, const u64* s, int a, const u64* t):
 *                                             whether the step from s through slot a to t = apply(s, a) is
 *                                             allowed (t may equal s: the hook decides about stuttering), while
 *                                             discovers(p, s) is false everywhere, so the search never discovers
 *                                             it. Only the step pass decides such a property, behind a one-GPU
 *                                             spawn_bfs / spawn_dfs that explored everything (no option;
 *                                             stateright_amd/csrc/step.hpp); a plugin takes it like a registered
 *                                             model (the plugin ABI version is unchanged:
 *                                             examples/plugins/step_counter.hip); a model without smask() has none
 *             qkey_bits(), SR_HD qkey(s)      (exact quotient visited set for multi-word states)
 *             SR_HD self_loops(s, enabled, out)   out = enabled slots whose next_state is s itself:
 *                                             FAST expansion counts them (state_count) without
 *                                             generating them. Every slot reported must be a
 *                                             self-loop; an unreported one is still detected
 *                                             (2pc reports all of them: 37% of successors)
 *             SR_HD enabled_moves(s, out) -> u32   out = enabled & ~self_loops in one pass, returns the
 *                                             number of self-loops removed (used in their place)
 *             static constexpr bool SELF_LOOPS_EXACT = true    every slot those leave changes the
 *                                             state: no successor is compared with its parent
 *             SR_HD action_masks(a, u64* clr, u64* set)   W == 1: for every enabled slot a,
 *                                             apply(s, a) = (s & ~clr) | set with masks of the slot
 *                                             alone; total over slots 0 .. 64 MW - 1. FAST expansion
 *                                             then looks successors up in a per-wave table (models of
 *                                             at most 64 slots; SR_ACTION_TABLE=0 keeps apply)
 *             SR_HD canonical(s, out)         a canonical representative under the model's symmetry
 *                                             (the opt-in symmetry_canonical reduction)
 *             SR_HD int cover_class(s, a)     the ACTION CLASS of slot a at state s, for the coverage pass
 *                                             (sr_opts.coverage): 0 <= class < cover_classes(), asked for
 *                                             the slots of enabled(s) only; with it come the host members
 *                                             int cover_classes() (at most 1024) and
 *                                             std::string cover_class_name(int c). Without the three, the
 *                                             class of a slot is the slot, named action_name(a) if the
 *                                             model's action ids are its slots (action_id_bound() ==
 *                                             max_actions()), "slot <a>" otherwise. For a model whose slots
 *                                             are positions (of a network, of a thread) rather than actions
 *                                             (Increment: the canonical action id; paxos: the message kind)
 *             SR_HD bool faulted(s)           s lost information when it was built (a state its
 *                                             encoding cannot hold): the check ends with
 *                                             SR_ERR_UNSUPPORTED; model_name() (host) names the
 *                                             model in that error
 *
 * Equal states must have equal words (the words ARE the state), and slots are enumerated in the
 * reference's `actions()` order, so FIFO runs reproduce the reference's visit order and paths.
 *
 *   #include "stateright_gpu_model.hpp"
 *   struct MyModel { ... };
 *   MyModel make_my_model(const int64_t* params, int32_t nparams, int device) { ... }
 *   SR_GPU_PLUGIN(my_model, MyModel, make_my_model)
 *
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<repo>/include my_model.hip \
 *         -o libmy_model.so -L/opt/rocm/lib -lrccl
 *
 * `make` builds the model from integer parameters (device < 0: host-only use, e.g. fingerprints)
 * and may throw sr::Error(SR_ERR_ARG, "...") for bad parameters. examples/plugins/sliding_puzzle.hip
 * is a complete example (the sliding puzzle of the reference's crate documentation, src/lib.rs:40-116).
 */
#ifndef STATERIGHT_GPU_MODEL_HPP
#define STATERIGHT_GPU_MODEL_HPP

#include "stateright_gpu.h"
#include "../stateright_amd/csrc/engine.hpp"

#define SR_GPU_PLUGIN(NAME, MODEL, MAKE)                                                                    \
    extern "C" const sr_plugin* sr_plugin_##NAME(void) {                                                    \
        static const sr_plugin p = {                                                                        \
            SR_PLUGIN_ABI, (uint32_t)sizeof(sr_opts), #NAME,                                                \
            [](const int64_t* a, int32_t n, const sr_opts* o, void* c, int32_t v, char* e, int32_t cap) -> void* { \
                return ::sr::plugin_create<MODEL>(MAKE, a, n, o, c, v, e, cap);                           \
            },                                                                                              \
            [](const int64_t* a, int32_t n, const int64_t* d, int32_t w, uint64_t* fp) -> int32_t {         \
                return ::sr::plugin_fingerprint<MODEL>(MAKE, a, n, d, w, fp);                             \
            }};                                                                                             \
        return &p;                                                                                          \
    }

#endif /* STATERIGHT_GPU_MODEL_HPP */
