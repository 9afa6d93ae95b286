"""ctypes binding to the MI355X engine's C ABI (include/stateright_gpu.h).

The shared library `stateright_amd/libstateright_gpu.so` is built in-tree by
`stateright_amd.build.build()` (hipcc --offload-arch=gfx950). There is no fallback: if the library
is missing, or no HIP device is visible, every checker call raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SR_LIB_PATH") or os.path.join(HERE, "libstateright_gpu.so")

SR_MODEL_LINEAR_EQUATION = 1
SR_MODEL_BINARY_CLOCK = 2
SR_MODEL_2PC = 3
SR_MODEL_INCREMENT = 4
SR_MODEL_INCREMENT_LOCK = 5
SR_MODEL_DGRAPH = 6
SR_MODEL_PAXOS = 7
SR_MODEL_PINGPONG = 9
SR_MODEL_ACTOR_FIXTURE = 10
SR_MODEL_ABD = 11
SR_MODEL_SINGLE_COPY = 12
SR_MODEL_LADDER = 13
SR_MODEL_SPREAD = 14
SR_MODEL_LIVE_GRAPH = 15
SR_MODEL_2PC_LIVE = 16
SR_MODEL_SPIN_LOCK = 17
SR_MODEL_FAIR_RINGS = 18
SR_MODEL_LEADS_GRAPH = 19
SR_MODEL_REQ_LOCK = 20
SR_MODEL_LEADS_DGRAPH = 21
SR_MODEL_STEP_GRAPH = 22
SR_MODEL_2PC_STEP = 23
SR_MODEL_STEP_DGRAPH = 24

SR_ORDER_AUTO, SR_ORDER_FIFO, SR_ORDER_FAST = 0, 1, 2
SR_ALWAYS, SR_EVENTUALLY, SR_SOMETIMES, SR_LEADS_TO, SR_ALWAYS_STEP = 0, 1, 2, 3, 4
# sr_stats.root_path (enum sr_root_path)
SR_ROOTS_INLINE, SR_ROOTS_FUSED, SR_ROOTS_LAUNCHES, SR_ROOTS_HEAD, SR_ROOTS_PARTS, SR_ROOTS_BUFFER = 1, 2, 3, 4, 5, 6


class sr_opts(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("target_state_count", ctypes.c_uint64),
        ("order", ctypes.c_int32),
        ("record_visits", ctypes.c_int32),
        ("capacity_hint", ctypes.c_uint64),
        ("profile", ctypes.c_int32),
        ("verbose", ctypes.c_int32),
        ("counters", ctypes.c_int32),
        ("defer_paths", ctypes.c_int32),
        ("symmetry", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("liveness", ctypes.c_int32),  # (the struct grew from 56 to 64 bytes for it)
        ("coverage", ctypes.c_int32),  # (what was reserved1: same offset)
        ("certify", ctypes.c_int32),  # (the struct grew from 64 to 72 bytes for it)
        ("reserved1", ctypes.c_int32),
    ]


# sr_opts.liveness (enum sr_liveness_mode) and sr_live_result.end_kind (enum sr_live_end)
SR_LIVENESS_OFF, SR_LIVENESS_COMPLETE, SR_LIVENESS_PROGRESS, SR_LIVENESS_WEAK, SR_LIVENESS_STRONG = 0, 1, 2, 3, 4
SR_LIVE_END_NONE, SR_LIVE_END_TERMINAL, SR_LIVE_END_LOOP, SR_LIVE_END_STUTTER = 0, 1, 2, 3


class sr_live_result(ctypes.Structure):
    _fields_ = [
        ("ran", ctypes.c_int32),
        ("init_index", ctypes.c_int32),
        ("not_p_states", ctypes.c_uint64),
        ("surviving", ctypes.c_uint64),
        ("examined", ctypes.c_uint64),
        ("rounds", ctypes.c_uint32),
        ("end_kind", ctypes.c_uint32),  # (what was reserved0: same offset)
        ("witness_len", ctypes.c_int64),
        ("loop_start", ctypes.c_int64),
        ("pass_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class _LiveFairStats(ctypes.Structure):
    """sr_live_weak and sr_live_strong: one layout, but for the second field (reserved0 / levels)."""

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


def _live_fair_fields(second):
    return [
        ("ran", ctypes.c_int32),
        second,
        ("cyclic_states", ctypes.c_uint64),
        ("components", ctypes.c_uint64),
        ("fair_components", ctypes.c_uint64),
        ("goal_states", ctypes.c_uint64),
        ("fair_states", ctypes.c_uint64),
        ("stem_len", ctypes.c_int64),
        ("loop_len", ctypes.c_int64),
        ("scc_rounds", ctypes.c_uint32),
        ("reach_rounds", ctypes.c_uint32),
        ("segments", ctypes.c_uint32),
        ("reserved1", ctypes.c_uint32),
        ("pass_ms", ctypes.c_double),
    ]


class sr_live_weak(_LiveFairStats):
    _fields_ = _live_fair_fields(("reserved0", ctypes.c_int32))


class sr_live_strong(_LiveFairStats):
    _fields_ = _live_fair_fields(("levels", ctypes.c_uint32))


class sr_live_leads(ctypes.Structure):
    _fields_ = [
        ("ran", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("triggered", ctypes.c_uint64),
        ("pending", ctypes.c_uint64),
        ("violating", ctypes.c_uint64),
        ("trigger_index", ctypes.c_int64),
        ("trigger_depth", ctypes.c_int64),
        ("seed_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


class sr_step_result(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("ran", ctypes.c_int32),
        ("edges", ctypes.c_uint64),
        ("violations", ctypes.c_uint64),
        ("sources", ctypes.c_uint64),
        ("step_index", ctypes.c_int64),
        ("step_action", ctypes.c_int64),
        ("init_index", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("witness_len", ctypes.c_int64),
        ("scan_ms", ctypes.c_double),
        ("min_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved0")}


class sr_coverage(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("ran", ctypes.c_int32),
        ("states", ctypes.c_uint64),
        ("terminal", ctypes.c_uint64),
        ("stutter_ends", ctypes.c_uint64),
        ("max_out_degree", ctypes.c_uint32),
        ("classes", ctypes.c_int32),
        ("nprops", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("pass_ms", ctypes.c_double),
        ("out_degree", ctypes.c_uint64 * 64),
    ]

    def as_dict(self):
        out = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved0", "out_degree")}
        out["out_degree"] = list(self.out_degree)
        return out


class sr_sim_opts(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("walks", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint32),
        ("record_walks", ctypes.c_int32),
        ("target_state_count", ctypes.c_uint64),
        ("verbose", ctypes.c_int32),
        ("profile", ctypes.c_int32),
        ("loops", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),  # (the tail padding of the 56-byte struct: never read)
        ("unique", ctypes.c_int32),  # (the struct grew from 56 to 72 bytes for the distinct-state count)
        ("stale_batches", ctypes.c_uint32),
        ("unique_capacity", ctypes.c_uint64),
    ]


class sr_sim_unique_result(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("on", ctypes.c_int32),
        ("unique", ctypes.c_uint64),
        ("overflow", ctypes.c_int32),
        ("stopped_stale", ctypes.c_int32),
        ("slots", ctypes.c_uint64),
        ("capacity", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


# end reasons of a simulated walk (csrc/sim.hpp SimEnd); SIM_LOOP only with loop detection
SIM_TERMINAL, SIM_DEPTH, SIM_FAULT = 1, 2, 3
SIM_LOOP = 4
SIM_LOOP_WINDOW = 8


class sr_stats(ctypes.Structure):
    _fields_ = [
        ("level_loop_sec", ctypes.c_double),
        ("total_sec", ctypes.c_double),
        ("expand_kernel_ms", ctypes.c_double),
        ("expand_launches", ctypes.c_uint64),
        ("levels", ctypes.c_uint64),
        ("table_capacity", ctypes.c_uint64),
        ("rehashes", ctypes.c_uint64),
        ("algorithmic_bytes", ctypes.c_uint64),
        ("successors", ctypes.c_uint64),
        ("words_per_state", ctypes.c_uint32),
        ("order_used", ctypes.c_uint32),
        ("restarts", ctypes.c_uint32),
        ("pipelined", ctypes.c_uint32),
        ("records_routed", ctypes.c_uint64),
        ("head_levels", ctypes.c_uint64),
        ("probes", ctypes.c_uint64),
        ("cas", ctypes.c_uint64),
        ("max_displacement", ctypes.c_uint64),
        ("displacement_limit", ctypes.c_uint32),
        ("table_doublings", ctypes.c_uint32),
        ("exchange_fallbacks", ctypes.c_uint32),
        ("owner_key", ctypes.c_uint32),
        ("balanced_levels", ctypes.c_uint32),
        ("table_encoding", ctypes.c_uint32),
        ("root_path", ctypes.c_uint32),
        ("reserved1", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class sr_table_audit(ctypes.Structure):
    _fields_ = [
        ("ran", ctypes.c_uint32),
        ("fifo", ctypes.c_uint32),
        ("slots", ctypes.c_uint64),
        ("occupied", ctypes.c_uint64),
        ("misplaced", ctypes.c_uint64),
        ("duplicates", ctypes.c_uint64),
        ("arena_states", ctypes.c_uint64),
        ("arena_missing", ctypes.c_uint64),
        ("arena_shared", ctypes.c_uint64),
        ("meta_wrong", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class sr_certificate(ctypes.Structure):
    _fields_ = [
        ("ran", ctypes.c_uint32),
        ("fifo", ctypes.c_uint32),
        ("explored_all", ctypes.c_uint32),
        ("skipped", ctypes.c_uint32),
        ("states", ctypes.c_uint64),
        ("levels", ctypes.c_uint64),
        ("inits", ctypes.c_uint64),
        ("repeated_inits", ctypes.c_uint64),
        ("roots_wrong", ctypes.c_uint64),
        ("map_missing", ctypes.c_uint64),
        ("tree_range", ctypes.c_uint64),
        ("tree_edge", ctypes.c_uint64),
        ("tree_slot", ctypes.c_uint64),
        ("edges", ctypes.c_uint64),
        ("repeated_edges", ctypes.c_uint64),
        ("closure_missing", ctypes.c_uint64),
        ("closure_unlisted", ctypes.c_uint64),
        ("closure_late", ctypes.c_uint64),
        ("fifo_not_first", ctypes.c_uint64),
        ("fifo_order", ctypes.c_uint64),
        ("nprops", ctypes.c_uint32),
        ("pmask", ctypes.c_uint32),
        ("holds", ctypes.c_uint64 * 32),
        ("first_index", ctypes.c_uint64 * 32),
        ("disc_index", ctypes.c_uint64 * 32),
        ("disc_wrong", ctypes.c_uint64 * 32),
        ("first_level", ctypes.c_uint32 * 32),
        ("disc_level", ctypes.c_uint32 * 32),
        ("pass_ms", ctypes.c_double),
    ]

    # the error counters: all 0 in a clean certificate (the per-property disc_wrong aside)
    ERRORS = ("roots_wrong", "map_missing", "tree_range", "tree_edge", "tree_slot", "closure_missing", "closure_unlisted",
              "closure_late", "fifo_not_first", "fifo_order")

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v)[:self.nprops] if name in ("holds", "first_index", "disc_index", "disc_wrong", "first_level", "disc_level") else v
        return out


class sr_dist_host_opts(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("rm_count", ctypes.c_int32),
        ("cmin", ctypes.c_uint64),
        ("corrupt_level", ctypes.c_int32),
        ("capacity_fail_at_end", ctypes.c_int32),
        ("fail_at_end", ctypes.c_int32),
        ("plan_div", ctypes.c_int32),
    ]


class sr_dist_host_result(ctypes.Structure):
    _fields_ = [
        ("unique", ctypes.c_uint64),
        ("state_count", ctypes.c_uint64),
        ("local_unique", ctypes.c_uint64),
        ("max_depth", ctypes.c_uint32),
        ("levels", ctypes.c_uint32),
        ("attempts", ctypes.c_uint32),
        ("restarts", ctypes.c_uint32),
        ("fallbacks", ctypes.c_uint32),
        ("disagreements", ctypes.c_uint32),
        ("overflow_level", ctypes.c_uint32),
        ("first_outcome", ctypes.c_uint32),
        ("plan_digest", ctypes.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# (name, restype, argtypes) of every exported entry point; tests check this list against the header.
_P = ctypes.c_void_p
_I64P = ctypes.POINTER(ctypes.c_int64)
SIGNATURES = [
    ("sr_opts_init", None, [ctypes.POINTER(sr_opts)]),
    ("sr_opts_init_sized", None, [ctypes.POINTER(sr_opts), ctypes.c_uint32]),
    ("sr_last_error", ctypes.c_char_p, []),
    ("sr_device_count", ctypes.c_int, []),
    ("sr_gpu_bfs_spawn", _P, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.POINTER(sr_opts)]),
    ("sr_gpu_bfs_join", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_is_done", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_is_running", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_state_count", ctypes.c_uint64, [_P]),
    ("sr_gpu_bfs_unique_state_count", ctypes.c_uint64, [_P]),
    ("sr_gpu_bfs_max_depth", ctypes.c_uint32, [_P]),
    ("sr_gpu_bfs_stats", ctypes.c_int32, [_P, ctypes.POINTER(sr_stats)]),
    ("sr_gpu_bfs_stats_sized", ctypes.c_int32, [_P, ctypes.POINTER(sr_stats), ctypes.c_uint32]),
    ("sr_gpu_bfs_launch_counters", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                    ctypes.c_int64]),
    ("sr_gpu_bfs_launch_profile", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64),
                                                   ctypes.c_int64]),
    ("sr_gpu_bfs_property_count", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_property", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int32)]),
    ("sr_gpu_bfs_discovery", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32]),
    ("sr_gpu_bfs_discovery_path", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, _I64P, ctypes.c_int64]),
    ("sr_gpu_bfs_describe_width", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_action_name", ctypes.c_int32, [_P, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int32]),
    ("sr_gpu_bfs_action_id_bound", ctypes.c_int64, [_P]),
    ("sr_gpu_bfs_init_count", ctypes.c_int32, [_P]),
    ("sr_gpu_bfs_replay", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, _I64P, ctypes.c_int64,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    ("sr_gpu_bfs_replay_trace", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]),
    ("sr_gpu_bfs_explore", ctypes.c_int32, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, _I64P,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64), _I64P,
                                            ctypes.c_int32]),
    ("sr_gpu_bfs_visits", ctypes.c_int64, [_P, _I64P, ctypes.c_int64]),
    ("sr_gpu_bfs_visit_tree", ctypes.c_int64, [_P, _I64P, _I64P, ctypes.c_int64]),
    ("sr_gpu_bfs_free", None, [_P]),
    ("sr_gpu_bfs_liveness", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(sr_live_result)]),
    ("sr_host_graph", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int64, _I64P, ctypes.c_int64]),
    ("sr_liveness_host", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                          ctypes.POINTER(sr_live_result), _I64P, ctypes.c_int32]),
    ("sr_liveness_host_fair", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                               ctypes.POINTER(sr_live_result), _I64P, ctypes.c_int32]),
    ("sr_gpu_bfs_sink_kind", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32]),
    ("sr_gpu_bfs_liveness_weak", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(sr_live_weak)]),
    ("sr_liveness_host_weak", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                               ctypes.POINTER(sr_live_result), ctypes.POINTER(sr_live_weak), _I64P, ctypes.c_int32]),
    ("sr_gpu_bfs_loop_fair", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32]),
    ("sr_gpu_bfs_liveness_strong", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(sr_live_strong)]),
    ("sr_liveness_host_strong", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                 ctypes.POINTER(sr_live_result), ctypes.POINTER(sr_live_strong), _I64P, ctypes.c_int32]),
    ("sr_gpu_bfs_liveness_leads", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(sr_live_leads)]),
    ("sr_gpu_bfs_replay_triggers", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    ("sr_liveness_host_leads", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.POINTER(sr_live_result), ctypes.POINTER(sr_live_leads), _I64P, ctypes.c_int32]),
    ("sr_gpu_bfs_loop_strongly_fair", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32]),
    ("sr_gpu_bfs_coverage", ctypes.c_int32, [_P, ctypes.POINTER(sr_coverage)]),
    ("sr_gpu_bfs_coverage_classes", ctypes.c_int32, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                     ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]),
    ("sr_gpu_bfs_coverage_props", ctypes.c_int32, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]),
    ("sr_gpu_bfs_coverage_class_name", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]),
    ("sr_coverage_host", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(sr_coverage),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]),
    ("sr_gpu_bfs_step", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(sr_step_result)]),
    ("sr_gpu_bfs_replay_step", ctypes.c_int32, [_P, ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32]),
    ("sr_step_host", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                      ctypes.POINTER(sr_step_result), _I64P, ctypes.c_int32]),
    ("sr_sim_opts_init_sized", None, [ctypes.POINTER(sr_sim_opts), ctypes.c_uint32]),
    ("sr_gpu_sim_spawn", _P, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.POINTER(sr_sim_opts)]),
    ("sr_gpu_sim_walk_records", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64]),
    ("sr_gpu_sim_hit", ctypes.c_int32, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
    ("sr_sim_walk", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                     _I64P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                     ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("sr_gpu_sim_walk_loop_starts", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64]),
    ("sr_sim_walk_loops", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                           ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("sr_gpu_sim_unique", ctypes.c_int32, [_P, ctypes.POINTER(sr_sim_unique_result)]),
    ("sr_gpu_sim_unique_fingerprints", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64]),
    ("sr_gpu_sim_batch_new", ctypes.c_int64, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64]),
    ("sr_sim_unique_host", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_int64]),
    ("sr_dist_unique_id", ctypes.c_int32, [ctypes.c_char_p]),
    ("sr_dist_init", _P, [ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]),
    ("sr_dist_local_group", ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_P)]),
    ("sr_dist_shm_init", _P, [ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64,
                              ctypes.c_int32]),
    ("sr_dist_rank", ctypes.c_int32, [_P]),
    ("sr_dist_world", ctypes.c_int32, [_P]),
    ("sr_dist_nranks", ctypes.c_int32, [_P]),
    ("sr_dist_kind", ctypes.c_int32, [_P, ctypes.c_char_p, ctypes.c_int32]),
    ("sr_dist_barrier", ctypes.c_int32, [_P]),
    ("sr_dist_allreduce_f64", ctypes.c_int32, [_P, ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32]),
    ("sr_dist_free", None, [_P]),
    ("sr_dist_host_protocol", ctypes.c_int32, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.POINTER(sr_dist_host_opts), ctypes.POINTER(sr_dist_host_result)]),
    ("sr_rccl_version", ctypes.c_int32, [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("sr_hip_runtime_version", ctypes.c_int32, [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("sr_device_synchronize", ctypes.c_int32, [ctypes.c_int32]),
    ("sr_build_digest", ctypes.c_char_p, []),
    ("sr_selftest_tables", ctypes.c_int32, []),
    ("sr_selftest_level_geometry", ctypes.c_int32, []),
    ("sr_selftest_models", ctypes.c_int32, []),
    ("sr_selftest_action_masks", ctypes.c_int32, []),
    ("sr_selftest_table_growth", ctypes.c_int32, []),
    ("sr_table_encoding", ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]),
    ("sr_gpu_bfs_spawn_plugin", _P, [_P, _I64P, ctypes.c_int32, ctypes.POINTER(sr_opts)]),
    ("sr_gpu_bfs_spawn_plugin_partitioned", _P, [_P, _P, ctypes.c_int32, _I64P, ctypes.c_int32,
                                                 ctypes.POINTER(sr_opts)]),
    ("sr_model_fingerprint", ctypes.c_int32, [ctypes.c_int32, _I64P, ctypes.c_int32, _I64P, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_uint64)]),
    ("sr_selftest_describe", ctypes.c_int64, [ctypes.c_int32, _I64P, ctypes.c_int32, ctypes.c_int64]),
    ("sr_gpu_bfs_spawn_partitioned", _P, [_P, ctypes.c_int32, ctypes.c_int32, _I64P, ctypes.c_int32,
                                          ctypes.POINTER(sr_opts)]),
    ("sr_gpu_bfs_table_audit", ctypes.c_int32, [_P, ctypes.POINTER(sr_table_audit), ctypes.c_uint32]),
    ("sr_selftest_rehash_gpu", ctypes.c_int32, [ctypes.c_int32]),
    ("sr_gpu_bfs_certificate", ctypes.c_int32, [_P, ctypes.POINTER(sr_certificate), ctypes.c_uint32]),
    ("sr_selftest_certify_gpu", ctypes.c_int32, [ctypes.c_int32]),
]

SR_DIST_ID_BYTES = 128

_lib = None


def load():
    """Loads the engine library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"MI355X engine library not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
        lib = ctypes.CDLL(LIB_PATH)
        ab = os.environ.get("SR_LIB_DIGEST_CHECK", "1") == "0"
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name, None)
            if fn is None and ab:  # an A/B build of older sources: entry points it lacks stay unbound
                continue
            if fn is None:
                raise ImportError(f"{LIB_PATH} lacks {name}: rebuild it")
            fn.restype = res
            fn.argtypes = args
        check_digest(lib)
        _lib = lib
    return _lib


class StaleLibraryError(ImportError):
    pass


def check_digest(lib, sources_root=None):
    """Refuses a library compiled from other sources than the ones beside it: sr_build_digest()
    must equal build.source_digest() (stateright_amd/build.py). SR_LIB_DIGEST_CHECK=0 turns the
    check off; only scripts/gpu_lib_ab.sh does that, to time a saved build of older sources against
    the current one (bench.py still records both digests in its line)."""
    if os.environ.get("SR_LIB_DIGEST_CHECK", "1") == "0":
        return
    from . import build
    want = build.source_digest() if sources_root is None else build.source_digest_at(sources_root)
    got = lib.sr_build_digest().decode()
    if got != want:
        raise StaleLibraryError(
            f"{LIB_PATH} was built from sources with digest {got}, but the sources here have digest {want}; "
            "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")


def build_digest():
    """The source digest compiled into the loaded library ("unstamped" for an A/B build of
    sources older than the stamp)."""
    lib = load()
    return lib.sr_build_digest().decode() if hasattr(lib, "sr_build_digest") else "unstamped"


def last_error():
    return load().sr_last_error().decode(errors="replace")


def table_encoding(words, key_bits, slots):
    """What the engine's table rules (csrc/kernels.hpp make_table_view, min_table_cap, filter_exact,
    filter_compact_ok) give a model of `words` words with a packed key of `key_bits` bits in a table
    of `slots` slots: dict(qbits, dbits, bbits, plimit, s32, filter (0 none, 1 8-byte entries,
    2 compact entries), filter_log2, min_cap_log2). Host-only."""
    out = (ctypes.c_uint32 * 8)()
    st = load().sr_table_encoding(words, key_bits, slots, out)
    if st != 0:
        raise ValueError(f"sr_table_encoding: {last_error()} (status {st})")
    return dict(zip(("qbits", "dbits", "bbits", "plimit", "s32", "filter", "filter_log2", "min_cap_log2"), out))


def sim_walk(model_id, params, seed, walk, max_depth=4096, nprops=32, loops=False):
    """Walk `walk` of the simulation checker on the host (csrc/sim.hpp; no device needed), as the device
    runs it: dict(steps, end (SIM_TERMINAL / SIM_DEPTH / SIM_FAULT), final_fp, actions (canonical ids),
    first_hit (per property: the step of the walk's hit, -1 = none), attempts (drawn slots whose next
    state was refused)). loops=True: with loop detection (end may be SIM_LOOP), and the dict gains
    loop_start: the index of the earlier state a walk that ended SIM_LOOP returned to, -1 otherwise."""
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    acts = (ctypes.c_int64 * max(1, max_depth))()
    end, att, start = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    fp = ctypes.c_uint64()
    hits = (ctypes.c_int32 * nprops)()
    if loops:
        n = lib.sr_sim_walk_loops(model_id, arr, len(params), seed, walk, max_depth, 1, acts, max_depth, ctypes.byref(end),
                                  ctypes.byref(fp), hits, nprops, ctypes.byref(att), ctypes.byref(start))
    else:
        n = lib.sr_sim_walk(model_id, arr, len(params), seed, walk, max_depth, acts, max_depth, ctypes.byref(end),
                            ctypes.byref(fp), hits, nprops, ctypes.byref(att))
    if n < 0:
        raise ValueError(f"sr_sim_walk: {last_error()} (status {n})")
    out = {"steps": n, "end": end.value, "final_fp": fp.value, "actions": list(acts[:n]), "first_hit": list(hits),
           "attempts": att.value}
    if loops:
        out["loop_start"] = start.value
    return out


def sim_unique_host(model_id, params, seed, walk0, nwalks, max_depth=4096, loops=False):
    """The distinct-state set of the simulation checker on the host (sr_sim_unique_host, csrc/sim.hpp;
    no device needed): the sorted distinct fingerprints of every state the walks walk0 .. walk0 +
    nwalks - 1 visit, as a numpy uint64 array; what `spawn_simulation(count_unique=True)` collects on
    the device."""
    import numpy as np
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    n = lib.sr_sim_unique_host(model_id, arr, len(params), seed, walk0, nwalks, max_depth, int(bool(loops)), None, 0)
    if n < 0:
        raise ValueError(f"sr_sim_unique_host: {last_error()} (status {n})")
    out = np.zeros(max(1, n), dtype=np.uint64)
    lib.sr_sim_unique_host(model_id, arr, len(params), seed, walk0, nwalks, max_depth, int(bool(loops)),
                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
    return out[:n]


def host_graph(model_id, params, max_states=1 << 22):
    """The reachable graph of a registered model by a host search (sr_host_graph; no device needed):
    (succ, inits, conds) with succ[i] = [(canonical action id, j)] in `actions()` order, inits the init
    states' numbers in order, and conds[i] the bit mask of the properties whose condition holds at i."""
    import numpy as np
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    n = lib.sr_host_graph(model_id, arr, len(params), max_states, None, 0)
    if n < 0:
        raise ValueError(f"sr_host_graph: {last_error()} (status {n})")
    buf = np.zeros(n, dtype=np.int64)
    lib.sr_host_graph(model_id, arr, len(params), max_states, buf.ctypes.data_as(_I64P), n)
    d = buf.tolist()
    states, k = d[0], d[1]
    inits, at = d[3:3 + k], 3 + k
    succ, conds = [], []
    for _ in range(states):
        conds.append(d[at])
        c = d[at + 1]
        succ.append(list(zip(d[at + 2:at + 2 + 2 * c:2], d[at + 3:at + 3 + 2 * c:2])))
        at += 2 + 2 * c
    return succ, inits, conds


COVER_MAX_CLASSES = 1024


def coverage_dict(res, names, enabled, taken, moved, prop_names, holds):
    """The dict both `coverage_host` and `GpuBfsChecker.coverage` return: the scalars of sr_coverage (ran,
    states, terminal, stutter_ends, max_out_degree, pass_ms and the counts `n_classes`, `nprops`), `classes`
    (a list of {name, enabled, taken, moved} in class order), `properties` ({name: holds}) and `out_degree`
    (64 buckets; the last holds 63 and more)."""
    out = res.as_dict()
    out["n_classes"] = out.pop("classes")
    out["classes"] = [{"name": n, "enabled": e, "taken": t, "moved": m} for n, e, t, m in zip(names, enabled, taken, moved)]
    out["properties"] = dict(zip(prop_names, holds))
    return out


def coverage_host(model_id, params, max_states=1 << 22, prop_names=None):
    """The coverage pass of a registered model on the host (sr_coverage_host, csrc/cover.hpp; no device
    needed): a host search over at most `max_states` states and the per-state rule the GPU pass applies.
    The dict of `coverage_dict`; the properties are keyed by `prop_names`, or by index without them."""
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    res = sr_coverage()
    res.struct_size = ctypes.sizeof(res)
    en, tk, mv = ((ctypes.c_uint64 * COVER_MAX_CLASSES)() for _ in range(3))
    holds = (ctypes.c_uint64 * 32)()
    names = ctypes.create_string_buffer(COVER_MAX_CLASSES * 256)
    n = lib.sr_coverage_host(model_id, arr, len(params), max_states, ctypes.byref(res), en, tk, mv, COVER_MAX_CLASSES, holds, 32,
                             names, len(names))
    if n < 0:
        raise ValueError(f"sr_coverage_host: {last_error()} (status {n})")
    c = res.classes
    keys = list(prop_names) if prop_names is not None else list(range(res.nprops))
    return coverage_dict(res, names.value.decode().split("\n")[:c], en[:c], tk[:c], mv[:c], keys, holds[:res.nprops])


def _liveness_host(name, call, stats=None):
    """Behind the liveness_host* functions: call(res, acts, cap) is the entry point `name`; the witness' buffer
    grows until it fits. The dict of sr_live_result plus `unique` and `actions`; stats = (key, struct) adds the
    mode's counters."""
    res = sr_live_result()
    cap = 1 << 16
    while True:
        acts = (ctypes.c_int64 * cap)()
        n = call(ctypes.byref(res), acts, cap)
        if n < 0:
            raise ValueError(f"{name}: {last_error()} (status {n})")
        if res.witness_len <= cap:
            break
        cap = res.witness_len
    out = res.as_dict()
    out["unique"] = n
    out["actions"] = list(acts[:max(0, res.witness_len)])
    if stats:
        out[stats[0]] = stats[1].as_dict()
    return out


def liveness_host(model_id, params, prop=0, max_states=1 << 22, fairness=0):
    """The complete `eventually` check of a registered model on the host (csrc/live.hpp; no device
    needed): a host search over at most `max_states` states, the fixpoint and the deterministic
    witness for the `eventually` property of index `prop`. The dict of sr_live_result, plus `unique`
    (the model's reachable states) and `actions` (the witness' canonical action ids; [] without one).
    fairness: 0 none, 1 progress fairness (a successor equal to its state is no successor)."""
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    return _liveness_host("sr_liveness_host", lambda res, acts, cap: lib.sr_liveness_host_fair(
        model_id, arr, len(params), prop, fairness, max_states, res, acts, cap))


def _liveness_host_fair(mode, stats, model_id, params, prop, max_states):
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    entry = getattr(lib, "sr_liveness_host_" + mode)
    return _liveness_host("sr_liveness_host_" + mode, lambda res, acts, cap: entry(
        model_id, arr, len(params), prop, max_states, res, ctypes.byref(stats), acts, cap), (mode, stats))


def liveness_host_weak(model_id, params, prop=0, max_states=1 << 22):
    """The complete `eventually` check under weak fairness on the host (csrc/live.hpp live_host_weak; no
    device needed): the dict of `liveness_host`, plus `weak`, the dict of sr_live_weak (cyclic_states,
    components, fair_components, goal_states, fair_states, stem_len, loop_len, ...). The witness'
    `actions` are the stem's followed by the closed walk's; ValueError (status -4) for a model whose
    slots are not fairness classes."""
    return _liveness_host_fair("weak", sr_live_weak(), model_id, params, prop, max_states)


def liveness_host_strong(model_id, params, prop=0, max_states=1 << 22):
    """The complete `eventually` check under strong fairness on the host (csrc/live.hpp live_host_strong; no
    device needed): the dict of `liveness_host`, plus `strong`, the dict of sr_live_strong (levels,
    cyclic_states, components, fair_components, goal_states, fair_states, stem_len, loop_len, ...). The
    witness' `actions` are the stem's followed by the closed walk's; ValueError (status -4) for a model whose
    slots are not fairness classes."""
    return _liveness_host_fair("strong", sr_live_strong(), model_id, params, prop, max_states)


LEADS_FAIRNESS = {"none": 0, "progress": 1, "weak": 2, "strong": 3}


def liveness_host_leads(model_id, params, prop, fairness=0, max_states=1 << 22):
    """The leads-to check of a registered model on the host (csrc/live.hpp LEADS-TO; no device needed) for the
    leads-to property of index `prop` in the mode `fairness` (0 / "none", 1 / "progress", 2 / "weak", 3 /
    "strong"): the dict of `liveness_host` over the whole witness (`actions`: the prefix' followed by the mode's
    own), plus `leads`, the dict of sr_live_leads (triggered, pending, violating, trigger_index, trigger_depth,
    seed_ms)."""
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    mode = LEADS_FAIRNESS.get(fairness, fairness)
    stats = sr_live_leads()
    return _liveness_host("sr_liveness_host_leads", lambda res, acts, cap: lib.sr_liveness_host_leads(
        model_id, arr, len(params), prop, mode, max_states, res, ctypes.byref(stats), acts, cap), ("leads", stats))


def step_host(model_id, params, prop, max_states=1 << 22, struct_size=None):
    """The step pass of a registered model on the host (sr_step_host, csrc/step.hpp; no device needed) for the
    step property of index `prop`: the dict of sr_step_result (ran, edges, violations, sources, step_index,
    step_action, init_index, witness_len, scan_ms, min_ms), plus `unique` (the model's reachable states) and
    `actions` (the witness' canonical action ids; [] without one). struct_size (tests): what the caller claims
    its struct to hold; the fields behind it keep what they had."""
    lib = load()
    params = list(params)
    arr = (ctypes.c_int64 * max(1, len(params)))(*params)
    cap = 1 << 12
    while True:
        res = sr_step_result()
        if struct_size is not None:
            ctypes.memset(ctypes.byref(res), 0xEE, ctypes.sizeof(res))
        res.struct_size = ctypes.sizeof(res) if struct_size is None else struct_size
        acts = (ctypes.c_int64 * cap)()
        n = lib.sr_step_host(model_id, arr, len(params), prop, max_states, ctypes.byref(res), acts, cap)
        if n < 0:
            raise ValueError(f"sr_step_host: {last_error()} (status {n})")
        if struct_size is not None or res.witness_len <= cap:
            break
        cap = res.witness_len
    out = res.as_dict()
    out["struct_size"] = res.struct_size
    out["unique"] = n
    out["actions"] = list(acts[:max(0, min(cap, res.witness_len))]) if struct_size is None else []
    return out


def runtime_versions():
    """{"hip": (runtime, compiled), "rccl": (runtime, compiled)} as the engine library sees them."""
    lib = load()
    out = {}
    for key, fn in (("hip", lib.sr_hip_runtime_version), ("rccl", lib.sr_rccl_version)):
        r, c = ctypes.c_int32(), ctypes.c_int32()
        out[key] = (r.value, c.value) if fn(ctypes.byref(r), ctypes.byref(c)) == 0 else (None, None)
    return out


def loaded_runtime_paths():
    """Paths of the HIP runtime and RCCL libraries mapped into this process (Linux)."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1] if line.count(" ") >= 5 else ""
                if "libamdhip64" in p or "librccl" in p:
                    paths.add(p)
    except OSError:
        pass
    return sorted(paths)
