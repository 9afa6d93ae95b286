"""Host-side mirror of Stateright's checker API over the MI355X engine.

Mirrors, name for name, the reference's `CheckerBuilder` (src/checker.rs:35-178), the `Checker`
trait (src/checker.rs:184-338) and `Path` (src/checker/path.rs), so that code written against
`model.checker().spawn_bfs().join()` reads the same. Every call goes through the C ABI in
include/stateright_gpu.h; there is no CPU fallback.
"""
import ctypes
import enum
import sys
import time

from . import _native as N


class Expectation(enum.IntEnum):
    """`Expectation` (src/lib.rs:293-300)."""
    Always = N.SR_ALWAYS
    Eventually = N.SR_EVENTUALLY
    Sometimes = N.SR_SOMETIMES
    LeadsTo = N.SR_LEADS_TO  # (no reference counterpart: "whenever the trigger holds, eventually the condition")
    LEADS_TO = N.SR_LEADS_TO  # (an alias, under the engine's own name for it)
    AlwaysStep = N.SR_ALWAYS_STEP  # (no reference counterpart: an invariant over steps, decided by the step pass)


class CheckerError(RuntimeError):
    """A failed engine call (the reference panics in these cases)."""

    def __init__(self, what, code=None):
        super().__init__(f"{what}: {N.last_error()}" + (f" (status {code})" if code is not None else ""))
        self.code = code


class Path:
    """`Path<State, Action>` (src/checker/path.rs:16): states with the action taken from each.

    States are the canonical integer descriptions shared with the CPU oracle; actions are their
    `Debug` text (e.g. "RmPrepare(3)"), with the canonical ids in `action_ids`.
    """

    def __init__(self, states, action_ids, action_names):
        self.states = [tuple(s) for s in states]
        self.action_ids = list(action_ids)
        self.action_names = list(action_names)

    def last_state(self):
        return self.states[-1]

    def into_states(self):
        return list(self.states)

    def into_actions(self):
        return list(self.action_names)

    def into_vec(self):
        acts = self.action_names + [None]
        return list(zip(self.states, acts))

    def __len__(self):
        return len(self.action_ids)

    def __str__(self):  # `impl Display for Path` (src/checker/path.rs:174-187)
        return f"Path[{len(self.action_ids)}]:\n" + "".join(f"- {a}\n" for a in self.action_names)

    def __repr__(self):
        return f"Path({self.action_names!r})"

    def __eq__(self, other):
        return isinstance(other, Path) and (self.states, self.action_ids) == (other.states, other.action_ids)

    def __hash__(self):
        return hash((tuple(self.states), tuple(self.action_ids)))


class StateRecorder:
    """`StateRecorder` visitor (src/checker/visitor.rs:70-99): records every visited state."""

    def __init__(self):
        self.states = []

    @classmethod
    def new_with_accessor(cls):
        r = cls()
        return r, (lambda: list(r.states))


class PathRecorder:
    """`PathRecorder` visitor (src/checker/visitor.rs:32-66): records the path to every visited
    state (as a set, like the reference's `HashSet<Path>`)."""

    def __init__(self):
        self.paths = set()

    @classmethod
    def new_with_accessor(cls):
        r = cls()
        return r, (lambda: set(r.paths))

    def visit(self, path):
        self.paths.add(path)


class CheckerBuilder:
    """`CheckerBuilder` (src/checker.rs:35-178) for a registered GpuModel."""

    def __init__(self, model):
        self._model = model
        self._opts = N.sr_opts()
        self._opts.struct_size = ctypes.sizeof(N.sr_opts)
        self._threads = 1
        self._visitor = None
        self._partitions = 1
        self._comm = None
        self._symmetry = False

    # --- options mirrored from the reference ---------------------------------------------------
    def threads(self, thread_count):
        """`threads` (src/checker.rs:170-172). The engine runs one host driver thread per GPU;
        the value is kept for API compatibility and does not change results."""
        self._threads = int(thread_count)
        return self

    def target_state_count(self, count):
        """`target_state_count` (src/checker.rs:164-166): stop at the first 1500-pop block
        boundary of the single-threaded reference order at which state_count >= count."""
        self._opts.target_state_count = int(count)
        return self

    def visitor(self, visitor):
        """`visitor` (src/checker.rs:175-177): a `StateRecorder`, a `PathRecorder`, or any callable
        taking a `Path` (`impl Fn(Path)`, src/checker/visitor.rs:23-30). The GPU explores a whole
        level per launch, so the visits are exported in bulk after the run and handed to the
        visitor in visit order (the reference's order in FIFO mode); a visitor cannot steer the
        search in the reference either."""
        if not (isinstance(visitor, (StateRecorder, PathRecorder)) or callable(visitor)):
            raise TypeError("visitor must be a StateRecorder, a PathRecorder or a callable taking a Path")
        self._visitor = visitor
        self._opts.record_visits = 1
        return self

    def symmetry(self):
        """`symmetry` (src/checker.rs:145-160). The BFS checker ignores it, as the reference's does
        (src/checker/bfs.rs:36-74 never reads options.symmetry); `spawn_dfs` rejects it (see there)."""
        self._symmetry = True
        return self

    def symmetry_canonical(self):
        """Engine opt-in: canonical symmetry reduction. Visited states, frontier and BFS tree hold one
        representative per orbit (2pc: RMs sorted by their full (rm_state, tm_prepared, Prepared msg)
        tuple), so `unique_state_count` is the number of reachable orbits, the same in every visit
        order; discovery paths are concrete paths of the original model. This is deliberately NOT the
        reference's `symmetry().spawn_dfs()` count (665 for 2pc N=5), whose representatives sort by
        rm_state alone and make the count depend on the DFS order (src/checker/dfs.rs:258-283)."""
        self._opts.symmetry = 1
        return self

    # --- engine-specific options ---------------------------------------------------------------
    def order(self, order):
        """"auto" (default), "fifo" (exact reference visit order) or "fast"."""
        self._opts.order = {"auto": N.SR_ORDER_AUTO, "fifo": N.SR_ORDER_FIFO, "fast": N.SR_ORDER_FAST}[order]
        return self

    def capacity_hint(self, unique_states):
        self._opts.capacity_hint = int(unique_states)
        return self

    def device(self, ordinal):
        self._opts.device = int(ordinal)
        return self

    def partitions(self, n):
        """Partition the visited set into `n` virtual partitions on one GPU (the multi-GPU protocol
        with a device-copy exchange; FAST order)."""
        self._partitions = int(n)
        return self

    def comm(self, communicator):
        """Partition the search over the GPUs of a `stateright_amd.distributed.Communicator`
        (one process per GPU, RCCL all-to-all per level; FAST order)."""
        self._comm = communicator
        return self

    def defer_paths(self, on=True):
        """Partitioned search: skip gathering the discovery paths at join (they are then built on
        demand, collectively: every rank must ask for the same property in the same order)."""
        self._opts.defer_paths = int(bool(on))
        return self

    def counters(self, on=True):
        """Count visited-set probes and CAS claims (stats()["probes"], ["cas"]) with a counting
        variant of the expand kernel (slower; for measurement passes only)."""
        self._opts.counters = int(bool(on))
        return self

    def profile(self, on=True):
        self._opts.profile = int(bool(on))
        return self

    def complete_liveness(self, on=True, fairness=None):
        """Engine opt-in: the complete `eventually` check. `spawn_bfs`, like the
        reference, refutes an `eventually` property only at a terminal state reached with the
        property's bit still set, so it misses a counterexample through a state that was first reached
        on a path where the property held, and every counterexample that runs round a cycle
        (src/checker.rs:400-413). With this on, a search that explored everything is followed by a
        backward fixpoint over the reachable set on the GPU: a property without a discovery then holds
        on every maximal path, and a discovery made by the pass is a terminal path or a lasso
        (`GpuBfsChecker.loop_start`, `liveness`), which `assert_discovery` then accepts. No fairness is
        assumed (a self-loop on a state where the property does not hold refutes it), the witness is
        not the shortest one, and `target_state_count`, partitions / comm, `symmetry_canonical` and
        plugin models are refused at spawn. Off by default; with it off nothing changes.

        `fairness="progress"` (progress fairness): a successor equal to its state is no successor, so
        an action that changes nothing (2pc's RmRcvCommitMsg at a Committed rm) is no step. A state is
        then a sink if it is terminal or a stutter end (it has successors, all of them itself); the
        witness never steps from a state to itself and ends at a terminal state, at a stutter end
        (`liveness(name)["end_kind"] == 3`) or by closing a loop of at least two distinct states. No
        discovery then means: the property holds on every maximal path that does not stay forever
        in one state that has a successor other than itself. It is NOT per-action weak fairness: a
        cycle through two or more distinct states still refutes the property. The same refusals
        apply; the simulation checker's `detect_loops` is unaffected (a self-loop closes a lasso
        there). Any other `fairness` but None raises ValueError."""
        if fairness is not None and fairness != "progress":
            raise ValueError(f'complete_liveness: fairness must be None or "progress", not {fairness!r}')
        self._opts.liveness = 0 if not on else N.SR_LIVENESS_PROGRESS if fairness == "progress" else N.SR_LIVENESS_COMPLETE
        return self

    def weak_fairness(self, on=True):
        """Engine opt-in: the complete `eventually` check under WEAK FAIRNESS per action slot (DESIGN.md
        section 12). Like `complete_liveness(fairness="progress")`, and further: a cycle refutes an
        `eventually` property only if a run round it can be fair to every slot, where a slot that is
        moving-enabled (enabled, and its step changes the state) at every state of the cycle must be
        taken by it. So a clock that can always tick no longer refutes everything. A discovery made by
        the pass ends at a terminal state or a stutter end, or is a lasso whose loop is weakly fair
        (`liveness(name)["weak"]` has the figures; `assert_discovery` accepts a lasso only if the host
        model finds its loop weakly fair). No discovery means: the property holds on every maximal run
        that is weakly fair to every slot. Only models whose slots are actions take it (DGraph,
        LiveGraph, TwoPhaseSys / TwoPhaseLiveSys, SpinLockSys); the others, and whatever
        `complete_liveness` refuses, are refused at spawn. Not strong fairness. `on=False` turns the
        complete check off."""
        self._opts.liveness = N.SR_LIVENESS_WEAK if on else 0
        return self

    def strong_fairness(self, on=True):
        """Engine opt-in: the complete `eventually` check under STRONG FAIRNESS per action slot (DESIGN.md
        section 12). Like `weak_fairness()`, and further: a slot that is moving-enabled again and again
        must be taken again and again, also where it is disabled in between (a thread's acquire while
        another thread holds the lock), so a starvation loop no longer refutes "every client is
        eventually served". A cycle refutes an `eventually` property only if some strongly connected
        set of its states takes, inside the set, every slot that a member moves on; such sets may lie
        inside components that are not fair, so the components are decomposed level by level
        (`liveness(name)["strong"]` has the figures: levels, components, fair_components, ...; there is
        no "weak" key in this mode). A discovery made by the pass ends at a terminal state or a stutter
        end, or is a lasso whose loop is strongly fair; `assert_discovery` accepts a lasso only if the
        host model finds its loop strongly fair. No discovery means: the property holds on every
        maximal run that is strongly fair to every slot, which subsumes weak fairness. The same models
        take it as `weak_fairness()`, with the same refusals; one GPU, the witness is not the shortest,
        and the number of levels is reported, not bounded. `on=False` turns the complete check off."""
        self._opts.liveness = N.SR_LIVENESS_STRONG if on else 0
        return self

    def certify(self, on=True):
        """Engine opt-in: the certificate pass. Behind a `spawn_bfs` / `spawn_dfs` on one
        GPU, kernels that share nothing with the search but the model and the table's lookup re-derive from
        the arena, the parent ranks and the final visited set that the arena starts with the init states, that
        every state has a parent in the level before it that produces it, that the arena is closed under
        successors with none listed late, and in FIFO order that the visit order is the reference's:
        `GpuBfsChecker.certificate()`. The search launches what it launches without the option. A
        partitioned spawn leaves the certificate's `ran` at 0."""
        self._opts.certify = int(bool(on))
        return self

    def coverage(self, on=True):
        """Engine opt-in: the coverage pass. A `spawn_bfs` / `spawn_dfs` on one GPU
        that explored everything is followed by one more expansion of every reachable state on the GPU,
        which counts per action class how often it was enabled, taken (its next state exists and is
        within the boundary) and moved (that state differs), per property the states where its condition
        holds, and the terminal states, stutter ends and out-degrees: `GpuBfsChecker.coverage()`,
        `coverage_report()`, `assert_covered()`. An action that is never taken, or a condition that holds
        nowhere or everywhere, is how an `always` property comes to hold vacuously. The search itself is
        unchanged. `target_state_count`, partitions / comm and `symmetry_canonical` are refused at spawn;
        plugin models take it; `spawn_simulation` ignores it. Off by default; with it off nothing changes."""
        self._opts.coverage = int(bool(on))
        return self

    def verbose(self, on=True):
        self._opts.verbose = int(bool(on))
        return self

    # --- spawn ---------------------------------------------------------------------------------
    def spawn_bfs(self):
        """`spawn_bfs` (src/checker.rs:124-129): non-blocking; call `join()`."""
        if self._comm is not None or self._partitions > 1:
            # (a visitor's record is gathered from every partition at join, collectively: every
            # rank of a communicator passes a visitor)
            return GpuBfsChecker(self._model, self._opts, self._visitor, comm=self._comm, partitions=self._partitions)
        return GpuBfsChecker(self._model, self._opts, self._visitor)

    spawn_gpu_bfs = spawn_bfs

    def spawn_dfs(self):
        """`spawn_dfs` (src/checker.rs:131-136, src/checker/dfs.rs) on the GPU engine.

        A check that runs to completion (no early exit) visits the same reachable set whatever the
        traversal, so `unique_state_count`, `state_count`, `is_done` and the set of discovered
        properties equal the reference DFS's; the engine explores level by level (FAST order) and
        its discovery paths are BFS-tree paths (valid, and shortest). When every property gets
        discovered, the reference stops at an order-dependent point of its depth-first order, and
        the counts then differ. `symmetry()` is refused: the reference's representatives
        (e.g. examples/2pc.rs:164-182) are not canonical forms, so the reduced count depends on the
        DFS visit order itself (2pc N=5: 665 in DFS order, tests/test_oracle_dfs.py), which a
        level-synchronous search cannot reproduce."""
        if self._symmetry:
            raise NotImplementedError(
                "symmetry().spawn_dfs(): the symmetry-reduced count depends on the reference's "
                "depth-first visit order (non-canonical representatives); not reproducible on the GPU. "
                "symmetry_canonical() gives an order-independent reduction (one state per orbit)")
        self._opts.order = N.SR_ORDER_FAST
        return self.spawn_bfs()

    def spawn_simulation(self, seed, walks=None, max_depth=4096, record_walks=False, detect_loops=False,
                         count_unique=False, unique_capacity=None, until_stale=None):
        """The simulation checker (Stateright's `spawn_simulation`, added after the 0.28 mirrored here):
        `walks` independent random traces of at most `max_depth` steps from the init states, one GPU
        lane per trace, the properties evaluated on every state. No visited set is kept, so a model
        too large for `spawn_bfs` still gets discoveries; a run without a discovery proves nothing.

        detect_loops=True (off by default; with it off nothing changes) also ends a trace where it
        returns to a state it has visited (end reason 4): such a trace is a lasso, a prefix and a cycle
        that can repeat forever, so an `eventually` property that held nowhere on it is discovered
        without a terminal state, which neither the plain traces nor `spawn_bfs` can report. Cycles of
        at most 8 states are found at their first closure, longer ones once the trace returns to a
        checkpoint taken at a power-of-two step; the discovery's path ends at the state it repeats
        (`GpuSimulationChecker.loop_start`). No fairness is assumed.

        count_unique=True (off by default; with it off nothing changes) also collects the fingerprints
        of every state the traces visit in a table on the GPU: `unique_state_count()` is then the number
        of DISTINCT states visited (`unique_fingerprints()`, `batch_new_states()`, `unique_info()`), a
        measure of how much ground the traces covered and whether more of them still reach anything
        new. It is a coverage measure, not a proof: states no trace reached are simply not in it. The
        traces, records, hits and the stop point are the same with it on or off. The table is sized
        for `unique_capacity` distinct states (default min(walks * (max_depth + 1), 2**28)); past it
        the count is a lower bound (`unique_info()["overflow"]`). until_stale=k also stops the check
        after the first whole batch that ends k consecutive batches without a new state; it needs
        count_unique, stands in for `walks` as the check's bound, and an overflow then fails the check.

        Trace w is a pure function of (model, seed, w, max_depth, detect_loops) (csrc/sim.hpp), and the check stops
        after the first whole batch of traces at whose end every property is discovered,
        `target_state_count` is reached or `walks` traces have run. walks=None needs a
        `target_state_count` or `until_stale` (a property may never be discovered). Honours `device`,
        `target_state_count`, `verbose` and `profile`; a visitor, partitions / comm,
        `symmetry_canonical` and plugin models are refused. Non-blocking; call `join()`."""
        if self._visitor is not None:
            raise ValueError("spawn_simulation: a visitor has nothing to visit (the walks keep no visit record)")
        if self._comm is not None or self._partitions > 1:
            raise ValueError("spawn_simulation: the simulation checker is not partitioned (no partitions / comm)")
        if self._opts.symmetry:
            raise ValueError("spawn_simulation: symmetry_canonical has no counterpart (there is no visited set to reduce)")
        if getattr(self._model, "plugin", None) is not None:
            raise ValueError("spawn_simulation: plugin models are not simulated (registered models only)")
        if not 1 <= int(max_depth) <= 2**20:
            raise ValueError("spawn_simulation: max_depth must be in 1..=2**20")
        if until_stale is not None and int(until_stale) < 1:
            raise ValueError("spawn_simulation: until_stale must be positive")
        if until_stale is not None and not count_unique:
            raise ValueError("spawn_simulation: until_stale needs count_unique=True (it counts batches without a new distinct state)")
        if unique_capacity is not None and not 1 <= int(unique_capacity) <= 2**30:
            raise ValueError("spawn_simulation: unique_capacity must be in 1..=2**30")
        if walks is None and not self._opts.target_state_count and until_stale is None:
            raise ValueError("spawn_simulation: give walks or a target_state_count (a property may never be discovered)")
        so = N.sr_sim_opts()
        N.load().sr_sim_opts_init_sized(ctypes.byref(so), ctypes.sizeof(so))
        so.device = self._opts.device
        so.seed = int(seed)
        so.walks = 0 if walks is None else int(walks)
        so.max_depth = int(max_depth)
        so.record_walks = int(bool(record_walks))
        so.target_state_count = self._opts.target_state_count
        so.verbose = self._opts.verbose
        so.profile = self._opts.profile
        so.loops = int(bool(detect_loops))
        so.unique = int(bool(count_unique))
        so.stale_batches = 0 if until_stale is None else int(until_stale)
        so.unique_capacity = 0 if unique_capacity is None else int(unique_capacity)
        if walks is not None and so.walks == 0:
            raise ValueError("spawn_simulation: walks must be positive")
        return GpuSimulationChecker(self._model, so)

    def serve(self, address=("127.0.0.1", 3000), block=True):
        """`serve` (src/checker.rs:107-113, src/checker/explorer.rs:71-129): spawns the GPU check and
        serves the Explorer's JSON routes (`/.status`, `/.states/<fp>/<fp>/...`) and a small UI over
        it. Blocks like the reference unless block=False, which returns the running
        `stateright_amd.explorer.Explorer` (its `.checker`, `.url`, `.shutdown()`)."""
        from .explorer import Explorer
        ex = Explorer(self.spawn_bfs(), address)
        if not block:
            return ex.start()
        try:
            ex.serve_forever()
        finally:
            ex.shutdown()
        return ex.checker


class GpuBfsChecker:
    """The `Checker` trait (src/checker.rs:184-338) implemented by the MI355X engine."""

    PATH_BUFFER = 65536  # states the first buffers of discovery() / discovery_fingerprints() hold (they regrow)

    def __init__(self, model, opts, visitor=None, comm=None, partitions=1):
        lib = N.load()
        self._lib = lib
        self._model = model
        self._visitor = visitor
        self._comm = comm
        params = list(model.params())
        arr = (ctypes.c_int64 * max(1, len(params)))(*params)
        plugin = getattr(model, "plugin", None)
        if plugin is not None:  # a GpuModel compiled into its own library (stateright_amd.plugin)
            if comm is not None or partitions > 1:
                self._h = lib.sr_gpu_bfs_spawn_plugin_partitioned(plugin.handle, comm.handle if comm is not None else None,
                                                                  partitions, arr, len(params), ctypes.byref(opts))
            else:
                self._h = lib.sr_gpu_bfs_spawn_plugin(plugin.handle, arr, len(params), ctypes.byref(opts))
        elif comm is not None or partitions > 1:
            self._h = lib.sr_gpu_bfs_spawn_partitioned(comm.handle if comm is not None else None, partitions,
                                                       model.MODEL_ID, arr, len(params), ctypes.byref(opts))
        else:
            self._h = lib.sr_gpu_bfs_spawn(model.MODEL_ID, arr, len(params), ctypes.byref(opts))
        self._liveness = bool(opts.liveness)
        self._weak = opts.liveness == N.SR_LIVENESS_WEAK
        self._strong = opts.liveness == N.SR_LIVENESS_STRONG
        self._progress = opts.liveness == N.SR_LIVENESS_PROGRESS or self._weak or self._strong  # (both subsume it)
        self._spawned("sr_gpu_bfs_spawn")

    def _spawned(self, what):
        """The state every checker keeps once its spawn call has returned the handle `self._h`."""
        if not self._h:
            raise CheckerError(what)
        self._joined = False
        self._props = None
        self._names = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.sr_gpu_bfs_free(h)
            self._h = None

    # --- Checker trait -------------------------------------------------------------------------
    def model(self):
        return self._model

    def state_count(self):
        return self._lib.sr_gpu_bfs_state_count(self._h)

    def unique_state_count(self):
        return self._lib.sr_gpu_bfs_unique_state_count(self._h)

    def max_depth(self):
        return self._lib.sr_gpu_bfs_max_depth(self._h)

    def join(self):
        if not self._joined:
            st = self._lib.sr_gpu_bfs_join(self._h)
            self._joined = True
            if st != 0:
                raise CheckerError("sr_gpu_bfs_join", st)
            if isinstance(self._visitor, StateRecorder):
                self._visitor.states.extend(self.visits())
            elif self._visitor is not None:
                visit = self._visitor.visit if isinstance(self._visitor, PathRecorder) else self._visitor
                for path in self.visit_paths():
                    visit(path)
        return self

    def is_done(self):
        return bool(self._lib.sr_gpu_bfs_is_done(self._h))

    def properties(self):
        if self._props is None:
            out = []
            buf = ctypes.create_string_buffer(256)
            exp = ctypes.c_int32()
            for i in range(self._lib.sr_gpu_bfs_property_count(self._h)):
                self._lib.sr_gpu_bfs_property(self._h, i, buf, 256, ctypes.byref(exp))
                out.append((buf.value.decode(), Expectation(exp.value)))
            self._props = out
        return self._props

    def _prop_index(self, name):
        for i, (n, _) in enumerate(self.properties()):
            if n == name:
                return i
        raise KeyError(f"Unknown property. requested={name}, available={[n for n, _ in self.properties()]}")

    def action_name(self, action_id):
        if action_id not in self._names:
            buf = ctypes.create_string_buffer(256)
            self._lib.sr_gpu_bfs_action_name(self._h, action_id, buf, 256)
            self._names[action_id] = buf.value.decode()
        return self._names[action_id]

    def action_id(self, action):
        if isinstance(action, int):
            return action
        for i in range(self._lib.sr_gpu_bfs_action_id_bound(self._h)):
            if self.action_name(i) == action:
                return i
        raise KeyError(f"unknown action {action!r}")

    def discovery_fingerprints(self, name):
        """The fingerprint chain init..discovery (`reconstruct_path` input, bfs.rs:314-342)."""
        i = self._prop_index(name)
        cap = self.PATH_BUFFER
        while True:  # (a witness of the liveness pass may be longer than the first buffer)
            buf = (ctypes.c_uint64 * cap)()
            n = self._lib.sr_gpu_bfs_discovery(self._h, i, buf, cap)
            if n < 0:
                raise CheckerError("sr_gpu_bfs_discovery", n)
            if n <= cap:
                return list(buf[:n])
            cap = n

    def discovery(self, name):
        """`discovery` (src/checker.rs:211-213): the Path for `name`, or None."""
        i = self._prop_index(name)
        width = self._lib.sr_gpu_bfs_describe_width(self._h)
        cap = self.PATH_BUFFER
        while True:  # (a witness of the liveness pass may be longer than the first buffers)
            acts = (ctypes.c_int64 * cap)()
            states = (ctypes.c_int64 * (cap * max(1, width)))()
            n = self._lib.sr_gpu_bfs_discovery_path(self._h, i, acts, cap, states, cap * max(1, width))
            if n == -1:
                return None
            if n < 0:
                raise CheckerError("sr_gpu_bfs_discovery_path", n)
            if n < cap:
                break
            cap = n + 1
        flat = list(states[:(n + 1) * width])
        st = [tuple(flat[k:k + width]) for k in range(0, len(flat), width)]
        ids = list(acts[:n])
        return Path(st, ids, [self.action_name(a) for a in ids])

    def discoveries(self):
        """`discoveries` (src/checker/bfs.rs:289-298): property name -> Path."""
        out = {}
        for name, _ in self.properties():
            p = self.discovery(name)
            if p is not None:
                out[name] = p
        return out

    def visits(self):
        width = self._lib.sr_gpu_bfs_describe_width(self._h)
        n = self._lib.sr_gpu_bfs_visits(self._h, None, 0)
        buf = (ctypes.c_int64 * max(1, n))()
        self._lib.sr_gpu_bfs_visits(self._h, buf, n)
        flat = list(buf[:n])
        return [tuple(flat[k:k + width]) for k in range(0, n, width)]

    def explore(self, fingerprints):
        """Explorer's `states` view (src/checker/explorer.rs:159-240): [(action name or None, state
        description or None, fingerprint or None)] of the init states (no fingerprints) or of the
        steps following the state the fingerprint path leads to; None if no state follows."""
        n = len(fingerprints)
        fps = (ctypes.c_uint64 * max(1, n))(*fingerprints)
        width = self._lib.sr_gpu_bfs_describe_width(self._h)
        cap = 64
        while True:  # re-called with room for every view when the first buffer is too small
            acts = (ctypes.c_int64 * cap)()
            has = (ctypes.c_int32 * cap)()
            fpo = (ctypes.c_uint64 * cap)()
            st = (ctypes.c_int64 * (cap * max(1, width)))()
            v = self._lib.sr_gpu_bfs_explore(self._h, fps, n, acts, has, fpo, st, cap)
            if v == -1:
                return None
            if v < 0:
                raise CheckerError("sr_gpu_bfs_explore", v)
            if v <= cap:
                break
            cap = v
        out = []
        for i in range(v):
            name = None if acts[i] < 0 else self.action_name(acts[i])
            if has[i]:
                out.append((name, tuple(st[i * width:(i + 1) * width]), fpo[i]))
            else:
                out.append((name, None, None))
        return out

    def visit_paths(self):
        """The path to every visited state, in visit order (what the reference hands to its
        visitor at each pop, src/checker/bfs.rs:187-189)."""
        n = self._lib.sr_gpu_bfs_visit_tree(self._h, None, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_bfs_visit_tree", n)
        parent = (ctypes.c_int64 * max(1, n))()
        action = (ctypes.c_int64 * max(1, n))()
        self._lib.sr_gpu_bfs_visit_tree(self._h, parent, action, n)
        states = self.visits()
        out = []
        for i in range(n):
            chain = []
            j = i
            while j >= 0:
                chain.append(j)
                j = parent[j]
            chain.reverse()
            ids = [action[k] for k in chain[1:]]
            out.append(Path([states[k] for k in chain], ids, [self.action_name(a) for a in ids]))
        return out

    def stats(self):
        s = N.sr_stats()
        self._lib.sr_gpu_bfs_stats_sized(self._h, ctypes.byref(s), ctypes.sizeof(s))
        return s.as_dict()

    def table_audit(self):
        """The visited-set audit of a check run with `counters()` (csrc/kernels_audit.hpp), a dict of
        sr_table_audit: ran, fifo, slots, occupied, misplaced, duplicates, arena_states, arena_missing,
        arena_shared, meta_wrong. Clean: the last five but arena_states are 0 and, for a check that
        explored everything, occupied == arena_states == unique_state_count() (after an early exit
        only occupied >= arena_states). ran is 0 without `counters()`."""
        a = N.sr_table_audit()
        st = self._lib.sr_gpu_bfs_table_audit(self._h, ctypes.byref(a), ctypes.sizeof(a))
        if st < 0:
            raise CheckerError("sr_gpu_bfs_table_audit", st)
        return a.as_dict()

    def certificate(self):
        """The certificate pass' figures (`CheckerBuilder.certify()`; joins the check), a dict of sr_certificate:
        ran, fifo, explored_all, skipped, states, levels, inits, repeated_inits, the error counters roots_wrong,
        map_missing, tree_range, tree_edge, tree_slot, closure_missing, closure_unlisted, closure_late,
        fifo_not_first and fifo_order (all 0 when clean), edges and repeated_edges (inits + edges +
        repeated_edges == state_count() when explored_all), pmask, and per property (lists in property order)
        holds, first_index, disc_index, disc_wrong, first_level and disc_level; all ones (2^64 - 1) stands for "none". ran is 0 without
        the option, and after a partitioned spawn."""
        self.join()
        c = N.sr_certificate()
        st = self._lib.sr_gpu_bfs_certificate(self._h, ctypes.byref(c), ctypes.sizeof(c))
        if st < 0:
            raise CheckerError("sr_gpu_bfs_certificate", st)
        return c.as_dict()

    def liveness(self, name):
        """The complete `eventually` check's outcome for property `name` (`complete_liveness()`), a dict:
        ran (0: the option is off, `name` is no `eventually` property, the search itself discovered it,
        or the search did not explore everything), not_p_states (reachable states where the condition
        does not hold), surviving (those from which a path exists on which it never holds), rounds (an
        implementation detail), examined, witness_len (steps; -1 without a witness), loop_start (-1:
        none, or a witness that closes no loop), end_kind (0 no witness, 1 it ends at a terminal state,
        2 it closes a loop, 3 it ends at a stutter end: progress fairness only), init_index (-1: the
        property holds) and pass_ms. A check under `weak_fairness()` adds "weak": the dict of sr_live_weak
        (cyclic_states, components, fair_components, goal_states, fair_states, stem_len, loop_len, and the
        round counters, which are implementation details); `surviving` is then |F_p'|, and `loop_start`
        the state the last state repeats (the closed walk may pass it more than once). A check under
        `strong_fairness()` adds "strong" instead: the dict of sr_live_strong (levels, the depth of the
        decomposition tree, components, all its nodes, fair_components, its fair nodes, and the rest as
        for "weak"). For a leads-to property the pass adds "leads": the dict of sr_live_leads (triggered, pending,
        violating: the reachable states where the trigger holds, those of them where the condition does not, and
        those of them from which a (fair) run exists on which it never does; trigger_index = trigger_depth: the
        seed's index on the witness, -1 without one; seed_ms); `witness_len`, `loop_start` and `init_index` are then
        over the whole path, prefix included, and a fair mode's `stem_len` counts from the seed."""
        r = N.sr_live_result()
        st = self._lib.sr_gpu_bfs_liveness(self._h, self._prop_index(name), ctypes.byref(r))
        if st != 0:
            raise CheckerError("sr_gpu_bfs_liveness", st)
        out = r.as_dict()
        ld = N.sr_live_leads()
        st = self._lib.sr_gpu_bfs_liveness_leads(self._h, self._prop_index(name), ctypes.byref(ld))
        if st != 0:
            raise CheckerError("sr_gpu_bfs_liveness_leads", st)
        if ld.ran:
            out["leads"] = ld.as_dict()
        for mode, stats in (("weak", N.sr_live_weak), ("strong", N.sr_live_strong)):
            if getattr(self, "_" + mode, False) and r.ran:
                s = stats()
                st = getattr(self._lib, "sr_gpu_bfs_liveness_" + mode)(self._h, self._prop_index(name), ctypes.byref(s))
                if st != 0:
                    raise CheckerError("sr_gpu_bfs_liveness_" + mode, st)
                if s.ran:
                    out[mode] = s.as_dict()
        return out

    def coverage(self):
        """The coverage pass' figures (`CheckerBuilder.coverage()`; joins the check), a dict: states (the
        distinct reachable states: `unique_state_count()`), terminal (states where no action yields a
        state), stutter_ends (states whose every successor is the state itself), max_out_degree, out_degree
        (states by number of successors, 64 buckets, the last for 63 and more), pass_ms, n_classes, nprops,
        `classes`: a list of {name, enabled, taken, moved} per action class (enabled: listed by `actions`;
        taken: with a next state within the boundary; moved: with one that differs from the state), and
        `properties`: {name: states where the property's condition holds}. Raises CheckerError if the
        option was off or the search did not explore everything (it stopped with every property
        discovered)."""
        self.join()
        res = N.sr_coverage()
        res.struct_size = ctypes.sizeof(res)
        st = self._lib.sr_gpu_bfs_coverage(self._h, ctypes.byref(res))
        if st != 0 or not res.ran:
            raise CheckerError("sr_gpu_bfs_coverage", st if st != 0 else None)
        c = res.classes
        en, tk, mv = ((ctypes.c_uint64 * max(1, c))() for _ in range(3))
        self._lib.sr_gpu_bfs_coverage_classes(self._h, en, tk, mv, c)
        holds = (ctypes.c_uint64 * max(1, res.nprops))()
        self._lib.sr_gpu_bfs_coverage_props(self._h, holds, res.nprops)
        names = []
        buf = ctypes.create_string_buffer(256)
        for i in range(c):
            self._lib.sr_gpu_bfs_coverage_class_name(self._h, i, buf, 256)
            names.append(buf.value.decode())
        return N.coverage_dict(res, names, en[:c], tk[:c], mv[:c], [n for n, _ in self.properties()], holds[:res.nprops])

    def coverage_report(self, w=None):
        """Prints the coverage table: one line per action class, then the properties and the state figures."""
        w = w or sys.stdout
        cov = self.coverage()
        width = max([len("action class")] + [len(c["name"]) for c in cov["classes"]])
        w.write(f"Coverage. states={cov['states']}, terminal={cov['terminal']}, stutter_ends={cov['stutter_ends']}, "
                f"max_out_degree={cov['max_out_degree']}\n")
        w.write(f"{'action class':<{width}}  {'enabled':>14}  {'taken':>14}  {'moved':>14}\n")
        for c in cov["classes"]:
            mark = "" if c["taken"] else "  <- never taken"
            w.write(f"{c['name']:<{width}}  {c['enabled']:>14}  {c['taken']:>14}  {c['moved']:>14}{mark}\n")
        for (name, exp), holds in zip(self.properties(), cov["properties"].values()):
            mark = "  <- holds nowhere" if holds == 0 else "  <- holds everywhere" if holds == cov["states"] else ""
            w.write(f'{exp.name.lower()} "{name}": condition holds at {holds} of {cov["states"]} states{mark}\n')
        return self

    def assert_covered(self, allow=()):
        """Raises AssertionError naming every action class that was never taken (`taken == 0`) and is not
        in `allow` (class names)."""
        allow = set(allow)
        missing = [c["name"] for c in self.coverage()["classes"] if c["taken"] == 0 and c["name"] not in allow]
        if missing:
            raise AssertionError(f"action classes never taken: {missing}")
        return self

    def loop_start(self, name):
        """`complete_liveness()`: if the discovery of the `eventually` property `name` is a lasso found
        by the pass, the index of the path's state that its last state repeats; None otherwise."""
        r = self.liveness(name)
        return r["loop_start"] if r["ran"] and r["witness_len"] >= 0 and r["loop_start"] >= 0 else None

    def trigger_index(self, name):
        """`complete_liveness()`: if the leads-to property `name` has a discovery, the index of the path's state
        at which its trigger holds and from which on its condition never does (the length of the prefix); None
        otherwise."""
        ld = self._leads_info(name)
        return ld["trigger_index"] if ld and ld["trigger_index"] >= 0 else None

    def _leads_info(self, name):
        """The "leads" dict of `liveness(name)`, or None if the pass did not decide the leads-to property `name`
        (nothing else does)."""
        return self.liveness(name).get("leads")

    def _leads_checked(self, name):
        return bool(self._leads_info(name))

    def step(self, name):
        """The step pass' figures for the step property `name` (joins the check), a dict:
        edges (the edges of the reachable graph: pairs of a state and an enabled action with a next state within
        the boundary), violations (the edges on which the property does not hold), sources (the states with such
        an edge), step_index (the index of the violating step on the discovery = the depth of its source; -1
        without one), step_action (its canonical action id), init_index, witness_len, scan_ms, min_ms. None when
        the property was NOT CHECKED: `name` is no step property, or the check was partitioned, ran under
        symmetry or with a target_state_count, was a simulation, or did not explore everything."""
        self.join()
        res = N.sr_step_result()
        res.struct_size = ctypes.sizeof(res)
        st = self._lib.sr_gpu_bfs_step(self._h, self._prop_index(name), ctypes.byref(res))
        if st != 0:
            raise CheckerError("sr_gpu_bfs_step", st)
        return res.as_dict() if res.ran else None

    def step_index(self, name):
        """If the step property `name` has a discovery, the index of the path's step that violates it (its last:
        the path has step_index + 1 actions); None otherwise."""
        s = self.step(name)
        return s["step_index"] if s and s["step_index"] >= 0 else None

    def _step_checked(self, name):
        return self.step(name) is not None

    def _last_step_holds(self, name, actions, init):
        """The host model's answer for the last step of the path (sr_gpu_bfs_replay_step): True / False, or None
        if the actions cannot be replayed from init state `init`."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        r = self._lib.sr_gpu_bfs_replay_step(self._h, init, arr, len(ids), self._prop_index(name))
        return None if r < 0 else bool(r)

    def launch_profile(self):
        """profile(): [(kernel_ms, frontier)] of every expand launch, in launch order."""
        n = self._lib.sr_gpu_bfs_launch_profile(self._h, None, None, 0)
        ms = (ctypes.c_double * max(1, n))()
        fr = (ctypes.c_uint64 * max(1, n))()
        self._lib.sr_gpu_bfs_launch_profile(self._h, ms, fr, n)
        return [(ms[i], fr[i]) for i in range(n)]

    def launch_counters(self):
        """[(probes, cas)] of every expand launch (builder.counters(); zeros otherwise)."""
        n = self._lib.sr_gpu_bfs_launch_counters(self._h, None, None, 0)
        pr = (ctypes.c_uint64 * max(1, n))()
        cs = (ctypes.c_uint64 * max(1, n))()
        self._lib.sr_gpu_bfs_launch_counters(self._h, pr, cs, n)
        return [(pr[i], cs[i]) for i in range(n)]

    # --- report / asserts (src/checker.rs:216-337) ---------------------------------------------
    def discovery_classification(self, name):
        exp = dict(self.properties())[name]
        return "example" if exp == Expectation.Sometimes else "counterexample"

    def report(self, w=None):
        w = w or sys.stdout
        start = time.monotonic()
        # `report` polls once per second while checking (src/checker.rs:223-228).
        while not self._joined and not self.is_done():
            w.write(f"Checking. states={self.state_count()}, unique={self.unique_state_count()}\n")
            for _ in range(100):
                if not self._lib.sr_gpu_bfs_is_running(self._h):
                    break
                time.sleep(0.01)
            if not self._lib.sr_gpu_bfs_is_running(self._h):
                break
        self.join()
        w.write(f"Done. states={self.state_count()}, unique={self.unique_state_count()}, "
                f"sec={int(time.monotonic() - start)}\n")
        found = self.discoveries()
        for name, path in found.items():
            w.write(f'Discovered "{name}" {self.discovery_classification(name)} {path}')
        for name, exp in self.properties():  # a leads-to property without a discovery: what the pass found
            if exp != Expectation.LeadsTo or name in found:
                continue
            ld = self._leads_info(name)
            if not ld:
                w.write(f'Leads-to "{name}": not checked\n')
            elif ld["triggered"]:
                w.write(f'Leads-to "{name}": holds (triggered {ld["triggered"]} states)\n')
            else:
                w.write(f'Leads-to "{name}": holds vacuously (never triggered)\n')
        for name, exp in self.properties():  # a step property without a discovery: what the step pass found
            if exp != Expectation.AlwaysStep or name in found:
                continue
            s = self.step(name)
            w.write(f'Step "{name}": holds ({s["edges"]} edges)\n' if s else f'Step "{name}": not checked\n')
        return self

    def assert_properties(self):
        for name, exp in self.properties():
            if exp == Expectation.Sometimes:
                self.assert_any_discovery(name)
            else:
                self.assert_no_discovery(name)

    def assert_any_discovery(self, name):
        found = self.discovery(name)
        if found is not None:
            return found
        assert self.is_done(), f'Discovery for "{name}" not found, but model checking is incomplete.'
        raise AssertionError(f'Discovery for "{name}" not found.')

    def assert_no_discovery(self, name):
        found = self.discovery(name)
        if found is not None:
            raise AssertionError(f'Unexpected "{name}" {self.discovery_classification(name)} {found}'
                                 f"Last state: {found.last_state()}\n")
        assert self.is_done(), f'Discovery for "{name}" not found, but model checking is incomplete.'
        if dict(self.properties())[name] == Expectation.LeadsTo and not self._leads_checked(name):
            raise AssertionError(f'Leads-to property "{name}" was not checked (it takes complete_liveness(), '
                                 "weak_fairness() or strong_fairness(), and a search that explored everything).")
        if dict(self.properties())[name] == Expectation.AlwaysStep and not self._step_checked(name):
            raise AssertionError(f'Step property "{name}" was not checked (the step pass takes a spawn_bfs / spawn_dfs on '
                                 "one GPU without symmetry or target_state_count, and a search that explored everything).")

    def replay(self, actions, init_index=0):
        """`Path::from_actions` on the host copy of the model: (states, conditions) or None."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        width = self._lib.sr_gpu_bfs_describe_width(self._h)
        states = (ctypes.c_int64 * ((len(ids) + 1) * width))()
        conds = (ctypes.c_int32 * 64)()
        n = self._lib.sr_gpu_bfs_replay(self._h, init_index, arr, len(ids), states, (len(ids) + 1) * width, conds, 64)
        if n < 0:
            return None
        flat = list(states)
        return [tuple(flat[k:k + width]) for k in range(0, len(flat), width)], list(conds[:len(self.properties())])

    def replay_trace(self, actions, init_index=0):
        """`Path::from_actions`: (per-state conditions [[cond of property p] per state], last state
        terminal?) or None if an action is not enabled along the way."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        n_props = len(self.properties())
        conds = (ctypes.c_int32 * max(1, (len(ids) + 1) * n_props))()
        term = ctypes.c_int32()
        n = self._lib.sr_gpu_bfs_replay_trace(self._h, init_index, arr, len(ids), conds, len(conds), ctypes.byref(term))
        if n < 0:
            return None
        flat = list(conds)
        return [flat[k * n_props:(k + 1) * n_props] for k in range(len(ids) + 1)], bool(term.value)

    def _accepts_lassos(self):
        """Whether this check can report a lasso for an `eventually` property (`complete_liveness()`)."""
        return self._liveness

    def _accepts_stutter_ends(self):
        """Whether this check ran under progress fairness (`complete_liveness(fairness="progress")`)."""
        return getattr(self, "_progress", False)

    def _loop_is_fair(self, actions, init, loop_start, strong=False):
        """The host model's answer for the loop of a lasso (sr_gpu_bfs_loop_fair): True iff it is weakly fair;
        strong: iff it is strongly fair (sr_gpu_bfs_loop_strongly_fair)."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        ask = self._lib.sr_gpu_bfs_loop_strongly_fair if strong else self._lib.sr_gpu_bfs_loop_fair
        return ask(self._h, init, arr, len(ids), loop_start) == 1

    def _sink_kind(self, actions, init):
        """The host model's answer for the state the actions lead to from init state `init`: 0 it has a
        successor other than itself, 1 terminal, 3 a stutter end (-1: no such path)."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        return self._lib.sr_gpu_bfs_sink_kind(self._h, init, arr, len(ids))

    def _replay_triggers(self, name, actions, init):
        """The leads-to property's trigger on every state of the path (sr_gpu_bfs_replay_triggers), or None."""
        ids = [self.action_id(a) for a in actions]
        arr = (ctypes.c_int64 * max(1, len(ids)))(*ids)
        out = (ctypes.c_int32 * (len(ids) + 1))()
        n = self._lib.sr_gpu_bfs_replay_triggers(self._h, init, arr, len(ids), self._prop_index(name), out, len(ids) + 1)
        return None if n < 0 else [bool(x) for x in out[:n]]

    def _assert_leads_discovery(self, name, actions, found, trigger_index, loop_start):
        """assert_discovery for a leads-to property: from some init state the actions lead, at some index t (the
        given trigger_index, else any), to a state where the trigger holds; the condition holds on no state from t
        on; and the path ends as the check's mode allows: at a terminal state, under a fairness mode at a stutter
        end, or at a state equal to the one at some index j (the given loop_start, else any) with t <= j < the
        last index, where under weak / strong fairness the loop from j must be fair."""
        i = self._prop_index(name)
        info = []
        for init in range(self._lib.sr_gpu_bfs_init_count(self._h)):
            r = self.replay_trace(actions, init)
            trig = self._replay_triggers(name, actions, init) if r is not None else None
            if r is None or trig is None:
                continue
            per_state, terminal = r
            states, _ = self.replay(actions, init)
            last = len(states) - 1
            starts = range(last + 1) if trigger_index is None else [trigger_index]
            for t in starts:
                if not 0 <= t <= last or not trig[t]:
                    info.append(f"the trigger does not hold at index {t}")
                    continue
                if any(s[i] for s in per_state[t:]):
                    info.append(f"the condition holds from index {t} on")
                    continue
                if loop_start is None and (terminal or (self._accepts_stutter_ends() and self._sink_kind(actions, init) == N.SR_LIVE_END_STUTTER)):
                    return
                for j in (range(t, last) if loop_start is None else [loop_start]):
                    if not t <= j < last:
                        info.append(f"loop_start {j} is not in [{t}, {last})")
                    elif states[j] != states[last]:
                        continue
                    elif self._weak and not self._loop_is_fair(actions, init, j):
                        info.append("the loop is not weakly fair")
                    elif self._strong and not self._loop_is_fair(actions, init, j, strong=True):
                        info.append("the loop is not strongly fair")
                    else:
                        return
                info.append(f"from index {t} the path neither ends at a sink nor closes a loop")
        extra = f" ({'; '.join(sorted(set(info)))})" if info else ""
        raise AssertionError(f'Invalid discovery for "{name}"{extra}, but a valid one was found. found={found.into_actions()}')

    def assert_discovery(self, name, actions, trigger_index=None, loop_start=None):
        """`assert_discovery` (src/checker.rs:292-337): the actions, from some init state, lead to a
        state violating an `always` / satisfying a `sometimes` property, or along a path on which
        an `eventually` property never holds and that ends at a terminal state. Only a check that can
        report lassos (`complete_liveness()`; the simulation checker's `detect_loops=True`) also accepts,
        for an `eventually` property, a path that ends at a state equal to an earlier state of the
        path: the cycle between them can repeat forever. A check under progress fairness also accepts,
        for an `eventually` property, a path that ends at a stutter end (a state with successors that
        all are the state itself), decided on the host model. A check under weak fairness accepts stutter
        ends likewise, and a lasso only if its loop is weakly fair on the host model; a check under strong
        fairness likewise, and a lasso only if its loop is strongly fair there. A leads-to property takes a path
        by the rule of `_assert_leads_discovery`; trigger_index and loop_start (that kind of property only) pin
        the two indices instead of leaving them to be found."""
        found = self.assert_any_discovery(name)
        i = self._prop_index(name)
        exp = self.properties()[i][1]
        if exp == Expectation.LeadsTo:
            return self._assert_leads_discovery(name, actions, found, trigger_index, loop_start)
        if exp == Expectation.AlwaysStep:  # any replayable path whose last step violates the property
            held = [self._last_step_holds(name, actions, init) for init in range(self._lib.sr_gpu_bfs_init_count(self._h))]
            if False in held:
                return
            why = "its last step does not violate the property" if True in held else "its actions cannot be replayed, or it has no step"
            raise AssertionError(f'Invalid discovery for "{name}" ({why}), but a valid one was found. found={found.into_actions()}')
        loops = exp == Expectation.Eventually and self._accepts_lassos()
        info = []
        for init in range(self._lib.sr_gpu_bfs_init_count(self._h)):
            r = self.replay_trace(actions, init)
            if r is None:
                continue
            per_state, terminal = r
            last = per_state[-1][i]
            if exp == Expectation.Always and not last:
                return
            if exp == Expectation.Sometimes and last:
                return
            if exp == Expectation.Eventually:
                satisfied = any(s[i] for s in per_state)
                closed = False
                if loops:
                    states, _ = self.replay(actions, init)
                    closed = states[-1] in states[:-1]
                    for mode, how in (("_weak", "weakly"), ("_strong", "strongly")):  # (only a loop that is fair so refutes)
                        if closed and getattr(self, mode, False):
                            closed = self._loop_is_fair(actions, init, states.index(states[-1]), strong=mode == "_strong")
                            if not closed:
                                info.append(f"incorrect counterexample closes a loop that is not {how} fair")
                if not terminal and not closed and self._accepts_stutter_ends():
                    closed = self._sink_kind(actions, init) == N.SR_LIVE_END_STUTTER
                if not satisfied and (terminal or closed):
                    return
                if satisfied:
                    info.append("incorrect counterexample satisfies eventually property")
                if not (terminal or closed):
                    info.append("incorrect counterexample is nonterminal" + (" and closes no loop" if loops else ""))
        extra = f" ({'; '.join(info)})" if info else ""
        raise AssertionError(f'Invalid discovery for "{name}"{extra}, but a valid one was found. '
                             f"found={found.into_actions()}")


class GpuSimulationChecker(GpuBfsChecker):
    """The `Checker` trait over the simulation checker (`CheckerBuilder.spawn_simulation`). `report`,
    `assert_*`, `discoveries`, `discovery` and `replay` are inherited unchanged, with these meanings:
    `state_count` is the number of states the walks visited, `unique_state_count` EQUALS it (there is
    no visited set: repeats count) unless the check ran with `count_unique=True` (then it is the
    number of distinct states visited, a lower bound if `unique_info()["overflow"]`; see
    `unique_info`, `unique_fingerprints`, `batch_new_states`), `max_depth` is the longest walk in
    steps, and `is_done` means "every property discovered", so `assert_no_discovery` /
    `assert_properties` of a property that is never violated report that model checking is
    incomplete: a run without a discovery proves nothing.
    With `detect_loops=True` the discovery of an `eventually` property may be a lasso (`loop_start`),
    which `assert_discovery` then accepts."""

    def __init__(self, model, sim_opts):
        lib = N.load()
        self._lib = lib
        self._model = model
        self._visitor = None
        self._comm = None
        self._sim_opts = sim_opts
        self._params = list(model.params())
        arr = (ctypes.c_int64 * max(1, len(self._params)))(*self._params)
        self._h = lib.sr_gpu_sim_spawn(model.MODEL_ID, arr, len(self._params), ctypes.byref(sim_opts))
        self._spawned("sr_gpu_sim_spawn")

    def walk_records(self):
        """record_walks=True: [(steps, end reason, fingerprint of the last state)] per walk, by walk
        index (end reason: 1 terminal, 2 depth, 3 fault, 4 loop)."""
        n = self._lib.sr_gpu_sim_walk_records(self._h, None, None, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_sim_walk_records", n)
        steps = (ctypes.c_uint32 * max(1, n))()
        end = (ctypes.c_uint32 * max(1, n))()
        fp = (ctypes.c_uint64 * max(1, n))()
        self._lib.sr_gpu_sim_walk_records(self._h, steps, end, fp, n)
        return list(zip(steps[:n], end[:n], fp[:n]))

    def walk_records_arrays(self):
        """walk_records as three numpy arrays (steps, end reason, fingerprint)."""
        import numpy as np
        n = self._lib.sr_gpu_sim_walk_records(self._h, None, None, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_sim_walk_records", n)
        steps = np.zeros(max(1, n), dtype=np.uint32)
        end = np.zeros(max(1, n), dtype=np.uint32)
        fp = np.zeros(max(1, n), dtype=np.uint64)
        self._lib.sr_gpu_sim_walk_records(self._h, steps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                          end.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                          fp.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
        return steps[:n], end[:n], fp[:n]

    def hit(self, name):
        """The discovery of property `name` as (step, walk index): the hit of the fewest steps, ties
        to the lowest walk index; None without a discovery."""
        walk, step = ctypes.c_uint64(), ctypes.c_uint32()
        if not self._lib.sr_gpu_sim_hit(self._h, self._prop_index(name), ctypes.byref(walk), ctypes.byref(step)):
            return None
        return step.value, walk.value

    def host_walk(self, i):
        """Walk `i` of this check re-walked on the host (`_native.sim_walk`), in this check's mode."""
        return N.sim_walk(self._model.MODEL_ID, self._params, self._sim_opts.seed, i, self._sim_opts.max_depth,
                          max(1, len(self.properties())), loops=bool(self._sim_opts.loops))

    def walk_loop_starts(self):
        """record_walks=True: per walk, by walk index, its loop start as a numpy int64 array: the index
        of the earlier state a walk that ended with reason 4 returned to, -1 for every other walk."""
        import numpy as np
        n = self._lib.sr_gpu_sim_walk_loop_starts(self._h, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_sim_walk_loop_starts", n)
        start = np.zeros(max(1, n), dtype=np.uint32)
        self._lib.sr_gpu_sim_walk_loop_starts(self._h, start.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n)
        out = start[:n].astype(np.int64)
        out[out == 0xFFFFFFFF] = -1
        return out

    def loop_start(self, name):
        """detect_loops=True: if the discovery of the `eventually` property `name` is a lasso, the index
        of the path's state that its last state repeats; None otherwise (no discovery, another kind
        of property, or a path that ends at a terminal state)."""
        h = self.hit(name)
        if h is None or not self._sim_opts.loops or self.properties()[self._prop_index(name)][1] != Expectation.Eventually:
            return None
        step, walk = h
        w = self.host_walk(walk)
        return w["loop_start"] if w["end"] == N.SIM_LOOP and w["steps"] == step else None

    def _accepts_lassos(self):
        """detect_loops=True: `assert_discovery` (the base class's) accepts a lasso for an `eventually`
        property."""
        return bool(self._sim_opts.loops)

    def unique_info(self):
        """The distinct-state count of a joined check: dict(on, unique, overflow (an insert was dropped:
        `unique` is a lower bound), stopped_stale (the check stopped by until_stale), slots, capacity
        (the table's geometry), batches). With count_unique off every entry but `batches` is 0."""
        self.join()
        res = N.sr_sim_unique_result()
        res.struct_size = ctypes.sizeof(res)
        st = self._lib.sr_gpu_sim_unique(self._h, ctypes.byref(res))
        if st != 0:
            raise CheckerError("sr_gpu_sim_unique", st)
        return res.as_dict()

    def unique_fingerprints(self):
        """count_unique=True: the fingerprints of the distinct states visited, sorted ascending, as a
        numpy uint64 array (compare with `_native.sim_unique_host`, or with `model_fingerprint` of
        the states another checker visited)."""
        import numpy as np
        self.join()
        n = self._lib.sr_gpu_sim_unique_fingerprints(self._h, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_sim_unique_fingerprints", n)
        out = np.zeros(max(1, n), dtype=np.uint64)
        self._lib.sr_gpu_sim_unique_fingerprints(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
        return out[:n]

    def batch_new_states(self):
        """count_unique=True: per batch, in order, how many distinct states it added (their sum is
        `unique_state_count()`): how coverage grew, and whether it still does. [] with the mode off."""
        self.join()
        n = self._lib.sr_gpu_sim_batch_new(self._h, None, 0)
        if n < 0:
            raise CheckerError("sr_gpu_sim_batch_new", n)
        out = (ctypes.c_uint64 * max(1, n))()
        self._lib.sr_gpu_sim_batch_new(self._h, out, n)
        return list(out[:n])

    def liveness(self, name):
        raise NotImplementedError("liveness: the simulation checker keeps no reachable set (complete_liveness is spawn_bfs's)")

    def _leads_info(self, name):
        return None  # (a walk decides no leads-to property)
