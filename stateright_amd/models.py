"""Registered GpuModels (include/stateright_gpu.h SR_MODEL_*), named after the reference models.

Each class carries the reference model's parameters and returns a `CheckerBuilder` from
`checker()`, like `Model::checker` (src/lib.rs:231-236).
"""
from . import _native as N
from .checker import CheckerBuilder


class _Model:
    MODEL_ID = 0

    def params(self):
        return []

    def checker(self):
        return CheckerBuilder(self)


class LinearEquation(_Model):
    """`LinearEquation { a, b, c }` (src/test_util.rs:140-188): find x, y with a*x + b*y == c in u8."""
    MODEL_ID = N.SR_MODEL_LINEAR_EQUATION

    def __init__(self, a, b, c):
        self.a, self.b, self.c = a, b, c

    def params(self):
        return [self.a, self.b, self.c]


class BinaryClock(_Model):
    """`BinaryClock` (src/test_util.rs:4-45)."""
    MODEL_ID = N.SR_MODEL_BINARY_CLOCK


class TwoPhaseSys(_Model):
    """`TwoPhaseSys { rms: 0..rm_count }` (examples/2pc.rs:10-121)."""
    MODEL_ID = N.SR_MODEL_2PC

    def __init__(self, rm_count):
        self.rm_count = rm_count

    def params(self):
        return [self.rm_count]


class TwoPhaseLiveSys(_Model):
    """`TwoPhaseSys` with two `eventually` properties after its three (csrc/models.hpp `TwoPhaseLive`; no
    reference counterpart): "every RM decides" (every rm Committed or Aborted) and "every RM commits".
    States, actions and counts are 2pc's. 2pc has no terminal state (RmRcvCommitMsg / RmRcvAbortMsg stay
    enabled as self-loops), so only `complete_liveness(fairness="progress")` says anything about them."""
    MODEL_ID = N.SR_MODEL_2PC_LIVE

    def __init__(self, rm_count):
        self.rm_count = rm_count

    def params(self):
        return [self.rm_count]


class SpinLockSys(_Model):
    """`threads` threads take a lock in turn while a clock ticks (csrc/models.hpp `SpinLock`; no reference
    counterpart), 1 <= threads <= 20: Acquire(i) while the lock is free, Release(i) by its holder (which
    serves thread i), and Tick, always enabled. Two `eventually` properties: "some thread served", which
    the Tick cycle refutes unless the check runs under `weak_fairness()`, and "every thread served", which
    a starvation lasso refutes even then (it would take strong fairness)."""
    MODEL_ID = N.SR_MODEL_SPIN_LOCK

    def __init__(self, threads):
        if not 1 <= threads <= 20:
            raise ValueError("SpinLockSys: threads must be in 1..=20")
        self.threads = threads

    def params(self):
        return [self.threads]


class FairRings(_Model):
    """Nested rings (csrc/models.hpp `FairRings`; no reference counterpart): the fixture of
    `strong_fairness()`. Lane j < lanes has the rings 0 .. d_j, d_j = 1 + (j mod d), of w positions each;
    Step walks round a ring, Out(k) leaves ring k at position 0 (ring 0 for the lane's terminal `done`
    state), In(k) enters ring k + 1 at position 1. A lane whose core is on (core == 1, or core == 2 and j
    odd) can also take Out(d_j) at position 2 of its innermost ring and stay there. One `eventually`
    property "done": `weak_fairness()` refutes it in every lane; under `strong_fairness()` it holds iff
    core == 0, and the fair set of a core lane lies d_j levels deep inside components that are not fair.
    1 <= d <= 28, 4 <= w <= 64, core in (0, 1, 2), 1 <= lanes <= 512."""
    MODEL_ID = N.SR_MODEL_FAIR_RINGS

    def __init__(self, d, w, core, lanes):
        if not (1 <= d <= 28 and 4 <= w <= 64 and core in (0, 1, 2) and 1 <= lanes <= 512):
            raise ValueError("FairRings: d in 1..=28, w in 4..=64, core in (0, 1, 2), lanes in 1..=512")
        self.d, self.w, self.core, self.lanes = d, w, core, lanes

    def params(self):
        return [self.d, self.w, self.core, self.lanes]


class Increment(_Model):
    """`increment` example `State::new(n)` (examples/increment.rs:109-197)."""
    MODEL_ID = N.SR_MODEL_INCREMENT

    def __init__(self, thread_count):
        self.thread_count = thread_count

    def params(self):
        return [self.thread_count]


class IncrementLock(_Model):
    """`increment_lock` example `State::new(n)` (examples/increment_lock.rs:3-107)."""
    MODEL_ID = N.SR_MODEL_INCREMENT_LOCK

    def __init__(self, thread_count):
        self.thread_count = thread_count

    def params(self):
        return [self.thread_count]


class Paxos(_Model):
    """The paxos example: `PaxosModelCfg { client_count, server_count: 3, network }` with an
    unordered non-duplicating network (examples/paxos.rs:223-263), checked through ActorModel
    (src/actor/model.rs:176-327) with a linearizability history (src/actor/register.rs:37-87).

    Action ids are canonical envelope codes (oracle/paxos.hpp `envelope_code`), so a path is
    comparable with the CPU oracle's. client_count 1..6 (the reference's bench.sh checks 6); the
    linearizability history is kept in the state and checked on the device (csrc/paxos.hpp)."""
    MODEL_ID = N.SR_MODEL_PAXOS

    def __init__(self, client_count=2, server_count=3):
        if server_count != 3:
            raise ValueError("the paxos encoding is compiled for server_count = 3 (examples/paxos.rs:275)")
        self.client_count = client_count
        self.server_count = server_count

    def params(self):
        return [self.client_count]

    KINDS = ("Prepare", "Prepared", "Accept", "Accepted", "Decided", "Put", "Get", "PutOk", "GetOk")

    @staticmethod
    def deliver(src, dst, kind, *fields):
        """Action id of `Deliver { src, dst, msg }` (src/actor/model.rs:18-24) in the canonical
        envelope code (oracle/paxos.hpp `envelope_code`). `fields` follow the reference message:
        Put(req, value), Get(req), PutOk(req), GetOk(req, value), Prepare(ballot),
        Prepared(ballot, last_accepted), Accept(ballot, proposal), Accepted(ballot),
        Decided(ballot, proposal); ballot = (round, id), proposal = (req, requester, value),
        last_accepted = None or (ballot, proposal)."""
        k = Paxos.KINDS.index(kind)

        def bal(b):
            return b[0] * 8 + b[1]

        def acc(a):
            return 0 if a is None else 1 + a[0][0] * 64 + a[0][1] * 8 + a[1][1]

        def ch(v):
            return ord(v) if isinstance(v, str) else int(v)

        if kind in ("Prepare", "Accepted"):
            f = bal(fields[0])
        elif kind == "Prepared":
            f = bal(fields[0]) * 4096 + acc(fields[1])
        elif kind in ("Accept", "Decided"):
            f = bal(fields[0]) * 16 + fields[1][1]
        elif kind in ("Put", "Get", "PutOk"):
            f = fields[0]
        else:
            f = fields[0] * 256 + ch(fields[1])
        return (((f * 16) + k) * 16 + dst) * 16 + src


class DGraph(_Model):
    """The reference's `DGraph` test fixture (src/test_util.rs:47-116): a directed graph over u8
    states built from paths, with one property "odd" (s % 2 == 1) of the given expectation — the
    model the reference checks `eventually` properties with (src/checker.rs:349-414)."""
    MODEL_ID = N.SR_MODEL_DGRAPH

    def __init__(self, expectation=N.SR_EVENTUALLY, paths=()):
        self.expectation = int(expectation)
        self.paths = [list(p) for p in paths]

    @classmethod
    def with_property(cls, expectation):
        return cls(expectation)

    def with_path(self, path):
        """`DGraph::with_path`: adds path[0] to the init states and the path's edges."""
        return DGraph(self.expectation, self.paths + [list(path)])

    def params(self):
        p = [self.expectation]
        for path in self.paths:
            p.append(len(path))
            p.extend(path)
        return p


class PingPong(_Model):
    """The reference's ping-pong actor fixture `PingPongCfg { max_nat, maintains_history }
    .into_model()` (src/actor/actor_test_util.rs:4-96) with `.lossy_network(..)` and
    `.duplicating_network(..)` (src/actor/model.rs:52-66; the reference defaults to a lossless
    duplicating network). Action ids: Deliver = envelope code * 4 + 1, Drop = code * 4 + 2
    (stateright_amd/csrc/actor.hpp). `max_nat` <= 7 runs on a 16-slot network encoding, 8..=14 on a
    32-slot one (its states describe 32 envelopes instead of 16)."""
    MODEL_ID = N.SR_MODEL_PINGPONG

    def __init__(self, max_nat, maintains_history=False, lossy=False, duplicating=True):
        self.max_nat, self.maintains_history = max_nat, maintains_history
        self.lossy, self.duplicating = lossy, duplicating

    def lossy_network(self, on=True):
        return PingPong(self.max_nat, self.maintains_history, on, self.duplicating)

    def duplicating_network(self, on=True):
        return PingPong(self.max_nat, self.maintains_history, self.lossy, on)

    def params(self):
        return [self.max_nat, int(self.lossy), int(self.duplicating), int(self.maintains_history)]


class ActorFixture(_Model):
    """The reference's one-actor fixtures (src/actor/model.rs:697-733): kind 0 =
    `handles_undeliverable_messages` (an init envelope to Id 99), kind 1 = `resets_timer`."""
    MODEL_ID = N.SR_MODEL_ACTOR_FIXTURE

    def __init__(self, kind):
        self.kind = kind

    def params(self):
        return [self.kind]


class Ladder(_Model):
    """Test fixture without a reference counterpart (csrc/models.hpp `Ladder`): `rungs` steps climbed
    in order and `free_bits` bits set in any order, one action slot each, so the slot count can pass
    64; (rungs + 1) * 2**free_bits states."""
    MODEL_ID = N.SR_MODEL_LADDER

    def __init__(self, rungs, free_bits):
        self.rungs, self.free_bits = rungs, free_bits

    def params(self):
        return [self.rungs, self.free_bits]


class Spread(_Model):
    """Test fixture without a reference counterpart (csrc/models.hpp `Spread`): the subsets of
    `free_bits` bits, packed with pseudo-random filler into a key of `key_bits` bits on `words` (1, 2
    or 4) words, so the key width, and with it the visited set's slot encoding, is a parameter.
    2**free_bits states, depth free_bits; `loops` (<= 4) further slots return the state itself without
    the model reporting them as self-loops; `sometimes "marked"` holds at the subset `mark`. The init
    states are the subsets 0 .. roots-1 in that order, then 0 .. dup-1 once more (duplicates)."""
    MODEL_ID = N.SR_MODEL_SPREAD

    def __init__(self, words, key_bits, free_bits, loops=0, mark=0, roots=1, dup=0):
        self.words, self.key_bits, self.free_bits, self.loops, self.mark = words, key_bits, free_bits, loops, mark
        self.roots, self.dup = roots, dup

    def params(self):
        p = [self.words, self.key_bits, self.free_bits, self.loops, self.mark]
        return p if (self.roots, self.dup) == (1, 0) else p + [self.roots, self.dup]


class LiveGraph(_Model):
    """Test fixture without a reference counterpart (csrc/models.hpp `LiveGraph`): a pseudo-random
    graph with cycles over the states v < 2**n_bits, out-degree `degree` (1..4), for the complete
    `eventually` check. r(v, k) = fmix64((fmix64(seed ^ v) + k) mod 2**64); v is terminal iff t_mod > 0
    and r(v, degree) % t_mod == 0, else slot k leads to r(v, k) mod 2**n_bits; `eventually "marked"`
    holds at v iff p_mod > 0 and r(v, degree + 1) % p_mod == 0; the init states are 0 .. roots-1."""
    MODEL_ID = N.SR_MODEL_LIVE_GRAPH

    def __init__(self, n_bits, degree, seed, p_mod, t_mod=0, roots=1, words=1, dup=0):
        self.n_bits, self.degree, self.seed, self.p_mod, self.t_mod, self.roots = n_bits, degree, seed, p_mod, t_mod, roots
        self.words = words  # 2 or 4: the same graph on states padded with words that are functions of v
        self.dup = dup      # the init states 0 .. dup-1 once more after the roots (duplicates)

    def params(self):
        p = [self.n_bits, self.degree, self.seed, self.p_mod, self.t_mod, self.roots]
        if self.dup:
            return p + [self.words, self.dup]
        return p if self.words == 1 else p + [self.words]


class LeadsGraph(_Model):
    """`LiveGraph`'s graph with the leads-to properties of the complete check (csrc/models.hpp `LeadsGraph`;
    no reference counterpart): 0 `eventually "marked"` as there; 1 leads-to "armed ~> marked", whose trigger
    holds at v iff q_mod > 0 and r(v, degree + 2) % q_mod == 0; 2 leads-to "always eventually marked", whose
    trigger is true."""
    MODEL_ID = N.SR_MODEL_LEADS_GRAPH

    def __init__(self, n_bits, degree, seed, p_mod, t_mod, roots, q_mod, words=1, dup=0):
        self.n_bits, self.degree, self.seed, self.p_mod, self.t_mod, self.roots = n_bits, degree, seed, p_mod, t_mod, roots
        self.q_mod, self.words, self.dup = q_mod, words, dup

    def params(self):
        p = [self.n_bits, self.degree, self.seed, self.p_mod, self.t_mod, self.roots, self.q_mod]
        if self.dup:
            return p + [self.words, self.dup]
        return p if self.words == 1 else p + [self.words]


class ReqLock(_Model):
    """A lock whose `threads` threads (1..8) first have to ask for it, while a clock ticks (csrc/models.hpp
    `ReqLockT`; no reference counterpart): Request(i), Acquire(i) while the lock is free and i waits,
    Release(i) by its holder, and Tick, always enabled. Property p < threads is the leads-to property
    "thread p waiting ~> thread p holds": refuted with no fairness and under progress fairness by the clock's
    cycle, under `weak_fairness()` for two or more threads by starvation, proved under `strong_fairness()`.
    Property `threads` is `eventually "some thread holds"`."""
    MODEL_ID = N.SR_MODEL_REQ_LOCK

    def __init__(self, threads):
        if not 1 <= threads <= 8:
            raise ValueError("ReqLock: threads must be in 1..=8")
        self.threads = threads

    def params(self):
        return [self.threads]


class LeadsDGraph(_Model):
    """`DGraph`'s adjacency from paths with an explicit list of trigger nodes (csrc/dgraph.hpp `LeadsDGraph`),
    for hand-drawn graphs of at most 256 states: one leads-to property "trigger ~> odd"."""
    MODEL_ID = N.SR_MODEL_LEADS_DGRAPH

    def __init__(self, triggers=(), paths=()):
        self.triggers = list(triggers)
        self.paths = [list(p) for p in paths]

    def with_path(self, path):
        return LeadsDGraph(self.triggers, self.paths + [list(path)])

    def params(self):
        p = [len(self.triggers)] + self.triggers
        for path in self.paths:
            p.append(len(path))
            p.extend(path)
        return p


class StepGraph(_Model):
    """`LiveGraph`'s graph with two step properties and no other (csrc/models.hpp `StepGraph`; no reference
    counterpart), the fixture of the step pass: 0 "no forbidden step", where the step (v, slot k) is forbidden
    iff f_mod > 0 and r(v, degree + 3 + k) % f_mod == 0; 1 "never down", violated iff the successor is below v."""
    MODEL_ID = N.SR_MODEL_STEP_GRAPH

    def __init__(self, n_bits, degree, seed, f_mod, t_mod=0, roots=1, words=1, dup=0):
        self.n_bits, self.degree, self.seed, self.f_mod, self.t_mod, self.roots = n_bits, degree, seed, f_mod, t_mod, roots
        self.words, self.dup = words, dup

    def params(self):
        p = [self.n_bits, self.degree, self.seed, self.f_mod, self.t_mod, self.roots]
        if self.dup:
            return p + [self.words, self.dup]
        return p if self.words == 1 else p + [self.words]


class StepDGraph(_Model):
    """`DGraph`'s adjacency from paths with an explicit list of forbidden (src, dst) pairs, at most 16
    (csrc/dgraph.hpp `StepDGraph`), for hand-drawn graphs of at most 256 states: one step property "no forbidden
    step". A pair that is no edge of the graph forbids nothing."""
    MODEL_ID = N.SR_MODEL_STEP_DGRAPH

    def __init__(self, forbidden=(), paths=()):
        self.forbidden = [tuple(f) for f in forbidden]
        self.paths = [list(p) for p in paths]

    def with_path(self, path):
        return StepDGraph(self.forbidden, self.paths + [list(path)])

    def params(self):
        p = [len(self.forbidden)]
        for src, dst in self.forbidden:
            p.extend((src, dst))
        for path in self.paths:
            p.append(len(path))
            p.extend(path)
        return p


class TwoPhaseStepSys(_Model):
    """`TwoPhaseSys` with two step properties after its three (csrc/models.hpp `TwoPhaseStep`; no reference
    counterpart): "a decided RM stays decided" (holds) and "the TM never aborts once an RM is prepared" (refuted
    by RmPrepare, TmAbort). States, actions and counts are 2pc's; only the step pass decides the two."""
    MODEL_ID = N.SR_MODEL_2PC_STEP

    def __init__(self, rm_count):
        self.rm_count = rm_count

    def params(self):
        return [self.rm_count]


class SingleCopyRegister(_Model):
    """The single-copy register `SingleCopyModelCfg { client_count, server_count }.into_model()`
    (examples/single-copy-register.rs:40-78): SingleCopyActor servers (a register value each, no
    consensus), RegisterActor clients, a non-duplicating network and a linearizability history.
    Its `check` CLI uses one server (linearizable); two or more are not linearizable."""
    MODEL_ID = N.SR_MODEL_SINGLE_COPY

    def __init__(self, client_count=2, server_count=1):
        self.client_count, self.server_count = client_count, server_count

    def params(self):
        return [self.client_count, self.server_count]


class AbdRegister(_Model):
    """The ABD linearizable register `AbdModelCfg { client_count, server_count }.into_model()`
    (examples/linearizable-register.rs:192-229): AbdActor servers, RegisterActor clients, a
    non-duplicating network and a linearizability history.

    Limits: `client_count` in 1..=6, `server_count` in 1..=4, at most 8 actors. The network of
    (C, S) holds at most B = C * max(1, 3d + S - 1, 4d) envelopes (d = S - majority: late replies
    are never removed), and the encoding follows from B: 8 network slots for C, S <= 3 with B <= 8
    (the states and fingerprints of those systems are what they always were), 16 slots for B <= 16
    (e.g. (4..6, 2), (2, 3), (3, 3), (1, 4), (2, 4)), and 32 slots for (4, 3), (5, 3), (3, 4) and
    (4, 4). Only the 32-slot encoding describes 32 envelopes per state; the others describe 16, as
    the CPU oracle does. A state past its slots fails `join()` with SR_ERR_UNSUPPORTED."""
    MODEL_ID = N.SR_MODEL_ABD

    def __init__(self, client_count=2, server_count=2):
        self.client_count, self.server_count = client_count, server_count

    def params(self):
        return [self.client_count, self.server_count]
