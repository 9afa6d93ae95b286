"""The certificate of a finished check (CheckerBuilder.certify(), checker.certificate(); csrc/certify.hpp):
what a test asserts of it, and a plain Python reference of its figures for small registered models.

`assert_certified(c, complete=True)`: every error counter is 0; for a check that explored everything the
count identities tie the certificate's own figures (a second expansion of the arena by kernels that share
nothing with the search) to the search's three integers, and every `always` / `sometimes` property is
discovered iff a listed state discovers it, at the level of the first such state, in FIFO order at that very
state. After an early exit or a target stop (complete=False) the closure pass does not run: the roots, map,
tree, order and property-level assertions remain.

The identity for the state count is inits + edges + repeated_edges == state_count(): an init state the model
lists twice is popped and expanded twice by the search (as by the reference), and the certificate counts the
successors of such a repeat apart from `edges`; without repeated init states repeated_edges is 0.

`reference(model)`: a search in the reference's FIFO order over `_native.host_graph`'s successor lists."""
from stateright_amd import Expectation
from stateright_amd import _native as N

NONE = 2 ** 64 - 1
ERRORS = N.sr_certificate.ERRORS


def certified_props(c):
    """[(index, name)] of the properties a certificate counts: `always` and `sometimes`."""
    return [(i, name) for i, (name, exp) in enumerate(c.properties()) if exp in (Expectation.Always, Expectation.Sometimes)]


def assert_certified(c, complete=True, cert=None):
    cert = c.certificate() if cert is None else cert
    assert cert["ran"] == 1 and cert["skipped"] == 0, cert
    bad = {e: cert[e] for e in ERRORS if cert[e]}
    assert not bad, (bad, cert)
    assert cert["levels"] >= 1 and cert["states"] >= cert["inits"] >= 1, cert
    props = certified_props(c)
    assert cert["pmask"] == sum(1 << i for i, _ in props), cert
    found = c.discoveries()
    if complete:
        assert cert["explored_all"] == 1, cert
        assert cert["closure_missing"] == cert["closure_unlisted"] == cert["closure_late"] == cert["fifo_not_first"] == 0
        assert cert["states"] - cert["repeated_inits"] == c.unique_state_count(), cert
        assert cert["inits"] + cert["edges"] + cert["repeated_edges"] == c.state_count(), cert
        if not cert["repeated_inits"]:
            assert cert["repeated_edges"] == 0, cert
        assert cert["levels"] - 1 == c.max_depth(), cert
    for i, name in props:
        assert cert["disc_wrong"][i] == 0, (name, cert)
        if name not in found:
            assert cert["disc_index"][i] == NONE, (name, cert)
            if complete:
                assert cert["holds"][i] == 0 and cert["first_index"][i] == NONE, (name, cert)
            continue
        assert cert["holds"][i] > 0 and cert["disc_index"][i] < cert["states"], (name, cert)
        assert cert["disc_level"][i] == cert["first_level"][i] == len(found[name]), (name, cert)
        if cert["fifo"]:
            assert cert["disc_index"][i] == cert["first_index"][i], (name, cert)
    return cert


def reference(model, props, max_states=1 << 22):
    """The figures a certificate must report for a registered model, by a search in the reference's FIFO order
    (level 0 is the init states reversed, repeats kept; a state keeps its first generator). props: the checker's
    `properties()`. Returns states, inits, repeated_inits, levels (their sizes), unique, state_count, max_depth,
    edges, repeated_edges, and per certified property index holds, first_index and first_level."""
    succ, inits, conds = N.host_graph(model.MODEL_ID, model.params(), max_states)
    order = list(reversed(inits))
    repeated = [False] * len(order)
    seen = set()
    for pos in range(len(inits)):  # in init order: arena index k - 1 - pos
        repeated[len(inits) - 1 - pos] = inits[pos] in seen
        seen.add(inits[pos])
    sizes, lo = [len(order)], 0
    edges = repeated_edges = 0
    while lo < len(order):
        hi = len(order)
        for at in range(lo, hi):
            out = succ[order[at]]
            if at < len(inits) and repeated[at]:
                repeated_edges += len(out)  # (popped and expanded like any other, as the search does)
            else:
                edges += len(out)
            for _, j in out:
                if j not in seen:
                    seen.add(j)
                    order.append(j)
        if len(order) > hi:
            sizes.append(len(order) - hi)
        lo = hi
    assert len(seen) == len(succ)
    level_of = [d for d, size in enumerate(sizes) for _ in range(size)]
    ref = {"states": len(order), "inits": len(inits), "repeated_inits": sum(repeated), "levels": sizes, "unique": len(seen),
           "state_count": len(inits) + edges + repeated_edges, "max_depth": len(sizes) - 1, "edges": edges,
           "repeated_edges": repeated_edges, "holds": {}, "first_index": {}, "first_level": {}}
    for p, (_, exp) in enumerate(props):
        if exp not in (Expectation.Always, Expectation.Sometimes):
            continue
        # conds holds the CONDITION; an `always` property is discovered where it fails, a `sometimes` one where it holds
        hit = [at for at, i in enumerate(order) if bool(conds[i] >> p & 1) != (exp == Expectation.Always)]
        ref["holds"][p] = len(hit)
        ref["first_index"][p] = hit[0] if hit else NONE
        ref["first_level"][p] = level_of[hit[0]] if hit else None
    return ref


def assert_matches_reference(cert, ref):
    """A complete check's certificate against `reference`: the figures no order changes, and in FIFO order the
    first discovering index."""
    assert (cert["states"], cert["inits"], cert["repeated_inits"], cert["levels"]) == \
        (ref["states"], ref["inits"], ref["repeated_inits"], len(ref["levels"])), (cert, ref)
    assert (cert["edges"], cert["repeated_edges"]) == (ref["edges"], ref["repeated_edges"]), (cert, ref)
    for p, holds in ref["holds"].items():
        assert cert["holds"][p] == holds, (p, cert, ref)
        if holds:
            assert cert["first_level"][p] == ref["first_level"][p], (p, cert, ref)
            if cert["fifo"]:
                assert cert["first_index"][p] == ref["first_index"][p], (p, cert, ref)
