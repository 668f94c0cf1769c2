"""CPU: the generator, the reference model and the executor of tests/handle_sequences.py, without the library. The conditions on the
committed sequences are asserted here, from the generated list, so that the `-m gpu` run of the same sequences cannot be vacuous:
what occurs (every step kind, every ordered pair of the state-changing kinds as neighbours, every family, start state and size), that
the reference alone takes every sequence to its end with exactly the refusals the model predicts, and that the executor's checks
catch each class of state bug when an adapter simulates it."""
import numpy as np
import pytest

import handle_sequences as hs


@pytest.fixture(scope="module")
def cases():
    return [hs.committed_case(i) for i in range(len(hs.SPECS))]


def test_sequences_are_deterministic_per_seed(restatement):
    for index in (0, 11, 14, len(hs.SPECS) - 1):
        a = hs.Generator(hs.SPECS[index], restatement).run()
        b = hs.Generator(hs.SPECS[index], restatement).run()
        assert a.id == b.id == hs.case_id(hs.SPECS[index])
        assert len(a.steps) == len(b.steps) and a.nodes.tobytes() == b.nodes.tobytes() and a.prims.tobytes() == b.prims.tobytes()
        for x, y in zip(a.steps, b.steps):
            assert x.keys() == y.keys()
            assert all(np.array_equal(x[key], y[key]) for key in x), (a.id, x, y)
    assert len({hs.case_id(s) for s in hs.SPECS}) == len(hs.SPECS)


def test_the_committed_set_covers_what_it_must(cases):
    kinds = [[st["op"] for st in c.steps] for c in cases]
    assert all(12 <= len(k) <= 16 for k in kinds), [(c.id, len(k)) for c, k in zip(cases, kinds) if not 12 <= len(k) <= 16]
    seen = {k for ks in kinds for k in ks}
    assert seen == set(hs.STATE_KINDS + hs.OTHER_KINDS), set(hs.STATE_KINDS + hs.OTHER_KINDS) ^ seen
    pairs = {(a, b) for ks in kinds for a, b in zip(ks, ks[1:])}
    missing = [(a, b) for a in hs.STATE_KINDS for b in hs.STATE_KINDS if (a, b) not in pairs]
    assert not missing, missing
    assert {c.family for c in cases} == set(hs.FAMILIES)
    assert {c.spec["start"] for c in cases} == set(hs.STARTS)
    assert {c.spec["depth"] for c in cases if c.spec["start"] == "deep"} == {65, 300}
    for family in hs.FAMILIES:
        mine = [c for c in cases if c.family == family]
        assert {1, 2} <= {c.spec["n"] for c in mine}, family
        want = set(hs.STARTS) - ({"deep"} if family[0] == "2" else set())
        assert {c.spec["start"] for c in mine} == want, family
    assert {c.spec["n"] for c in cases} >= set(hs.SIZES)
    assert {c.spec["build"][0] for c in cases if c.spec["start"] == "build"} == {b[0] for b in hs.BUILDS}
    assert {True, False} == {c.spec["lattice"] for c in cases}
    # what the drawn arguments reach
    steps = [(c, st) for c in cases for st in c.steps]
    assert {st["carry"] for _, st in steps if st["op"] == "append_chain"} == {"sync_device", "refit", "refit_boxes"}
    assert {bool(st["side"]) for _, st in steps if st["op"] in ("refit_boxes", "refit_tris")} == {True, False}
    assert {st["look"] for _, st in steps} == {"all", "device", "records"}
    for c in cases:
        if c.spec["start"] == "wide":                        # extract_bvh(0) is the way to a tree optimize accepts, and it is taken
            ops = [(st["op"], st.get("root")) for st in c.steps]
            assert ("extract", 0) in ops and "optimize" in [o for o, _ in ops[ops.index(("extract", 0)):]], c.id


def test_extract_roots_are_leaves_inner_nodes_and_the_root(cases, restatement):
    seen = set()
    for c in cases:
        model = hs.RefAdapter(restatement, c.family)
        model.start(c.spec, c.prims, c.nodes, c.ids)
        for st in c.steps:
            if st["op"] == "extract":
                seen.add("root" if st["root"] == 0 else "leaf" if int(model.nodes["index"][st["root"]]) & 15 else "inner")
            model.step(st)
    assert seen == {"root", "leaf", "inner"}


def test_growth_starts_under_64_levels_and_ends_over(cases, restatement):
    grown = 0
    for c in cases:
        model = hs.RefAdapter(restatement, c.family)
        model.start(c.spec, c.prims, c.nodes, c.ids)
        for st in c.steps:
            before = hs.tree_facts(model.nodes)[1]
            model.step(st)
            if st["op"] == "append_chain":
                assert hs.tree_facts(model.nodes)[1] > 64, c.id
                grown += before < 64
    assert grown >= 3


def test_the_reference_alone_runs_every_sequence_to_its_end(cases, restatement):
    """Legality tracking is right (no optimize with unreachable nodes, no root out of range, no split of a one-primitive leaf: the
    model would refuse or the checker fail), and the refusals are exactly the deliberate ones."""
    total = refusals = 0
    for c in cases:
        log = []
        assert hs.execute(c, hs.RefAdapter(restatement, c.family), restatement, checks="AB", log=log) == len(c.steps)
        assert [entry[:2] for entry in log] == [(k, st["op"]) for k, st in enumerate(c.steps)], c.id      # every step, in order
        assert log[-1][2] >= 50, (c.id, "rays that hit", log[-1][2])
        refused = [st["op"] for st in c.steps if st["op"].startswith("refuse")]
        assert len(refused) <= 1, c.id
        total += len(c.steps)
        refusals += len(refused)
        model = hs.RefAdapter(restatement, c.family)
        model.start(c.spec, c.prims, c.nodes, c.ids)
        for st in c.steps:
            out = model.step(st)
            assert (out is not None and out[0] == "refused") == st["op"].startswith("refuse"), (c.id, st["op"], out)
            if st["op"] == "refuse_optimize":
                assert out[1:] == hs.REFUSED_OPTIMIZE
            if st["op"] == "refuse_refit":
                assert out[1:] == hs.REFUSED_REFIT
    assert refusals >= 2 and total - refusals >= 0.85 * total, (total, refusals)


@pytest.mark.parametrize("defect", hs.DEFECTS, ids=lambda d: d.__name__)
def test_the_checks_discriminate(cases, restatement, defect):
    """Each simulated state bug is caught by the executor on at least one committed sequence."""
    caught = []
    for c in cases:
        try:
            hs.execute(c, defect(restatement, c.family), restatement, checks="AB")
        except hs.Mismatch as exc:
            caught.append((c.id, str(exc)))
    assert caught, f"{defect.__name__}: no committed sequence notices it"
    print(f"{defect.__name__}: caught on {len(caught)} of {len(cases)} sequences, first by {caught[0][1]}")
    assert caught[0][0] in caught[0][1], f"{defect.__name__} was caught by sequence {caught[0][0]} without naming it"
