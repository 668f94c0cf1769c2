"""-m gpu: the committed sequences of tests/handle_sequences.py on the library, one test per sequence, and the transitions known to be
subtle as hand-written sequences that do not depend on the draw. After every step the aged handle is compared byte for byte with the
reference model (streams, arrays, accessor view, hit records and counters) and with a fresh handle made from the model's arrays
(point and box queries, traversal_cost); tests/test_handle_sequences_host.py asserts what the committed set covers."""
import numpy as np
import pytest

import handle_sequences as hs

pytestmark = pytest.mark.gpu


def _run(case, orc, restatement):
    checker = restatement if hs.needs_growing_stack(case) else orc
    assert hs.execute(case, hs.GpuAdapter(case.family), checker) == len(case.steps)


@pytest.mark.parametrize("index", range(len(hs.SPECS)), ids=[hs.case_id(s) for s in hs.SPECS])
def test_committed_sequence(orc, restatement, index):
    _run(hs.committed_case(index), orc, restatement)


def _spec(name, family, n, **kw):
    return hs._spec(name, family, n, seed=kw.pop("seed", 900), **kw)


DEVICE, ALL = {"look": "device"}, {"look": "all"}


def test_side_stream_refit_then_cost_then_read(orc, restatement):
    """1: read, refit_boxes on a non-blocking side stream, traversal_cost, read, with no synchronisation in between: the root box and
    the mirror wait for the refit themselves."""
    case = hs.scripted_case(_spec("side_stream", "3f", 2000, build=hs.BUILDS[7]),
                            [("read", ALL), ("refit_boxes", {"side": True, "wait": False, "look": "cost"}), ("read", ALL)])
    _run(case, orc, restatement)


@pytest.mark.parametrize("carry", ["sync_device", "refit", "refit_boxes"])
@pytest.mark.parametrize("family", ["3f", "3d"])
def test_growth_past_64_levels_in_place(orc, restatement, family, carry):
    """2: a traced shallow tree (its depth is known to the handle) grows a chain of 70 pairs under one leaf; whichever call carries
    the edit to the device, the next trace walks the deep tree with a deep stack."""
    case = hs.scripted_case(_spec("growth", family, 300, leaf=(2, 4)), [("read", DEVICE), ("append_chain", {"carry": carry, "look": "device"}), ("refit_tris", ALL)])
    assert hs.tree_facts(case.nodes)[1] < 64
    _run(case, orc, restatement)


@pytest.mark.parametrize("family,depth", [("3f", 300), ("3d", 65)])
def test_deep_chain_optimized_then_a_shallow_subtree(orc, restatement, family, depth):
    """3: the depth follows the tree down as well: deep chain, optimize, trace, extract_bvh of a shallow subtree, trace."""
    g = hs.Generator(_spec("deep", family, depth + 1, start="deep", depth=depth), hs._restatement())
    g.take("optimize", look="device")
    f = g.facts()
    small = f["inner"][(f["under"][f["inner"]] <= 8) & (f["inner"] > 0)]
    assert len(small)
    g.take("extract", root=int(small[0]), look="device")
    g.take("refit_tris", look="all")
    assert hs.tree_facts(g.model.nodes)[1] < 8
    _run(g.case, orc, restatement)


@pytest.mark.parametrize("family", ["3f", "3d"])
def test_wide_array_refusal_and_the_way_out(orc, restatement, family):
    """4: an array with unused sibling pairs: optimize refused, refit_boxes, extract_bvh(0), optimize, refit_tris, trace."""
    case = hs.scripted_case(_spec("wide", family, 300, start="wide"),
                            [("refuse_optimize", DEVICE), ("refit_boxes", DEVICE), ("extract", DEVICE), ("optimize", DEVICE), ("refit_tris", ALL)])
    assert case.steps[2]["root"] == 0
    _run(case, orc, restatement)


@pytest.mark.parametrize("family", ["2f", "2d"])
def test_2d_narrow_mirror_through_edits_and_device_ops(orc, restatement, family):
    """5: the 20/40-byte view: get_node, set_bbox, optimize, the view again, refit_boxes, set_bbox, refit, the stream."""
    case = hs.scripted_case(_spec("narrow", family, 300, lattice=family == "2d"),
                            [("get_node", DEVICE), ("set_bbox", DEVICE), ("optimize", DEVICE), ("get_node", ALL), ("refit_boxes", DEVICE), ("set_bbox", DEVICE),
                             ("refit", DEVICE), ("read", ALL)])
    _run(case, orc, restatement)


@pytest.mark.parametrize("family", ["3f", "3d"])
def test_device_resident_life_without_a_mirror(orc, restatement, family):
    """6: deserialize_device, refit_tris, serialize_device, deserialize_device, optimize: the mirror is filled by the last look only."""
    case = hs.scripted_case(_spec("resident", family, 2000, start="deserialize_device", build=hs.BUILDS[4]),
                            [("refit_tris", DEVICE), ("roundtrip_device", DEVICE), ("optimize", DEVICE), ("read", ALL)])
    _run(case, orc, restatement)


@pytest.mark.parametrize("family", hs.FAMILIES)
def test_one_primitive_every_legal_step(orc, restatement, family):
    """7: the root is a leaf and there are no pair records: every step kind that is legal there, once."""
    kinds = ["read", "sync_host", "set_bbox", "refit", "refit_boxes", "optimize", "extract", "roundtrip_host", "roundtrip_device", "append_remove"]
    kinds += ["get_node"] if family[0] == "2" else ["refit_tris", "append_chain"]
    case = hs.scripted_case(_spec("one", family, 1), kinds)
    assert len(case.nodes) == 1
    _run(case, orc, restatement)


@pytest.mark.parametrize("family", ["3f", "2d"])
def test_mirror_valid_then_stale_then_read_again(orc, restatement, family):
    """8: build, read, optimize (the valid mirror is pushed and refreshed), refit_boxes (it goes stale), optimize, read."""
    case = hs.scripted_case(_spec("mirror", family, 2000, build=hs.BUILDS[3]),
                            [("read", ALL), ("optimize", DEVICE), ("refit_boxes", DEVICE), ("optimize", DEVICE), ("read", ALL)])
    _run(case, orc, restatement)


@pytest.mark.parametrize("family", ["3f", "2f"])
def test_side_stream_refit_then_extract(orc, restatement, family):
    """9 (found by reading while these tests were written): extract_bvh runs on the library's own stream and, unlike refit(),
    optimize() and the mirror, did not wait for a refit_boxes in flight on a non-blocking stream: the subtree could keep the boxes
    from before it. Nothing waits between the two calls here."""
    g = hs.Generator(_spec("side_extract", family, 2000, build=hs.BUILDS[2]), hs._restatement())
    g.take("refit_boxes", side=True, wait=False, look="counts")
    g.take("extract", root=int(g.model.nodes["index"][0]) >> 4, look="stream")
    g.take("refit_boxes", side=True, wait=False, look="counts")
    g.take("extract", root=0, look="all")
    _run(g.case, orc, restatement)
