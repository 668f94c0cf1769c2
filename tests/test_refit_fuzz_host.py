"""CPU: the text of the primitive-driven refit (refit_body.inc through tests/cpp/refit_body_host.cpp) on the cases and moves of
tests/refit_adversarial.py: signed zeros, NaN in chosen slots, infinities and empty boxes, a root of zero extent, foreign geometry;
trees of the checker's builders from one primitive to 1500, leaf limits (1, 1) to (9, 15). Nodes and pair records equal
leaf_boxes + the checker's Bvh::refit byte for byte, from boxes (3D and 2D) and from triangles.

And the conditions under which the same cases mean something on the device (tests/test_gpu_refit_fuzz.py): each of three wrong
selection rules — the comparison reversed, IEEE minNum / maxNum, the right child as accumulator — gets node bounds wrong on every case
large enough to offer the placements, the planted NaN reaches the root and only it does, and over the cases every slot of the node
layout carries a surviving NaN."""
import functools

import numpy as np
import pytest

import adversarial_queries as adv
import oracle
import refit_adversarial as ra
from test_gpu_refit_prims import expected_tree
from test_refit_prims_host import BOXES2, BOXES3, TRIS, check, compile_harness


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return compile_harness(tmp_path_factory.mktemp("refit_fuzz"))


@functools.lru_cache(maxsize=None)
def _witnesses(case):
    return ra.witnesses(case, moves=("zeros", "nan_leaf", "nan_root"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("case", ra.CASES, ids=adv.case_id)
def test_kernel_text_equals_the_expectation_on_every_move(dll, orc, case):
    kind, n, lim, bq, dtype, seed = case
    raw, nodes, ids = ra.checker_tree(orc, case)
    dim = ra.dim_of(case)
    counts = nodes["index"].astype(np.uint64) & np.uint64(15)
    assert int(counts.sum()) == n and int(counts.max()) <= lim[1] and (n > 1 or len(nodes) == 1)
    for name in ra.MOVES:
        moved = ra.apply(case, name, raw, nodes, ids)
        assert moved.dtype == raw.dtype and moved.shape == ((n, 9) if ra.is_tri(case) else (n, 2 * dim)), name
        bb = ra.moved_boxes(orc, moved)
        want = check(dll, orc, nodes, ids, bb, BOXES3 if dim == 3 else BOXES2, bb, dim=dim)
        assert (want["index"] == nodes["index"]).all(), name
        if ra.is_tri(case):
            check(dll, orc, nodes, ids, bb, TRIS, moved)
        src = ra.sphere_source(case, name, raw)
        if src is not None:                                    # the boxes of these moves are Sphere::get_bbox of an array the device can be fed
            assert ra.bounds(orc, src)[0].tobytes() == moved.tobytes(), name
        if name == "collapse":
            root = want["bounds"][0]
            assert (root[0::2] == root[1::2]).all() and np.isfinite(root).all()
        if name == "inf" and n >= 17:
            assert np.isinf(want["bounds"][0]).any()


@pytest.mark.parametrize("case", [c for c in ra.CASES if c[1] >= 17], ids=adv.case_id)
def test_wrong_models_are_caught(orc, case):
    """Not vacuous: on every case of 17 primitives or more, `zeros` tells all three wrong models from the expectation, and both NaN
    moves tell IEEE minNum / maxNum and the right-child accumulator from it."""
    w = _witnesses(case)
    print(adv.case_id(case), w)
    assert min(w["zeros"].values()) > 0, w["zeros"]
    for name in ("nan_leaf", "nan_root"):
        assert w[name]["ieee"] > 0 and w[name]["right_acc"] > 0, (name, w[name])


@pytest.mark.parametrize("case", [c for c in ra.CASES if c[1] >= 17], ids=adv.case_id)
def test_zeros_are_placed_where_the_order_shows(orc, case):
    """In the moved boxes themselves: a sibling pair of leaves (+0, -0) and one (-0, +0), and where the leaf limits allow leaves of two,
    a leaf whose last two slots are (+0, -0) and one with (-0, +0)."""
    raw, nodes, ids = ra.checker_tree(orc, case)
    dim = ra.dim_of(case)
    draw, pairs, big = ra.zeros_plan(ra.move_rng(case, "zeros"), nodes)
    axis = draw % dim
    bb = ra.moved_boxes(orc, ra.apply(case, "zeros", raw, nodes, ids))
    assert (bb[:, axis] == 0).all() and (bb[:, dim + axis] == 0).all()
    t = ra.Topology(nodes)
    want = expected_tree(orc, nodes, ids, bb, dim).nodes()
    assert len(pairs) == min(2, len(t.sibling_leaf_pairs())) >= 1           # (a tree of three nodes has one pair)
    for j, (l, r) in enumerate(pairs):
        for slot in (2 * axis, 2 * axis + 1):
            assert bool(np.signbit(want["bounds"][l][slot])) == (j == 1) and bool(np.signbit(want["bounds"][r][slot])) == (j == 0)
            assert bool(np.signbit(want["bounds"][t.parent[l]][slot])) == (j == 0)        # the climb keeps the right child's zero
    taken = {leaf for pair in pairs for leaf in pair}
    assert len(big) == min(2, sum(1 for leaf in t.leaves if t.count[leaf] >= 2 and int(leaf) not in taken))
    assert big or case[2][1] == 1 or len(nodes) == 3
    for j, leaf in enumerate(big):
        a, b = int(ids[t.last(leaf) - 1]), int(ids[t.last(leaf)])
        assert bool(np.signbit(bb[a, axis])) == (j == 1) and bool(np.signbit(bb[b, axis])) == (j == 0)
        assert bool(np.signbit(want["bounds"][leaf][2 * axis])) == (j == 0)               # the fold keeps the last slot's zero


def _nan_slots(case, reaches_root):
    """The node-layout slots the planted NaN of nan_root occupies."""
    col = ra.nan_root_columns(case)[0 if reaches_root else 1]
    return {2 * col, 2 * col + 1} if ra.is_tri(case) else {ra._box_slot(col, ra.dim_of(case))}


@pytest.mark.parametrize("case", ra.CASES, ids=adv.case_id)
def test_planted_nans_stay_and_vanish_as_the_reference_has_it(orc, case):
    raw, nodes, ids = ra.checker_tree(orc, case)
    dim = ra.dim_of(case)
    t = ra.Topology(nodes)
    # nan_leaf: the last slot keeps it; a first slot, and p0 / p1 of a triangle, do not
    stays, vanishes, in_tri = ra.nan_leaf_plan(ra.move_rng(case, "nan_leaf"), nodes)
    moved = ra.apply(case, "nan_leaf", raw, nodes, ids)
    assert int(np.isnan(moved).sum()) == 1 + (vanishes is not None) + (ra.is_tri(case) and in_tri is not None)
    want = expected_tree(orc, nodes, ids, ra.moved_boxes(orc, moved), dim).nodes()
    assert int(np.isnan(want["bounds"][stays]).sum()) == (2 if ra.is_tri(case) else 1)
    for leaf in (vanishes, in_tri):
        assert leaf is None or not np.isnan(want["bounds"][leaf]).any()
    if case[1] >= 17:
        assert vanishes is not None or case[2][1] == 1
        assert in_tri is not None
    # nan_root: up the right spine to the root and nowhere else; the left child's stops at its parent
    right, left = ra.nan_root_plan(ra.move_rng(case, "nan_root"), nodes)
    want = expected_tree(orc, nodes, ids, ra.moved_boxes(orc, ra.apply(case, "nan_root", raw, nodes, ids)), dim).nodes()
    assert set(np.flatnonzero(np.isnan(want["bounds"][0])).tolist()) == _nan_slots(case, True)
    carriers = set(np.flatnonzero(np.isnan(want["bounds"]).any(axis=1)).tolist())
    assert carriers == set(t.spine) | ({left} if left is not None else set())
    if case[1] >= 17:
        assert left is not None or len(nodes) == 3             # (two leaves under the root: every left child hangs on the right spine)
    if left is not None:
        assert set(np.flatnonzero(np.isnan(want["bounds"][left])).tolist()) == _nan_slots(case, False)
        assert not np.isnan(want["bounds"][t.parent[left]]).any()


def test_every_node_slot_carries_a_surviving_nan(orc):
    """Over the parametrisation, per family: min and max of every axis hold a NaN in some expected tree, in a leaf and in the root."""
    for cases, dim in ((ra.CASES3, 3), (ra.CASES2, 2)):
        in_leaf, in_root = np.zeros(2 * dim, dtype=np.int64), np.zeros(2 * dim, dtype=np.int64)
        for case in cases:
            raw, nodes, ids = ra.checker_tree(orc, case)
            leaves = ra.Topology(nodes).leaves
            for name in ("nan_leaf", "nan_root"):
                want = expected_tree(orc, nodes, ids, ra.moved_boxes(orc, ra.apply(case, name, raw, nodes, ids)), dim).nodes()
                in_leaf += np.isnan(want["bounds"][leaves]).any(axis=0)
                in_root += np.isnan(want["bounds"][0])
        assert (in_leaf > 0).all() and (in_root > 0).all(), (dim, in_leaf, in_root)


def test_the_cases_hold_the_fixed_shapes_and_stay_small():
    assert len(ra.CASES3) == 24 and len(ra.CASES2) == 6
    for cases in (ra.CASES3, ra.CASES2):
        assert any(c[1] == 1 for c in cases) and any(c[1] == 2 and c[2] == (1, 1) for c in cases)
        assert any(c[1] == 200 and c[2] == (9, 15) for c in cases) and any(c[1] == 1500 for c in cases)
        assert max(c[1] for c in cases) <= ra.MAX_N
    assert any(c[1] == 1500 and c[2] == (9, 15) for c in ra.CASES3)
    assert {c[0] for c in ra.CASES3} == set(ra.KINDS3) and {c[4] for c in ra.CASES3} == {np.float32, np.float64}
    assert any(c[2] == (1, 1) and c[1] >= 17 for c in ra.CASES)


def test_the_model_tells_the_rules_apart():
    """refit_model itself: the three wrong rules on two boxes, against what each is defined to do."""
    nodes = np.zeros(3, dtype=oracle.NODEF)
    nodes["index"] = [1 << 4, (0 << 4) | 1, (1 << 4) | 1]
    ids = np.arange(2, dtype=np.uint64)
    bb = np.array([[0.0, 1, 1, 2, 2, np.nan], [-0.0, np.nan, 1, 2, 2, 3]], dtype=np.float32)
    root = {rule: ra.refit_model(nodes, ids, bb, 3, rule)["bounds"][0] for rule in ra.RULES}
    sign = {rule: bool(np.signbit(b[0])) for rule, b in root.items()}
    assert sign == {"reference": True, "reversed": False, "ieee": True, "right_acc": False}
    assert {rule: bool(np.isnan(b[2])) for rule, b in root.items()} == {"reference": True, "reversed": False, "ieee": False, "right_acc": False}
    assert {rule: bool(np.isnan(b[5])) for rule, b in root.items()} == {"reference": False, "reversed": False, "ieee": False, "right_acc": True}
    assert _bits(root["ieee"][1:2])[0] == _bits(np.array([2.0], np.float32))[0]
