"""CPU: the host harness of the instanced ray kernels (tests/instanced_scenes.py: instanced_body.inc compiled by g++) on the adversarial
scenes of tests/instanced_adversarial.py — mirrored, exact, squashed, huge / tiny, far, coincident and dead instances; top trees of one
leaf with 1 and with 15 instances, of two leaves, and built ones with leaf limits (1, 1) and (9, 15); geometries whose root is a leaf of
1, 2 and 15 triangles, with zero-area and duplicated triangles; tables of 16 and 17 geometries; 1 to 1021 rays with zero, -0.0 and NaN
direction components, origins on box planes, tmin > tmax, tmax = 0 and tmin = tmax = t.

Five tiers, strongest first: (a) bit-equal to the composition where the order is fixed; (b) the exact tier against plain numpy, nothing
excluded; (c) robust mode against a float64 flattened brute force on the clear rays; (d) robust mode under built top trees: the
order-free properties; (e) fast mode under built top trees: it may lose hits to box culling, it never invents or distorts one. And
deep stacks with the marker at every tier of the stack (LDS, scratch, HBM spill).

Measured by test_float64_truth (worst relative error in t of the reference composition against the float64 truth over the clear rays,
the bound on the walk being 4 times that; unclear share):
    benign float32 6.14e-06 (1.1 %)   benign float64 4.90e-14 (1.1 %)
    mirror float32 2.92e-05 (0.9 %)   mirror float64 5.24e-14 (0.9 %)
    far    float32 3.89e-03 (6.3 %)   far    float64 3.22e-11 (6.5 %)
Fast mode under the built top trees of test_built_top_trees loses 0 to 297 of 800 to 1650 hits of the robust composition, all but 0 to
15 per scene on axis-aligned rays."""
import functools

import numpy as np
import pytest

import adversarial_queries as adv
import instanced_adversarial as ia
import instanced_scenes as sc
from instanced_scenes import INVALID, MODES4
from test_instanced_host import expect_single_leaf


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return sc.compile_harness(tmp_path_factory.mktemp("instanced_fuzz"))


def bit_equal(scene, rays, modes=MODES4, ids=(False, True), deep_cap=0):
    """Tier (a): records, instances and counters of the harness against the composition in slot order. -> hits per mode."""
    out = {}
    for any_hit, robust in modes:
        for original_ids in ids:
            want, want_inst, want_cnt = expect_single_leaf(scene, rays, any_hit, robust, original_ids)
            got, got_inst, got_cnt = sc.host_walk(scene, rays, any_hit, robust, original_ids, deep_cap=deep_cap)
            assert sc.same_records(got, want), (any_hit, robust, original_ids)
            assert (got_inst == want_inst).all(), (any_hit, robust, original_ids)
            assert (got_cnt == want_cnt).all(), (any_hit, robust, got_cnt, want_cnt)
            out[(any_hit, robust)] = int((got["prim"] != INVALID).sum())
    return out


# ---- (a) single-leaf top trees: every class, every tiny shape, all ray kinds --------------------------------------------------------

def single_leaf_cases():
    """(name, classes, instances, table size (0: the five tiny geometries as they are), dtype, rays, seed): every class alone and all
    mixed, both scalar types and the ray counts dealt round robin."""
    kinds = list(ia.CLASSES) + ["mixed"]
    out = []
    for j, kind in enumerate(kinds):
        for dtype in (np.float32, np.float64):
            out.append((kind, tuple(ia.CLASSES) if kind == "mixed" else (kind,), (15, 12, 9)[j % 3], 0, dtype,
                        ia.RAY_COUNTS[(j + (dtype == np.float64)) % len(ia.RAY_COUNTS)], 300 + 2 * j + (dtype == np.float64)))
    # tables of exactly 16 and 17 geometries (kInstSmallGeoms and one more), the last entry in use
    out += [("table", ("benign", "mirror", "squash"), 15, 16, np.float32, 1021, 330), ("table", ("benign", "mirror", "squash"), 15, 17, np.float64, 257, 331)]
    return out


def case_id(c):
    return f"{c[0]}-i{c[2]}-g{c[3]}-{np.dtype(c[4]).name}-r{c[5]}"


def single_leaf_scene(dll, orc, case, dead=0.1, which=None):
    kind, classes, n, table, dtype, n_rays, seed = case
    rng = np.random.default_rng(seed)
    geoms = ia.tiny_geometries(orc, rng, dtype)
    if table:
        geoms = ia.table_of(geoms, table)
    m, gids, dead_ids = ia.instances(rng, n, dtype, classes, len(geoms), dead=0 if which is not None else dead)
    if which is not None:
        m64 = m.astype(np.float64)
        dead_ids = ia.kill(rng, m64, gids, len(geoms), which=which)
        m = m64.astype(dtype)
    scene = sc.Scene(dll, geoms, m, gids).single_leaf_top(seed)
    assert all(not scene.enabled(i) for i in dead_ids)
    if table:
        assert any(scene.enabled(i) and int(gids[i]) == table - 1 for i in range(n))
    rays = ia.special_rays(scene, n_rays, seed, first_pass=lambda r: sc.compose(scene, r, scene.top_ids, False, True)[0])
    if kind in ("full_leaf", "table", "squash") and any(scene.enabled(i) for i in range(n)):       # and the grazing rays from 30 and 3000 units
        rays = np.ascontiguousarray(np.concatenate([rays, ia.grazing_rays(scene, np.random.default_rng(seed + 5), 12)]))
    return scene, rays, dead_ids


@pytest.mark.parametrize("case", single_leaf_cases(), ids=case_id)
def test_single_leaf_classes_equal_the_composition(dll, orc, case):
    scene, rays, dead_ids = single_leaf_scene(dll, orc, case)
    hits = bit_equal(scene, rays)
    if len(rays) >= 257:
        assert hits[(False, True)] > len(rays) // 10
    _, inst, _ = sc.host_walk(scene, rays, False, True)
    assert not np.isin(inst, dead_ids).any()


TINY = [("one", ("benign",), 1, 0, np.float32, 1021, 340), ("one", ("mirror",), 1, 0, np.float64, 65, 341),
        ("full_leaf", ("benign", "squash", "mirror"), 15, 0, np.float32, 1021, 342), ("full_leaf", ("far", "pow2"), 15, 0, np.float64, 257, 343)]


@pytest.mark.parametrize("case", TINY, ids=case_id)
def test_tiny_top_leaves_equal_the_composition(dll, orc, case):
    """A leaf of one instance; a leaf of 15 whose first, a middle and the last slot are dead: the marker of the 14th slot has no slots
    left, and the slot loop steps over dead slots at both ends."""
    n = case[2]
    scene0, _, _ = single_leaf_scene(dll, orc, case, dead=0)
    slots = scene0.top_ids                                     # slot -> instance (the scene is rebuilt with the same seed: same shuffle)
    which = [int(slots[0]), int(slots[7]), int(slots[14])] if n == 15 else None
    scene, rays, dead_ids = single_leaf_scene(dll, orc, case, dead=0, which=which)
    assert (scene.top_ids == slots).all() and len(dead_ids) == (3 if n == 15 else 0)
    hits = bit_equal(scene, rays)
    assert hits[(False, True)] > len(rays) // 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_all_dead_scene_misses_everything(dll, orc, dtype):
    """Every instance dead: every ray misses, nothing but the top leaf is counted."""
    case = ("dead", ("benign", "far"), 12, 0, dtype, 257, 350)
    scene, rays, dead_ids = single_leaf_scene(dll, orc, case, dead=0, which=list(range(12)))
    assert len(dead_ids) == 12
    bit_equal(scene, rays)
    live = int((~sc.nan_flagged(rays)).sum())
    for any_hit, robust in MODES4:
        got, inst, cnt = sc.host_walk(scene, rays, any_hit, robust)
        assert (got["prim"] == INVALID).all() and (inst == INVALID).all() and (cnt == [0, 0, live]).all()
        assert got["t"].tobytes() == np.ascontiguousarray(rays[:, 7]).tobytes()
    # ... and under a built top tree: the composition's counters (nothing) plus the top tree's own walk, which is the checker's
    # single-level walk of that tree over primitives nothing can hit (zero triangles): its pair records and its leaves
    scene = ia.built_top(scene, orc, (1, 1), (0, 2))
    assert ia.top_leaves(scene) == 12
    for any_hit, robust in MODES4:
        got, inst, cnt = sc.host_walk(scene, rays, any_hit, robust)
        assert (got["prim"] == INVALID).all() and (inst == INVALID).all()
        assert (cnt == ia.top_walk_counters(orc, scene, rays, any_hit, robust)).all(), (any_hit, robust, cnt)


def test_the_composition_takes_the_special_rays(orc, dll):
    """The reference alone (no harness result is looked at): the composition handles zero, -0.0 and NaN directions, origins on box
    planes, tmin > tmax, tmax = 0 and tmin = tmax = t without raising, and same_records compares the NaNs it reports."""
    scene, rays, _ = single_leaf_scene(dll, orc, ("mixed", tuple(ia.CLASSES), 15, 0, np.float32, 1021, 360))
    d = rays[:, 3:6]
    zeros = (d == 0).sum(axis=1)
    assert all((zeros == k).sum() > 5 for k in (1, 2, 3)) and (np.signbit(d) & (d == 0)).any() and np.isnan(d).any(axis=1).sum() > 5
    assert (rays[:, 6] > rays[:, 7]).any() and (rays[:, 7] == 0).any()
    pinned = (rays[:, 6] == rays[:, 7]) & (rays[:, 7] > 0)
    assert pinned.sum() > 10
    for any_hit, robust in MODES4:
        a, a_inst, _ = sc.compose(scene, rays, scene.top_ids, any_hit, robust)
        b, b_inst, _ = sc.compose(scene, rays, scene.top_ids, any_hit, robust)
        assert sc.same_records(a, b) and (a_inst == b_inst).all()
        null = zeros == 3
        assert (a["prim"][null] == INVALID).all() and (a["prim"][rays[:, 6] > rays[:, 7]] == INVALID).all()
    closest, _, _ = sc.compose(scene, rays, scene.top_ids, False, True)
    assert (closest["prim"][pinned] != INVALID).all() and (closest["t"][pinned] == rays[pinned, 7]).all()


# ---- (b) the exact tier -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_inputs(seed, n_inst, n_rays):
    """Lattice triangles in root-leaf geometries of 1, 2 and 15, pow2 instances, lattice rays: float64 arrays, exact in float32 too."""
    rng = np.random.default_rng(seed)
    tris = [ia.lattice_tris(rng, k, np.float64) for k in (1, 2, 15, 15)]
    tris[3][5] = tris[3][4]                                    # two coincident triangles in one leaf: a tie inside a geometry
    m = ia.pow2(rng, n_inst, np.float64)
    if n_inst >= 2:
        m[n_inst - 1] = m[n_inst - 2]                          # two coincident instances: a tie between slots
    gids = ia.assign_geometries(rng, m, 4)
    rays = ia.lattice_rays(rng, n_rays, np.float64)
    return tris, m, gids, rays


def exact_scene(dll, orc, seed, n_inst, n_rays, dtype):
    tris, m, gids, rays = exact_inputs(seed, n_inst, n_rays)
    geoms = [ia.leaf_geometry(orc, t.astype(dtype)) for t in tris]
    scene = sc.Scene(dll, geoms, m.astype(dtype), gids).single_leaf_top(seed)
    return scene, tris, rays.astype(dtype)


def check_exact(world2obj, top_ids, obj2world, tris, gids, rays, results, what):
    """`results`: {any_hit: (records, instances)} of a walk under a single-leaf top tree with slots `top_ids`, against exact_pairs."""
    assert (world2obj.astype(np.float64) == ia.exact_inverse(obj2world)).all(), what
    order = [int(i) for i in top_ids]
    pairs = ia.exact_pairs(world2obj, tris, gids, order, rays, rays.dtype)
    ia.assert_intermediates_exact(ia.exact_pairs(world2obj, tris, gids, order, rays, np.float32), ia.exact_pairs(world2obj, tris, gids, order, rays, np.float64))
    witnesses = {}
    for any_hit, (got, inst) in results.items():
        prim, want_inst, t, u, v, tied = ia.exact_expect(pairs, rays, any_hit)
        assert (got["prim"] == prim).all() and (inst == want_inst).all(), (what, any_hit, np.flatnonzero((got["prim"] != prim) | (inst != want_inst))[:8])
        for f, want in (("t", t), ("u", u), ("v", v)):
            assert np.ascontiguousarray(got[f]).tobytes() == want.tobytes(), (what, any_hit, f)
        hit = prim != INVALID
        on_end = hit & ((t == rays[:, 6]) | (t == rays[:, 7]))
        on_edge = hit & ((u == 0) | (v == 0) | (u + v == 1))
        witnesses[any_hit] = (int(hit.sum()), int(tied.sum()), int(on_end.sum()), int(on_edge.sum()))
    return witnesses


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("seed,n_inst,n_rays", [(401, 15, 1021), (402, 1, 65), (403, 6, 257)])
def test_exact_tier_equals_numpy(dll, orc, seed, n_inst, n_rays, dtype):
    scene, tris, rays = exact_scene(dll, orc, seed, n_inst, n_rays, dtype)
    results = {}
    for any_hit in (False, True):
        for robust in (False, True):                           # (a single-leaf top tree and root-leaf geometries: no box is ever tested)
            got, inst, _ = sc.host_walk(scene, rays, any_hit, robust)
            if any_hit in results:
                assert sc.same_records(got, results[any_hit][0]) and (inst == results[any_hit][1]).all()
            results[any_hit] = (got, inst)
    w = check_exact(scene.world2obj, scene.top_ids, scene.obj2world, tris, scene.gids, rays, results, (seed, np.dtype(dtype).name))
    print(f"exact tier seed {seed} {np.dtype(dtype).name}: (hits, ties in t, t on tmin / tmax, hits on an edge) closest {w[False]}, any {w[True]}")
    if n_rays >= 1021:                                         # not vacuous
        assert min(w[False]) > 0 and w[False][0] > 100


# ---- (c) the float64 flattened truth, robust mode ----------------------------------------------------------------------------------------

TRUTH_CASES = [(kind, dtype, 500 + j) for j, kind in enumerate(ia.TRUTH_CLASSES) for dtype in (np.float32, np.float64)]


def truth_scene(dll, orc, kind, dtype, seed):
    """40 instances of one class (about 10 % dead) of the soup and two leaf geometries under a built top tree; 800 of scene_rays and 400
    rays at triangle centroids."""
    rng = np.random.default_rng(seed)
    geoms = ia.truth_geometries(orc, rng, dtype)
    m, gids, _ = ia.instances(rng, 40, dtype, (kind,), len(geoms))
    scene = ia.built_top(sc.Scene(dll, geoms, m, gids), orc, (1, 8), (0, 2))
    return scene, np.ascontiguousarray(np.concatenate([sc.scene_rays(scene, 800, seed + 50), ia.centroid_rays(scene, rng, 400)]))


def reference_against_truth(scene, rays, kind, dtype):
    """The precondition of tier (c), on the reference alone: float64_truth, and the composition's agreement with it. Every case but
    far / float32 agrees on all clear rays. There one ulp of a coordinate, 2^-10 at 1e4, is the margin itself: the rounded object-space
    origin is off by about 2e-3, which a ray at a shallow angle to its triangle turns into tenths of a barycentric unit, and the
    composition misses or swaps a few hits that the truth has well inside a triangle (18 of 1200 rays here). The claim is restricted to what
    holds: those rays are excused, counted and printed. -> (truth, excused rays, the reference's worst relative error in t, unclear share)."""
    truth = ia.float64_truth(scene, rays)
    reference, ref_inst, _ = sc.compose(scene, rays, range(scene.n), False, True, original_ids=True)
    excused = ia.truth_mismatch(truth, reference, ref_inst)
    if not (kind == "far" and dtype == np.float32):
        assert not excused.any()
    assert excused.sum() <= len(rays) // 20                    # (keeps the tier from becoming vacuous; not a measured bound)
    ref_err, unclear = ia.check_against_truth(truth, reference, ref_inst, "the reference composition", excused)
    print(f"float64 truth {kind} {np.dtype(dtype).name}: reference composition worst relative error in t {ref_err:.3g}, unclear {100 * unclear:.1f} %, "
          f"clear rays on which the reference differs from the truth {int(excused.sum())} of {len(rays)}")
    assert unclear <= 0.10
    return truth, excused, ref_err


@pytest.mark.parametrize("kind,dtype,seed", TRUTH_CASES, ids=[f"{k}-{np.dtype(d).name}" for k, d, _ in TRUTH_CASES])
def test_float64_truth(dll, orc, kind, dtype, seed):
    """Robust closest-hit with ORIGINAL_IDS against the float64 brute force over the world-space triangles: on the clear rays the same
    hit or miss, instance and primitive; t within 4 times the worst relative error of the reference composition itself, measured here
    on the same rays (the module's docstring and DESIGN.md record the values). At most 10 % of the rays may be unclear."""
    scene, rays = truth_scene(dll, orc, kind, dtype, seed)
    truth, excused, ref_err = reference_against_truth(scene, rays, kind, dtype)
    got, inst, _ = sc.host_walk(scene, rays, False, True, original_ids=True)
    err, _ = ia.check_against_truth(truth, got, inst, "the walk", excused)
    assert err <= 4 * ref_err, (err, ref_err)
    got_any, inst_any, _ = sc.host_walk(scene, rays, True, True, original_ids=True)
    clear = ~truth[4] & ~excused
    assert ((got_any["prim"] != INVALID)[clear] == truth[0][clear]).all()


# ---- (d), (e) built top trees --------------------------------------------------------------------------------------------------------------

def built_cases(seed, drawn):
    """(class, instances, leaf limits, (builder, quality), dtype, table size, seed). Fixed: every size of TOP_SIZES under both leaf
    limits of TOP_LIMITS, the builders of adversarial_queries.BUILDERS in turn (shifted by the seed), the two scenes of 65 instances
    with tables of 16 and 17 geometries (every table entry used by a live instance); and `drawn` more shapes from the seed. The
    classes and the two scalar types are dealt round robin."""
    rng = np.random.default_rng(seed)
    shapes = [(n, lim) for n in ia.TOP_SIZES for lim in ia.TOP_LIMITS]
    shapes = [(n, lim, adv.BUILDERS[(j + seed) % len(adv.BUILDERS)]) for j, (n, lim) in enumerate(shapes)]
    for _ in range(drawn):
        shapes.append((int(rng.choice(ia.TOP_SIZES)), ia.TOP_LIMITS[int(rng.integers(0, 2))], adv.BUILDERS[int(rng.integers(0, len(adv.BUILDERS)))]))
    kinds = ia.ROUNDED_CLASSES + ("mixed",)
    out = []
    for j, (n, lim, bq) in enumerate(shapes):
        table = (16, 17)[lim == (9, 15)] if (n == 65 and j < 10) else 0
        out.append((kinds[(j + seed) % len(kinds)], n, lim, bq, (np.float32, np.float64)[(j + j // 2) % 2], table, 100 * seed + j))
    return out


def built_id(c):
    kind, n, lim, bq, dtype, table, seed = c
    return f"{kind}-i{n}-leaf{lim[0]}_{lim[1]}-b{bq[0]}q{bq[1]}-g{table}-{np.dtype(dtype).name}"


def built_scene_parts(dll, orc, case, soup=None):
    """The scene of a built-top case without its top tree, and its rays: scene_rays, rays at triangle centroids, the grazing rays from
    30 and 3000 units, the axis-aligned rays."""
    kind, n, lim, bq, dtype, table, seed = case
    rng = np.random.default_rng(seed)
    geoms = ia.tiny_geometries(orc, rng, dtype, soup)
    if table:
        geoms = ia.table_of(geoms, table)
    classes = ia.ROUNDED_CLASSES if kind == "mixed" else (kind,)
    m, gids, _ = ia.instances(rng, n, dtype, classes, len(geoms))
    scene = sc.Scene(dll, geoms, m, gids)
    if table:
        assert set(int(g) for g in gids if g < table) == set(range(table))
    return scene, rng


def built_rays(scene, rng, seed):
    live = [i for i in range(scene.n) if scene.enabled(i)]
    centroid = ia.centroid_rays(scene, rng, 700)
    graze = ia.grazing_rays(scene, rng, max(2, 400 // len(live)))
    return np.ascontiguousarray(np.concatenate([sc.scene_rays(scene, 600, seed + 7), centroid, graze, ia.axis_rays(scene, rng, 300)]))


BUILT_CASES = built_cases(6, 2)


@pytest.mark.parametrize("case", BUILT_CASES, ids=built_id)
def test_built_top_trees(dll, orc, case):
    """(d) robust mode keeps every hit of the box-free composition, with its t byte for byte; (e) fast mode never invents or distorts a
    hit. The loss counts of fast mode are printed: documentation, not a threshold."""
    kind, n, lim, bq, dtype, table, seed = case
    scene, rng = built_scene_parts(dll, orc, case)
    scene = ia.two_leaf_top(scene) if (n == 2 and lim == (1, 1)) else ia.built_top(scene, orc, lim, bq)
    counts = scene.top_nodes["index"].astype(np.uint64) & np.uint64(15)
    assert counts.max() <= lim[1] and (n < 17 or scene.top_depth() >= 1)
    rays = built_rays(scene, rng, seed)
    got, inst, _ = sc.host_walk(scene, rays, False, True)
    got_any, inst_any, _ = sc.host_walk(scene, rays, True, True)
    hits = ia.order_free(orc, scene, rays, got, inst, got_any, inst_any)
    assert hits > 500
    stable = ia.order_insensitive(scene, rays)
    assert stable.mean() > 0.98
    for any_hit in (False, True):
        common, _, _ = sc.compose(scene, rays, range(scene.n), any_hit, True)      # (robust: see one_sided)
        fast, fast_inst, _ = sc.host_walk(scene, rays, any_hit, False)
        if any_hit:                                            # (any-hit reports whichever hit it meets first: only hit or miss is one-sided)
            common["t"] = np.where(common["prim"] != INVALID, -np.inf, common["t"]).astype(scene.dtype)
        lost, of = ia.one_sided(orc, scene, rays, common, fast, fast_inst, False, built_id(case), stable)
        zeros = (rays[:, 3:6] == 0).any(axis=1)
        lost_axis = int(((common["prim"] != INVALID) & (fast["prim"] == INVALID) & zeros).sum())
        print(f"{built_id(case)} {'any' if any_hit else 'closest'}-hit fast mode: lost {lost} of {of} hits of the composition, {lost_axis} of them on axis-aligned rays")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fast_mode_loses_nothing_on_benign_scenes(dll, orc, dtype):
    """200 benign instances, scene_rays (no zero direction component, origins 1.6 scene radii from the centre): the fast walk under a
    built top tree reports every hit of the box-free fast composition, with its t."""
    scene = sc.scene200(dll, orc, dtype, seed=79)
    rays = sc.scene_rays(scene, 1500, seed=23)
    common, _, _ = sc.compose(scene, rays, range(scene.n), False, False)
    fast, fast_inst, _ = sc.host_walk(scene, rays, False, False)
    lost, of = ia.one_sided(orc, scene, rays, common, fast, fast_inst, False, "benign")
    assert lost == 0 and of > 500
    assert fast["t"].tobytes() == common["t"].tobytes()


def test_fast_mode_axis_aligned_rays_lose_hits_to_the_top_boxes(dll, orc):
    """Pins the inherited behaviour rather than a wish: with a direction component of exactly zero the fast constants are
    inv = copysign(max, d) and -inv * org, which overflows for |org| > 1, so boxes of a built top tree fail and hits are lost; under a
    single-leaf top tree (no top box is tested) the same rays lose nothing to the top level."""
    rng = np.random.default_rng(77)
    geoms = sc.three_geometries(orc, np.float32)
    m = np.array([sc.affine(rng, (3.0 * (k % 4), 3.0 * (k // 4), 0.0)) for k in range(12)])
    scene = sc.Scene(dll, geoms, m.astype(np.float32), np.arange(12, dtype=np.uint32) % 3)
    rays = ia.axis_rays(scene, rng, 1021)
    common, _, _ = sc.compose(scene, rays, range(12), False, False)
    robust, _, _ = sc.host_walk(ia.built_top(scene, orc, (1, 1), (0, 2)), rays, False, True)
    built, built_inst, _ = sc.host_walk(scene, rays, False, False)
    lost, of = ia.one_sided(orc, scene, rays, common, built, built_inst, False, "axis")
    flat, _, _ = sc.host_walk(scene.single_leaf_top(), rays, False, False)
    print(f"axis-aligned rays, 12 instances: the fast composition hits {of}, robust under a built top tree {int((robust['prim'] != INVALID).sum())}, "
          f"fast under a built top tree {of - lost}, fast under a single leaf {int((flat['prim'] != INVALID).sum())}")
    assert sc.same_records(flat, sc.compose(scene, rays, scene.top_ids, False, False)[0])
    assert int((robust["prim"] != INVALID).sum()) == of and robust["t"].tobytes() == sc.compose(scene, rays, range(12), False, True)[0]["t"].tobytes()
    assert lost > 0


# ---- deep stacks: the marker in every tier ---------------------------------------------------------------------------------------------------

def chain_expectation(scene, rays, order, any_hit, robust):
    """The composition in the chain's walk order, and the top tree's share of the counters: closest-hit fetches every top record and
    visits every top leaf; any-hit stops at the first instance with a hit (instance i: i + 1 leaves, min(i + 1, depth) records)."""
    n, depth = scene.n, scene.n - 1
    want, want_inst, cnt = sc.compose(scene, rays, order if not any_hit else range(n), any_hit, robust)
    live = ~sc.nan_flagged(rays)
    if any_hit:
        visited = np.where(want_inst == INVALID, n, want_inst.astype(np.int64) + 1)[live]
        cnt[0] += int(np.minimum(visited, depth).sum())
        cnt[2] += int(visited.sum())
    else:
        cnt[0] += depth * int(live.sum())
        cnt[2] += n * int(live.sum())
    return want, want_inst, cnt


@pytest.mark.parametrize("top_depth,geom_depth", ia.CHAIN_CASES)
def test_chain_top_tree_over_chain_geometry(dll, restatement, top_depth, geom_depth):
    """The marker at stack heights 7 and 8 (LDS / scratch), 63 and 64 (scratch / HBM), a bound of exactly 64 (no Deep kernel), of 65 (the
    first spill: cap 2) and a long spill; the stack bound and the spill's size as the host assembles them from the depths."""
    scene, rays, deep_cap, order = ia.chain_top_scene(dll, restatement, top_depth, geom_depth, 96)
    bound = top_depth + 1 + geom_depth
    assert deep_cap == (bound - 63 if bound > 64 else 0)
    for any_hit, robust in MODES4:
        want, want_inst, want_cnt = chain_expectation(scene, rays, order, any_hit, robust)
        got, inst, cnt = sc.host_walk(scene, rays, any_hit, robust, deep_cap=deep_cap)
        assert sc.same_records(got, want) and (inst == want_inst).all(), (any_hit, robust)
        assert (cnt == want_cnt).all(), (any_hit, robust, cnt, want_cnt)
        hit = got["prim"] != INVALID
        assert hit.sum() >= 16
        if not any_hit:                                        # mostly the nearest triangle of the nearest instance: the deepest of both chains
            deepest = hit & (inst == top_depth)
            assert deepest.sum() >= 0.9 * hit.sum() and (got["prim"][deepest] == geom_depth).all()
            assert cnt[0] >= (top_depth + geom_depth) * hit.sum()
    if bound > 64:
        # The walk holds at most `bound` entries, the last of them at index bound - 1: bound - 64 spill entries are enough, and the
        # host's bound - 64 + 1 has one entry of slack. (So a host that sized the spill bound - 64 would not be caught by any result.)
        want, want_inst, want_cnt = chain_expectation(scene, rays, order, False, True)
        got, inst, cnt = sc.host_walk(scene, rays, False, True, deep_cap=bound - 64)
        assert sc.same_records(got, want) and (inst == want_inst).all() and (cnt == want_cnt).all()
