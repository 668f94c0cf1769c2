"""-m gpu: the refusal of a caller's array that is indexed by original primitive id and too short for the tree's prim ids, through
the raw C entry points, byte for byte: `<who>: <n> <noun> given, but prim_ids refers to primitive <largest> (the array is indexed by
original primitive id)`. Two 3D float trees of 4 primitives (prim ids a permutation of 0..3: the largest is 3), every entry point
that takes such an array refused with 3 rows and served with 4; the instanced query's own sentence; and the cached largest id shared
by two kinds on one tree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -2
TRIS = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [2, 0, 0, 3, 0, 0, 2, 1, 0], [0, 2, 0, 1, 2, 0, 0, 3, 0], [2, 2, 1, 3, 2, 1, 2, 3, 1]], np.float32)
SPHERES = np.array([[0, 0, 0, 0.5], [2, 0, 0, 0.5], [0, 2, 0, 0.5], [2, 2, 1, 0.5]], np.float32)
NOUNS = {"overlap_boxes": "boxes", "overlap_self": "boxes", "intersect_tris": "triangles", "intersect_tris_self": "triangles",
         "tri_distance": "triangles", "region_tris": "primitives", "region_spheres": "primitives", "refit_boxes": "primitives",
         "refit_tris": "primitives"}


class Scene:
    """The two trees, the arrays the entry points read (4 rows each, in HBM) and one query of every kind."""

    def __init__(self):
        import torch
        import bvh_amd
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        self.tris, self.spheres = dev(TRIS), dev(SPHERES)
        self.tri_boxes, tri_centers = bvh_amd.tri_bounds(self.tris)
        self.sphere_boxes, sphere_centers = bvh_amd.sphere_bounds(self.spheres)
        self.tri_tree = bvh_amd.DefaultBuilder.build(self.tri_boxes, tri_centers)
        self.sphere_tree = bvh_amd.DefaultBuilder.build(self.sphere_boxes, sphere_centers)
        for tree in (self.tri_tree, self.sphere_tree):
            assert sorted(tree.prim_ids.tolist()) == [0, 1, 2, 3]
        self.box = dev([[-1, -1, -1, 4, 4, 4]])                                   # one query box, triangle and region (a half space)
        self.tri = dev([[0, 0, -1, 3, 0, 2, 0, 3, 2]])
        self.plane = dev([[0, 0, 1, -10]])
        self.counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.hits = torch.zeros((1, 4), dtype=torch.float32, device="cuda")

    def call(self, name, n_src):
        """The raw entry point `name` with n_src rows announced for its by-id array: the return code."""
        from bvh_amd import _lib
        fn = getattr(_lib.load(), f"bvh3f_{name}")
        t, s, cnt = self.tri_tree._h, self.sphere_tree._h, self.counts.data_ptr()
        if name == "overlap_boxes":
            return fn(t, self.tri_boxes.data_ptr(), n_src, self.box.data_ptr(), 1, 0, cnt, None, None, None, None)
        if name == "overlap_self":
            return fn(t, self.tri_boxes.data_ptr(), n_src, 0, cnt, None, None, None, None)
        if name == "intersect_tris":
            return fn(t, self.tris.data_ptr(), n_src, self.tri.data_ptr(), 1, 0, cnt, None, None, None, None)
        if name == "intersect_tris_self":
            return fn(t, self.tris.data_ptr(), n_src, 0, cnt, None, None, None, None)
        if name == "tri_distance":
            return fn(t, self.tris.data_ptr(), n_src, self.tri.data_ptr(), 1, float("inf"), None, 0, self.hits.data_ptr(), None, None, None)
        if name == "region_tris":
            return fn(t, self.tris.data_ptr(), n_src, self.plane.data_ptr(), 1, 1, 0, cnt, None, None, None, None, None)
        if name == "region_spheres":
            return fn(s, self.spheres.data_ptr(), n_src, self.plane.data_ptr(), 1, 1, 0, cnt, None, None, None, None, None)
        if name == "refit_boxes":
            return fn(s, self.sphere_boxes.data_ptr(), n_src, None)
        assert name == "refit_tris"
        return fn(t, self.tris.data_ptr(), n_src, None, None)


@pytest.fixture(scope="module")
def scene():
    return Scene()


def refusal(who, n, noun, largest=3):
    return f"{who}: {n} {noun} given, but prim_ids refers to primitive {largest} (the array is indexed by original primitive id)"


@pytest.mark.parametrize("name", list(NOUNS))
def test_short_array_refused_full_array_served(scene, name):
    import torch
    from bvh_amd import _lib
    rc = scene.call(name, 3)
    message = _lib.last_error()
    print(name, rc, repr(message))
    assert rc == ERR_ARG
    assert message.encode() == refusal(name, 3, NOUNS[name]).encode()
    assert scene.call(name, 4) == 0, _lib.last_error()
    torch.cuda.synchronize()


def test_instanced_keeps_its_own_sentence(scene):
    import torch
    import bvh_amd
    from bvh_amd import _lib
    prims12 = bvh_amd.precompute_tris(scene.tris, scene.tri_tree.device_prim_ids())
    moves = np.zeros((4, 12), np.float32)
    moves[:, [0, 5, 10]] = 1                                                      # identity, translated along x
    moves[:, 3] = 10 * np.arange(4)
    world2obj, boxes, centers = bvh_amd.instance_prepare([(scene.tri_tree, prims12)], moves)
    top = bvh_amd.DefaultBuilder.build(boxes, centers)
    assert sorted(top.prim_ids.tolist()) == [0, 1, 2, 3]
    table = (_lib.Geometry * 1)()
    table[0].bvh, table[0].d_tris12 = scene.tri_tree._h, prims12.data_ptr()
    rays = torch.tensor([[0.25, 0.25, -5, 0, 0, 1, 0, 100]], dtype=torch.float32, device="cuda")
    instances = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda n_instances: _lib.load().bvh3f_intersect_rays_instanced(top._h, table, 1, world2obj.data_ptr(), None, n_instances, rays.data_ptr(), 1, 0,
                                                                          scene.hits.data_ptr(), instances.data_ptr(), None, None)
    rc = call(3)
    message = _lib.last_error()
    print(rc, repr(message))
    assert rc == ERR_ARG
    assert message.encode() == b"intersect_rays_instanced: 3 instances given, but the top tree's prim_ids refer to instance 3"
    assert call(4) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert int(instances[0]) == 0


def test_cached_largest_id_serves_another_kind():
    import torch
    from bvh_amd import _lib
    fresh = Scene()                                                              # no entry point has asked this tree for its largest id yet
    assert fresh.call("intersect_tris", 3) == ERR_ARG
    assert _lib.last_error() == refusal("intersect_tris", 3, "triangles")
    assert fresh.call("overlap_boxes", 4) == 0, _lib.last_error()
    assert fresh.call("overlap_boxes", 3) == ERR_ARG
    assert _lib.last_error() == refusal("overlap_boxes", 3, "boxes")
    torch.cuda.synchronize()
    assert int(fresh.counts[0]) == 4                                              # the query box holds all four boxes
