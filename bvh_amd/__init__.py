"""bvh_amd — MI355X-native BVH construction and traversal behind madmann91/bvh's API.

Host-side mirror of the reference's interface for the hot path (names follow bvh::v2):

    DefaultBuilder.build(bboxes, centers, Config(quality=Quality.High), thread_pool=None) -> Bvh
    BinnedSahBuilder.build / SweepSahBuilder.build
    Bvh.nodes / Bvh.prim_ids / Bvh.serialize() / Bvh.deserialize()
    intersect(bvh, prims, rays, any_hit=False, robust=False) -> hits            (batched Bvh::intersect)
    ray_hit_count / ray_hits(bvh, prims, rays, leaf="tri", robust=False)        (every primitive a ray crosses, in the tree's order, 3D)
    ray_hits_nearest(bvh, prims, rays, k, leaf="tri", robust=False) -> hits, counts (the first k crossings of a ray, front to back, 3D)
    closest_points(bvh, prims, points, max_distance=inf, leaf="tri") -> hits   (nearest primitive per point, 3D)
    sphere_cast(bvh, prims, rays, radius, leaf="tri", robust=False) -> hits     (first contact of a ball swept along each ray, 3D)
    tri_distance(bvh, tris9, query_tris, max_distance=inf) -> hits              (nearest mesh triangle to each query triangle / segment, 3D)
    radius_count / radius_search(bvh, prims, points, radius=r, leaf="tri")      (every primitive within r of each point, 3D)
    knn(bvh, prims, points, k, max_distance=inf, leaf="tri") -> ids, dist, counts (the k nearest primitives per point, sorted, 3D)
    winding_prepare(bvh, prims) -> moments; winding_numbers / occupancy / signed_distance(bvh, prims, moments, points, beta=2) (is a point inside the mesh, 3D)
    overlap_count / overlap_search(bvh, bboxes, query_boxes), self_overlaps(bvh, bboxes) (primitives whose boxes overlap a box; broad phase, 3D)
    tri_intersect_count / tri_intersect_search(bvh, tris9, query_tris), self_intersections(bvh, tris9) (triangles that intersect a triangle; narrow phase, 3D)
    region_count / region_search(bvh, prims, planes, leaf="tri", exact=False), frustum_planes(eye, direction, up, fov_y, aspect, near, far) (primitives inside a set of planes: frusta, slabs, half-spaces, 3D)
    instance_prepare(geometries, transforms) / intersect_instanced(top, geometries, world2obj, rays) (two-level scenes of placed meshes, 3D)
    tri_bounds / precompute_tris / sphere_bounds                                (Tri::get_bbox, PrecomputedTri)

Everything computes in hand-written HIP kernels through the C-ABI of libbvh_amd.so
(include/bvh_amd.h); torch is only used for device memory and streams. There is no CPU fallback.
"""
from .api import (BinnedSahBuilder, MiniTreeBuilder, SplitHeuristic, Bvh, Config, DefaultBuilder, Quality, RayFlags, SweepSahBuilder, ThreadPool, prepare_trace,  # noqa: F401
                  HITD, HITF, INVALID, NODED, NODEF, NODE2D, NODE2F, closest_points, hits_to_numpy, intersect, precompute_tris, sphere_bounds,
                  tri_bounds, gather, radius_count, radius_search, offsets_from_counts, ray_hit_count, ray_hits, ray_hits_nearest, RAY_NEAREST_MAX_K, sphere_cast, knn, KNN_MAX_K, winding_prepare, winding_numbers, signed_distance, occupancy, overlap_count, overlap_search, self_overlaps, tri_intersect_count, tri_intersect_search, self_intersections, tri_distance, region_count, region_search, frustum_planes, REGION_MAX_PLANES, instance_prepare, intersect_instanced, std_sort_ids, radix_sort_pairs, radix_order, reinsertion_stats, last_optimize_profile, pinhole_rays, shade_eyelight)
from ._lib import BvhAmdError  # noqa: F401
