"""Scenes and queries of the winding-number tests (tests/test_winding_host.py, tests/test_gpu_winding.py): plain numpy generators,
at most 4k triangles each. Closed surfaces are oriented with (p1 - p0) x (p2 - p0) pointing outward, so the winding number is 1 inside.
Not a test module."""
import numpy as np

from conftest import load_golden

CLEARANCE = 0.02          # classified queries keep this distance from the ideal surfaces (all of unit scale)


def uv_sphere(stacks=32, slices=64, radius=1.0, center=(0.0, 0.0, 0.0), flip=False):
    """slices * (2 + 2 * (stacks - 2)) triangles (32 x 64: 3968), vertices on the sphere, outward (inward with flip)."""
    th = np.pi * np.arange(stacks + 1) / stacks
    ph = 2 * np.pi * np.arange(slices + 1) / slices
    ph[-1] = 0.0                                              # the seam's vertices are the same numbers
    p = lambda i, j: np.array([np.sin(th[i]) * np.cos(ph[j]), np.sin(th[i]) * np.sin(ph[j]), np.cos(th[i])])
    north, south = np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0])
    tris = []
    for j in range(slices):
        tris.append([north, p(1, j), p(1, j + 1)])
        for i in range(1, stacks - 1):
            a, b, c, d = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            tris.append([a, b, c])
            tris.append([a, c, d])
        tris.append([south, p(stacks - 1, j + 1), p(stacks - 1, j)])
    t = np.asarray(tris, dtype=np.float64) * radius + np.asarray(center, dtype=np.float64)
    if flip:
        t = t[:, [0, 2, 1]]
    return t.reshape(-1, 9)


def torus(major=48, minor=32, R=1.0, r=0.4):
    """2 * major * minor triangles (3072), outward."""
    u = 2 * np.pi * np.arange(major + 1) / major
    v = 2 * np.pi * np.arange(minor + 1) / minor
    u[-1] = v[-1] = 0.0
    p = lambda i, j: np.array([(R + r * np.cos(v[j])) * np.cos(u[i]), (R + r * np.cos(v[j])) * np.sin(u[i]), r * np.sin(v[j])])
    tris = []
    for i in range(major):
        for j in range(minor):
            a, b, c, d = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            tris.append([a, b, c])
            tris.append([a, c, d])
    return np.asarray(tris, dtype=np.float64).reshape(-1, 9)


def shell():
    """A unit sphere and, inside it, a sphere of radius 0.5 facing its own centre: winding 1 in the wall, 0 in the cavity and outside."""
    return np.concatenate([uv_sphere(16, 32), uv_sphere(16, 32, radius=0.5, flip=True)])


def doubled_sphere():
    """Every triangle twice: winding 2 inside."""
    s = uv_sphere(20, 40)
    return np.repeat(s, 2, axis=0)


def hemisphere():
    """The upper half of the sphere: open."""
    s = uv_sphere()
    return s[s.reshape(-1, 3, 3)[:, :, 2].mean(axis=1) > 0]


def holed_sphere():
    """The sphere with every 20th triangle removed."""
    s = uv_sphere()
    return s[np.arange(len(s)) % 20 != 0]


def soup2k():
    return load_golden("soup2k")["prims"].astype(np.float64).reshape(-1, 9)


def _sphere_rule(radius=1.0, inside=1):
    def rule(q):
        d = np.linalg.norm(q, axis=1)
        return np.where(d < radius, inside, 0), np.abs(d - radius)
    return rule


def _torus_rule(q, R=1.0, r=0.4):
    d = np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - R) ** 2 + q[:, 2] ** 2)
    return np.where(d < r, 1, 0), np.abs(d - r)


def _shell_rule(q):
    d = np.linalg.norm(q, axis=1)
    return np.where((d < 1.0) & (d > 0.5), 1, 0), np.minimum(np.abs(d - 1.0), np.abs(d - 0.5))


# name -> (generator, rule or None). A rule maps float64 points to (the winding number of the IDEAL surface, the distance to it): the
# meshes are inscribed within 0.005 of their ideal surfaces, so a point at CLEARANCE or more has the same winding number for both.
SCENES = {
    "sphere": (uv_sphere, _sphere_rule()),
    "torus": (torus, _torus_rule),
    "shell": (shell, _shell_rule),
    "doubled": (doubled_sphere, _sphere_rule(inside=2)),
    "hemisphere": (hemisphere, None),
    "holed": (holed_sphere, None),
    "soup2k": (soup2k, None),
}
CLOSED = ["sphere", "torus", "shell", "doubled"]


def queries(tris9, n=2048, seed=7, rule=None):
    """n points uniform in the scene's box scaled 1.5 about its centre; with a rule, those at least CLEARANCE from the surface and their
    winding numbers. -> (points float64 (m, 3), expected int (m,) or None)"""
    v = tris9.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    q = mid + (np.random.default_rng(seed).random((n, 3)) * 2 - 1) * half
    if rule is None:
        return q, None
    w, dist = rule(q)
    keep = dist >= CLEARANCE
    return q[keep], w[keep]


def solid_angles64(tris9, q):
    """float64 Van Oosterom-Strackee solid angles of every triangle seen from every point: (len(q), len(tris))."""
    t = np.asarray(tris9, dtype=np.float64).reshape(-1, 3, 3)
    out = np.empty((len(q), len(t)))
    for k, p in enumerate(np.asarray(q, dtype=np.float64)):
        a, b, c = t[:, 0] - p, t[:, 1] - p, t[:, 2] - p
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        det = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", a, c) * lb + np.einsum("ij,ij->i", b, c) * la
        out[k] = 2 * np.arctan2(det, den)
    return out


def brute_winding64(tris9, q):
    """(w, sum of |solid angle| / 4 pi) per point, float64, all triangles."""
    om = solid_angles64(tris9, q)
    return om.sum(axis=1) / (4 * np.pi), np.abs(om).sum(axis=1) / (4 * np.pi)
