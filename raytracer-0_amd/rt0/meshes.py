"""Procedural triangle models for TRIANGLE scene entries.

BASELINE config 5 names a ~100k-triangle model (the reference's Happy Buddha
OBJ is git-ignored and absent): `icosphere(6)` (81,920 triangles)
stands in for it, as SURVEY suggests.  `wavy_icosphere` displaces the sphere
so that rays graze many triangles at different depths (a harder BVH case).
"""
import numpy as np


def icosphere(level, radius=1.0):
    """Unit icosahedron subdivided `level` times, projected onto the sphere:
    20 * 4**level triangles, counter-clockwise seen from outside.
    Returns (positions float32 [nv, 3], triangles int32 [nt, 3])."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = list(f)
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        nf = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return (np.array(verts) * radius).astype(np.float32), np.array(faces, np.int32)


def wavy_icosphere(level, radius=1.0, amp=0.08, freq=6.0):
    """icosphere displaced along the normal by amp*sin(freq*x)*sin(freq*y)*sin(freq*z)."""
    v, f = icosphere(level)
    p = v.astype(np.float64)
    s = 1.0 + amp * np.sin(freq * p[:, 0]) * np.sin(freq * p[:, 1]) * np.sin(freq * p[:, 2])
    return (p * (s * radius)[:, None]).astype(np.float32), f


def world_triangles(positions, triangles, pos, scale):
    """World-space triangle vertices [nt, 9] of an instance (pos + scale * v), in
    the float32 arithmetic of librt0's BVH input (rt0_host.cpp build_bvh)."""
    v = np.asarray(positions, np.float32)[np.asarray(triangles).reshape(-1)]
    w = np.asarray(pos, np.float32)[None, :] + np.float32(scale) * v
    return w.astype(np.float32).reshape(-1, 9)


# ---------------------------------------------------------------- hard meshes
# Small models that stress the BVH builders and the walk where the icospheres
# do not: axis-aligned faces (zero-thickness boxes), duplicates, degenerate
# triangles, slivers, a small model inside a huge one (tests/test_trace.py).

def _soup(tris):
    """[nt, 3, 3] vertex triples -> (positions [3 nt, 3] float32, triangles int32 [nt, 3])."""
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def single_triangle():
    return _soup([[(-1.0, -0.5, 0.25), (1.0, -0.75, -0.5), (0.125, 1.0, 0.5)]])


def cube(half=1.0):
    """Axis-aligned cube of 12 triangles, counter-clockwise seen from outside."""
    h = float(half)
    v = np.array([(x, y, z) for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))]
    return v, np.array(t, np.int32)


def quad_grid(n, axis=2, half=1.0, level=0.25):
    """n x n quads (2 n^2 right triangles with legs on the axes) in the plane
    coordinate[axis] = level, spanning [-half, half]^2 on the other two axes."""
    g = np.linspace(-half, half, n + 1)
    a, b = np.meshgrid(g, g, indexing="ij")
    p = np.zeros((n + 1, n + 1, 3))
    p[..., (axis + 1) % 3] = a
    p[..., (axis + 2) % 3] = b
    p[..., axis] = level
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    q00, q10, q11, q01 = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    t = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])
    return p.reshape(-1, 3).astype(np.float32), t.astype(np.int32)


def repeated(model, times):
    """Every triangle of a model `times` times."""
    v, t = model
    return v, np.repeat(t, times, axis=0)


def stadium():
    """A 24 x 24 grid scaled 0.3 over two 80-unit triangles: a small model
    inside a huge one."""
    v, t = quad_grid(24, axis=1, half=0.3, level=0.0)
    big = np.array([(-40, -0.5, -40), (40, -0.5, -40), (40, -0.5, 40), (-40, -0.5, 40)], np.float32)
    tb = np.array([(0, 2, 1), (0, 3, 2)], np.int32) + len(v)
    return np.concatenate([v, big]), np.concatenate([t, tb])


def slivers(n=400, length=2.0, width=0.01, seed=7):
    """n randomly placed and oriented slivers (length x width)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 3))
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(a, rng.normal(size=(n, 3)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    tris = np.stack([c - 0.5 * length * a, c + 0.5 * length * a, c + width * b], 1)
    return _soup(tris)


def concentric(n=48, first=1e-3, growth=1.25, level=0.5):
    """n coplanar triangles around one centroid, sizes growing geometrically,
    each turned by the golden angle."""
    tris = []
    for k in range(n):
        r, ph = first * growth ** k, 2.399963229728653 * k
        ang = ph + np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
        tris.append(np.stack([r * np.cos(ang), r * np.sin(ang), np.full(3, level)], -1))
    return _soup(tris)


def cube_with_degenerates():
    """The cube plus four degenerate triangles: a repeated vertex, a zero
    edge (the last two vertices equal), collinear vertices, all three equal."""
    v, t = cube()
    extra = np.array([(0.5, 0.25, 0.125), (-0.25, 0.5, 0.75), (0.125, 0.375, 0.4375)], np.float32)
    k = len(v)
    v = np.concatenate([v, extra])
    deg = np.array([(k, k, k + 1), (k, k + 1, k + 1), (k, k + 2, k + 1), (k + 2, k + 2, k + 2)], np.int32)
    return v, np.concatenate([t, deg])


def menagerie():
    """name -> (positions, triangles) of the hard models."""
    return {
        "triangle": single_triangle(),
        "triangle_twice": repeated(single_triangle(), 2),
        "cube": cube(),
        "grid_x": quad_grid(32, 0),
        "grid_y": quad_grid(32, 1),
        "grid_z": quad_grid(32, 2),
        "grid_thrice": repeated(quad_grid(8, 2), 3),
        "stadium": stadium(),
        "slivers": slivers(),
        "concentric": concentric(),
        "cube_degenerate": cube_with_degenerates(),
        "wavy_icosphere": wavy_icosphere(2),
    }
