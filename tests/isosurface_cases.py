"""Marching tetrahedra on the Kuhn split, restated in vectorised NumPy from the specification in include/dfnet_hip.h (not from the
kernel), and the analytic fields the iso-surface tests use.

The restatement shares the kernel's definitions and none of its code: the inside rule `sigma >= iso` in fp32 (NaN outside), the six
tetrahedra per cell in the lexicographic order of the axis permutations, the edge keys id(lower node) * 7 + type, vertex ids = ranks
of the crossed edges in key order, `t` in fp32, the case rules for k = 1, 2, 3 inside vertices and a winding table made on the unit
cell with every crossing at the edge midpoint.  Positions are formed in float64 from the same fp32 axes and the fp32 `t`, so the
kernel's fp32 positions sit within a derived rounding bound of them (tests/test_gpu_isosurface.py)."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))          # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx = tet 0..5


def tet_vertices(tet):
    """The four corners of tet `tet` as 0/1 offsets: v0 = 0, v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1)."""
    a, b, _ = PERMS[tet]
    v = np.zeros((4, 3), int)
    v[1, a] = 1
    v[2, a] = v[2, b] = 1
    v[3] = 1
    return v


def case_triangles(tet, mask):
    """[(edge, edge, edge)] of tet `tet` whose inside vertices are the bits of `mask`; an edge is a pair of tet-vertex indices.  The
    winding comes from the unit cell with every crossing at the edge midpoint: the normal points from the inside vertices to the
    outside ones; where the rule's own order points the other way its last two corners are exchanged."""
    ins = [v for v in range(4) if mask >> v & 1]
    out = [v for v in range(4) if not mask >> v & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (p, q), (r, s) = ins, out
        A, B, C, D = (p, r), (p, s), (q, s), (q, r)
        tris = [(A, B, C), (A, C, D)]
    else:
        w = ins[0] if len(ins) == 1 else out[0]
        tris = [tuple((w, u) for u in range(4) if u != w)]
    corners = tet_vertices(tet).astype(float)
    toward = corners[out].mean(0) - corners[ins].mean(0)
    wound = []
    for tri in tris:
        P = [(corners[x] + corners[y]) / 2 for x, y in tri]
        dot = float(np.cross(P[1] - P[0], P[2] - P[0]) @ toward)
        assert abs(dot) > 1e-9
        wound.append(tri if dot > 0 else (tri[0], tri[2], tri[1]))
    return wound


CASES = [[case_triangles(tet, m) for m in range(16)] for tet in range(6)]


def marching_tets(sigma, axes, iso):
    """(verts float64 [V,3], faces int64 [F,3], t float32 [V], ends int64 [V,2] = the node ids of every vertex's edge)."""
    sigma = np.ascontiguousarray(sigma, dtype=np.float32)
    nx, ny, nz = sigma.shape
    xs, ys, zs = (np.asarray(a, dtype=np.float32) for a in axes)
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    iso = np.float32(iso)
    inside = sigma >= iso                                   # NaN compares false: outside
    ids = np.arange(nx * ny * nz, dtype=np.int64).reshape(nx, ny, nz)
    keys, lo_ids, hi_ids = [], [], []
    for typ in range(7):
        dx, dy, dz = (typ + 1) & 1, (typ + 1) >> 1 & 1, (typ + 1) >> 2 & 1
        lo = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        hi = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        crossed = inside[lo] != inside[hi]
        keys.append(ids[lo][crossed] * 7 + typ)
        lo_ids.append(ids[lo][crossed])
        hi_ids.append(ids[hi][crossed])
    keys, lo_ids, hi_ids = (np.concatenate(a) for a in (keys, lo_ids, hi_ids))
    order = np.argsort(keys, kind="stable")
    keys, lo_ids, hi_ids = keys[order], lo_ids[order], hi_ids[order]
    flat = sigma.reshape(-1)
    s_a, s_b = flat[lo_ids], flat[hi_ids]
    with np.errstate(all="ignore"):
        t = (iso - s_a) / (s_b - s_a)                       # float32 throughout
        t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(1))).astype(np.float32)

    def position(node):
        i, rem = np.divmod(node, ny * nz)
        j, k = np.divmod(rem, nz)
        return np.stack([xs[i], ys[j], zs[k]], -1).astype(np.float64)
    pa, pb = position(lo_ids), position(hi_ids)
    verts = pa + t.astype(np.float64)[:, None] * (pb - pa)
    # faces: per cell (the id of its lowest node), tet, triangle
    cell = ids[:nx - 1, :ny - 1, :nz - 1].reshape(-1)
    rows = []
    for tet in range(6):
        corner = tet_vertices(tet)
        node = np.stack([cell + (c[0] * ny + c[1]) * nz + c[2] for c in corner], -1)       # [cells, 4]
        code = corner[:, 0] + 2 * corner[:, 1] + 4 * corner[:, 2]
        ins = inside.reshape(-1)[node]
        mask = (ins * (1 << np.arange(4))).sum(-1)
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if sel.size == 0:
                continue
            for ti, tri in enumerate(CASES[tet][m]):
                vid = []
                for x, y in tri:
                    lo_v, hi_v = min(x, y), max(x, y)
                    key = node[sel, lo_v] * 7 + ((code[hi_v] ^ code[lo_v]) - 1)
                    at = np.searchsorted(keys, key)
                    assert (keys[at] == key).all()
                    vid.append(at)
                rows.append(np.stack([cell[sel], np.full(sel.size, tet), np.full(sel.size, ti)] + vid, -1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        faces = rows[:, 3:].astype(np.int64)
    else:
        faces = np.zeros((0, 3), np.int64)
    return verts, faces, t, np.stack([lo_ids, hi_ids], -1)


def canonical_faces(faces):
    """Every triangle rotated to start at its smallest id, the list sorted: equal for equal oriented surfaces in any face order."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    r = np.argmin(f, 1)
    f = np.stack([f[np.arange(len(f)), (r + s) % 3] for s in range(3)], -1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def surface_invariants(verts, faces):
    """dict(closed = every directed edge once and its reverse once, euler = V - E + F, volume = signed, all_used = every vertex id
    referenced) of an indexed triangle list; positions only enter the volume."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    V = v.shape[0]
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    dk = d[:, 0] * max(V, 1) + d[:, 1]
    rk = d[:, 1] * max(V, 1) + d[:, 0]
    uniq, counts = np.unique(dk, return_counts=True)
    closed = bool((counts == 1).all() and np.array_equal(uniq, np.unique(rk)))
    E = len(np.unique(np.minimum(dk, rk)))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)
    return {"closed": closed, "euler": V - E + f.shape[0], "volume": volume,
            "all_used": bool(np.array_equal(np.unique(f), np.arange(V)))}


# ------------------------------------------------------------------------------------------------ the fields
def linspace_axes(bounds, shape):
    x0, y0, z0, x1, y1, z1 = bounds
    return tuple(np.linspace(a, b, n).astype(np.float32) for a, b, n in ((x0, x1, shape[0]), (y0, y1, shape[1]), (z0, z1, shape[2])))


def mesh(axes):
    return np.meshgrid(*(a.astype(np.float64) for a in axes), indexing="ij")


SPHERE_R = 0.7


def sphere():
    """R^2 - |x|^2, R = 0.7, on 12 x 10 x 9 over [-1,1]^3: closed, Euler characteristic 2."""
    axes = linspace_axes((-1, -1, -1, 1, 1, 1), (12, 10, 9))
    X, Y, Z = mesh(axes)
    return (SPHERE_R ** 2 - (X * X + Y * Y + Z * Z)).astype(np.float32), axes, 0.0


def torus():
    """Major radius 0.6, minor 0.25, on 16 x 15 x 9 over [-1,1]^2 x [-.5,.5]: closed, Euler characteristic 0; a few exact ties."""
    axes = linspace_axes((-1, -1, -.5, 1, 1, .5), (16, 15, 9))
    X, Y, Z = mesh(axes)
    return (0.25 ** 2 - ((np.sqrt(X * X + Y * Y) - 0.6) ** 2 + Z * Z)).astype(np.float32), axes, 0.0


def two_spheres():
    """Two disjoint balls (radius 0.3 about (-.5,0,0) and 0.25 about (.45,.1,-.05)) on 14 x 9 x 8: closed, Euler characteristic 4."""
    axes = linspace_axes((-1, -.5, -.5, 1, .5, .5), (14, 9, 8))
    X, Y, Z = mesh(axes)
    a = 0.3 ** 2 - ((X + .5) ** 2 + Y * Y + Z * Z)
    b = 0.25 ** 2 - ((X - .45) ** 2 + (Y - .1) ** 2 + (Z + .05) ** 2)
    return np.maximum(a, b).astype(np.float32), axes, 0.0


def integer_axes(shape):
    return tuple(np.arange(n, dtype=np.float32) for n in shape)


def tilted_plane():
    """2.5 - x + 0.25 y on 5 x 6 x 7 with integer axes: an open surface, exact in fp32."""
    axes = integer_axes((5, 6, 7))
    X, Y, Z = mesh(axes)
    return (2.5 - X + 0.25 * Y).astype(np.float32), axes, 0.0


def plane_through_nodes():
    """2 - x on 5 x 4 x 3 with integer axes: the surface passes through the nodes x = 2 (ties: zero-area triangles)."""
    axes = integer_axes((5, 4, 3))
    X, Y, Z = mesh(axes)
    return (2.0 - X).astype(np.float32), axes, 0.0


def constant(value):
    axes = integer_axes((4, 4, 4))
    return np.full((4, 4, 4), value, np.float32), axes, 0.5


def one_corner():
    """2 x 2 x 2 with node (0,0,0) inside: the corner every one of the six tetrahedra shares, so 6 triangles."""
    s = np.zeros((2, 2, 2), np.float32)
    s[0, 0, 0] = 1.0
    return s, integer_axes((2, 2, 2)), 0.25


def trig(shape, seed=0):
    """A many-component field: a sum of three sinusoid products, threshold 0.1."""
    axes = linspace_axes((-1, -1, -1, 1, 1, 1), shape)
    X, Y, Z = mesh(axes)
    f = np.sin(7.3 * X + seed) * np.cos(5.1 * Y) + np.sin(6.7 * Z + 0.4) * np.cos(4.3 * X) + 0.5 * np.sin(9.1 * Y * Z + 0.2)
    return f.astype(np.float32), axes, 0.1


def with_nans():
    """The trigonometric field on 9 x 8 x 7 with every 11th node NaN (and one +inf, one -inf): NaN is outside."""
    s, axes, iso = trig((9, 8, 7), seed=1)
    flat = s.reshape(-1).copy()
    flat[::11] = np.nan
    flat[5], flat[17] = np.inf, -np.inf
    return flat.reshape(s.shape), axes, iso


def non_uniform():
    """A sphere-like field on axes with irregular spacing (coordinates are looked up, never recomputed from bounds)."""
    rng = np.random.default_rng(3)
    axes = tuple(np.cumsum(rng.uniform(0.05, 0.4, n)).astype(np.float32) - off for n, off in ((8, 1.0), (7, .8), (9, 1.1)))
    X, Y, Z = mesh(axes)
    return (0.5 - (X * X + 1.5 * Y * Y + 0.7 * Z * Z)).astype(np.float32), axes, 0.0
