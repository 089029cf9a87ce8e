"""CHECKER ONLY — NumPy float64 restatement of include/invr_surface.h's contract: the closest point on a triangle mesh (Ericson's
region walk with the header's operation order, the lexicographic (key, face) minimum over ALL faces) and the barycentric
interpolation, plus the mesh builders of the tests.  psbody.mesh / CGAL (tools/prepare_zjumocap.py:177-240, 312-400 of the reference)
are not available, so the reference of the tests is the contract's own brute force, chunked over the lattice points.

NumPy's element-wise +, -, *, / and sqrt on float64 are single IEEE operations, rounded separately: an expression written with the
header's parentheses has the header's bits.  Every quantity of the walk is evaluated for every (point, face) and the first region whose
condition holds selects among them, which is the walk's result."""
import numpy as np

from tests.posescene_reference import lattice, lattice_points          # noqa: F401  (the lattice rule is include/invr_posescene.h's)

CLAMPED = 8          # region code of a region-7 result whose (v, w) the clamp changed


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def closest_on_faces(p, a, b, c):
    """p (P,1,3) or (P,3)[:, None]; a, b, c (1,F,3) float64 corners -> key, u, v, w, region, each (P,F)."""
    P = [p[..., k] for k in range(3)]
    A, B, C = ([x[..., k] for k in range(3)] for x in (a, b, c))
    ab = [B[k] - A[k] for k in range(3)]
    ac = [C[k] - A[k] for k in range(3)]
    ap = [P[k] - A[k] for k in range(3)]
    bp = [P[k] - B[k] for k in range(3)]
    cp = [P[k] - C[k] for k in range(3)]
    with np.errstate(all='ignore'):
        d1, d2 = dot(ab, ap), dot(ac, ap)
        d3, d4 = dot(ab, bp), dot(ac, bp)
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        in1 = (d1 <= 0) & (d2 <= 0)
        left = ~in1
        in2 = left & (d3 >= 0) & (d4 <= d3)
        left &= ~in2
        in3 = left & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        left &= ~in3
        in4 = left & (d6 >= 0) & (d5 <= d6)
        left &= ~in4
        in5 = left & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        left &= ~in5
        in6 = left & (va <= 0) & (e >= 0) & (g >= 0)
        in7 = left & ~in6
        v3 = d1 / (d1 - d3)
        w5 = d2 / (d2 - d6)
        w6 = e / (e + g)
        den = 1.0 / ((va + vb) + vc)
        v7r, w7r = vb * den, vc * den
        v7 = np.where(v7r > 0, v7r, 0.0)
        v7 = np.where(v7 < 1, v7, 1.0)
        w7 = np.where(w7r > 0, w7r, 0.0)
        w7 = np.where(w7 < 1.0 - v7, w7, 1.0 - v7)
        clamped = in7 & ~((v7 == v7r) & (w7 == w7r))
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        v = np.select([in1, in2, in3, in4, in5, in6], [zero, one, v3, zero, zero, 1.0 - w6], v7)
        w = np.select([in1, in2, in3, in4, in5, in6], [zero, zero, zero, one, w5, w6], w7)
        u = np.select([in1, in2, in3, in4, in5, in6], [one, zero, 1.0 - v3, zero, 1.0 - w5, zero], (1.0 - v7) - w7)
        q = [(A[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        for k in range(3):
            q[k] = np.select([in1, in2, in4], [A[k] + zero, B[k] + zero, C[k] + zero], q[k])
        ex, ey, ez = P[0] - q[0], P[1] - q[1], P[2] - q[2]
        key = (ex * ex + ey * ey) + ez * ez
    region = np.select([in1, in2, in3, in4, in5, in6, clamped], [1, 2, 3, 4, 5, 6, CLAMPED], 7).astype(np.int8)
    return key, u, v, w, region


def closest_scalar(p, a, b, c):
    """The header's walk read line by line for ONE point and ONE face (Python floats are IEEE doubles) -> (key, (u, v, w), region):
    what the vectorised form is held against in tests/test_surface_reference_cpu.py."""
    p, a, b, c = ([float(t) for t in x] for x in (p, a, b, c))
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]

    def div(x, y):                                    # (the IEEE quotient also where Python's own division raises)
        with np.errstate(all='ignore'):
            return float(np.float64(x) / np.float64(y))

    def finish(u, v, w, region, corner=None):
        ab, ac = sub(b, a), sub(c, a)
        q = corner if corner is not None else [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        e = sub(p, q)
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], (u, v, w), region
    ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return finish(1.0, 0.0, 0.0, 1, a)
    bp = sub(p, b)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return finish(0.0, 1.0, 0.0, 2, b)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        v = div(d1, d1 - d3)
        return finish(1.0 - v, v, 0.0, 3)
    cp = sub(p, c)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return finish(0.0, 0.0, 1.0, 4, c)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = div(d2, d2 - d6)
        return finish(1.0 - w, 0.0, w, 5)
    va = d3 * d6 - d5 * d4
    e, g = d4 - d3, d5 - d6
    if va <= 0 and e >= 0 and g >= 0:
        w = div(e, e + g)
        return finish(0.0, 1.0 - w, w, 6)
    den = div(1.0, (va + vb) + vc)
    v0, w0 = vb * den, vc * den
    v = v0 if v0 > 0 else 0.0
    v = v if v < 1 else 1.0
    w = w0 if w0 > 0 else 0.0
    w = w if w < 1.0 - v else 1.0 - v
    return finish((1.0 - v) - w, v, w, 7 if (v == v0 and w == w0) else CLAMPED)


def brute_force(verts, faces, points, budget=1 << 17, with_ties=False):
    """The contract over ALL faces for each float64 point -> (face int32, bary (n,3) float64, dist float32, region int8 of the
    winner (0 where face = -1)[, the number of faces holding the winner's key])."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    points = np.asarray(points, np.float64)
    ok = ((faces >= 0) & (faces < len(v))).all(axis=1)
    ids = np.nonzero(ok)[0]                              # ascending: argmin's first minimum is the lowest face
    n = len(points)
    face = np.full(n, -1, np.int32)
    bary = np.zeros((n, 3), np.float64)
    dist = np.full(n, np.inf, np.float32)
    region = np.zeros(n, np.int8)
    ties = np.zeros(n, np.int64)
    if len(ids):
        a, b, c = (v[faces[ids, k]][None] for k in range(3))
        chunk = max(1, budget // len(ids))
        for s in range(0, n, chunk):
            p = points[s:s + chunk, None, :]
            key, uu, vv, ww, reg = closest_on_faces(p, a, b, c)
            key = np.where(np.isnan(key), np.inf, key)
            j = np.argmin(key, axis=1)
            at = np.arange(len(j))
            best = key[at, j]
            won = np.isfinite(best)
            sl = slice(s, s + len(j))
            face[sl] = np.where(won, ids[j], -1)
            bary[sl] = np.where(won[:, None], np.stack([uu[at, j], vv[at, j], ww[at, j]], axis=1), 0.0)
            dist[sl] = np.sqrt(best).astype(np.float32)
            region[sl] = np.where(won, reg[at, j], 0)
            ties[sl] = np.where(won, (key == best[:, None]).sum(axis=1), 0)
    return (face, bary, dist, region, ties) if with_ties else (face, bary, dist, region)


def interpolate(attr, faces, face, bary):
    """barycentric_interpolation (prepare_zjumocap.py:167-175) as the header states it -> (n, C) float32; face = -1 gives 0."""
    attr = np.asarray(attr, np.float32).astype(np.float64)
    attr = attr.reshape(len(attr), -1)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    face = np.asarray(face, np.int64)
    ok = (face >= 0) & (face < len(faces))
    idx = faces[np.where(ok, face, 0)]
    ok &= ((idx >= 0) & (idx < len(attr))).all(axis=1)
    idx = np.where(ok[:, None], idx, 0)
    u, v, w = (np.asarray(bary, np.float64)[:, k, None] for k in range(3))
    out = ((u * attr[idx[:, 0]] + v * attr[idx[:, 1]]) + w * attr[idx[:, 2]]).astype(np.float32)
    return np.where(ok[:, None], out, np.float32(0))


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
ORIGIN, STEP = np.array([-0.37, 0.11, 1.03]), np.array([0.025, 0.03, 0.02])
DYADIC_ORIGIN, DYADIC_STEP = np.array([-1.0, 0.5, 2.0]), np.array([0.125, 0.125, 0.125])
MESHES = ['tri1', 'tet', 'soup63', 'soup64', 'soup65', 'soup1000', 'big', 'identical', 'dyadic_octahedron', 'degenerate', 'all_degenerate',
          'sliver', 'far', 'unreferenced']


# In double, with float32 corners, no aspect ratio a float32 mesh can hold (1e-7) makes Ericson's walk inconsistent enough to need the
# clamp: measured over 1e7 (point, sliver) pairs, region 7 is hardly reached and never with (v, w) outside the triangle.  Exactly
# collinear corners a, a + 3 d, a + 4 d do it for points abeam of the far segment (va + vb + vc is pure rounding noise there): about 4
# in 1e6 pairs.  These four (a, d in units of 2^-12 m, found by a seeded search with this restatement) reach the clamp AS WINNERS at
# points of the lattice ORIGIN + i * STEP, i < (17, 9, 33), among the other faces of mesh('sliver', ...).
NEEDLES = [([-1302, 1420, 5496], [-55, -72, -415]), ([-49, 2357, 6306], [28, -604, -332]), ([-1445, -135, 6216], [89, 79, 180]),
           ([713, -155, 6445], [-452, 475, -331])]


def soup(g, n, lo, hi, size=0.03, pad=0.05):
    """n small triangles with their own three vertices each, centres uniform over the box."""
    centre = g.uniform(lo - pad, hi + pad, (n, 1, 3))
    verts = (centre + g.uniform(-size, size, (n, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n).reshape(n, 3)


def mesh(name, dims):
    """-> (verts (V,3) float32, faces (F,3) int32, origin, step) of mesh `name` over the lattice `dims`, seeded by both."""
    g = np.random.RandomState(sum(map(ord, name)) * 1000 + dims[0] * 97 + dims[1] * 13 + dims[2])
    origin, step = (DYADIC_ORIGIN, DYADIC_STEP) if name == 'dyadic_octahedron' else (ORIGIN, STEP)
    lo, hi = origin, origin + (np.array(dims) - 1) * step
    mid, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 0.1)
    if name == 'tri1':                                # small, in the middle of the box, in general position: points on every side of it
        v = mid[None] + np.array([[-0.06, -0.03, -0.05], [0.07, -0.02, 0.03], [-0.01, 0.05, 0.08]]) + g.uniform(-0.005, 0.005, (3, 3))
        f = np.array([[0, 1, 2]])
    elif name == 'tet':
        v = mid[None] + 0.08 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) + g.uniform(-0.005, 0.005, (4, 3))
        f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    elif name.startswith('soup'):
        v, f = soup(g, int(name[4:]), lo, hi)
    elif name == 'big':                               # every triangle spans the lattice: a candidate in every tile
        corners = np.stack([lo - 0.2 * ext, np.array([hi[0], lo[1], hi[2]]) + 0.2 * ext * [1, -1, 1], hi + 0.2 * ext], axis=0)
        v = (corners[None] + g.uniform(-0.1, 0.1, (300, 3, 3)) * ext).reshape(-1, 3)
        f = np.arange(900).reshape(300, 3)
    elif name == 'identical':
        v, _ = soup(g, 1, lo, hi)
        f = np.repeat(np.array([[0, 1, 2]]), 1000, axis=0)
    elif name == 'dyadic_octahedron':                 # corners ON lattice points, two steps from a lattice point along each axis
        centre = origin + (np.array(dims) // 2) * step
        v = np.concatenate([centre[None] + s * 2 * step[a] * np.eye(3)[a][None] for a in range(3) for s in (1, -1)])
        f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    elif name == 'degenerate':
        v, f = soup(g, 30, lo, hi)
        line = mid[None] + np.array([[-0.05, 0, 0], [0.0, 0, 0], [0.075, 0, 0]])          # exactly collinear: they differ in x only
        V = len(v) + 3
        extra = [[90, 90, 91], [0, 0, 0], [3, 4, 4], [5, 4, 5], [92, 91, 90], [90, 92, 91], [91, 91, 91],          # a == b, a == b == c, collinear
                 [-1, 0, 1], [0, -1, 1], [0, 1, -1], [V, 0, 1], [0, V, 1], [0, 1, V], [-1, -1, -1], [V, V, V], [2 ** 31 - 1, 0, 1], [-2 ** 31, 3, 4]]
        v = np.concatenate([v, line])
        f = np.concatenate([f, np.array(extra, np.int64)])
        f = f[g.permutation(len(f))]
    elif name == 'all_degenerate':                    # no face takes part
        v, _ = soup(g, 4, lo, hi)
        V = len(v)
        f = np.array([[-1, 0, 1], [0, V, 1], [2, 3, -5], [V + 7, 0, 0], [-1, -1, -1], [V, V, V]] * 20)
    elif name == 'sliver':
        # normal triangles among slivers: long edge ~1 m along x through the box, apex off the edge by ratio * length but at least one
        # float32 step — aspect ratios from 1e-2 down to 1e-7
        v, f = soup(g, 40, lo, hi)
        sl = []
        for ratio in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-7, 1e-7):
            a = np.array([lo[0] - 0.5, g.uniform(lo[1], hi[1]), g.uniform(lo[2], hi[2])]).astype(np.float32)
            b = (a + np.array([1.0 + g.uniform(0, 0.2), 0, 0])).astype(np.float32)
            c = (a.astype(np.float64) + g.uniform(0.2, 0.8) * (b.astype(np.float64) - a)).astype(np.float32)
            k = 1 + int(g.randint(2))
            c[k] = np.nextafter(c[k], np.float32(np.inf)) if ratio < 2e-7 else np.float32(c[k] + ratio * (b[0] - a[0]))
            sl += [a, b, c]
        for a, d in NEEDLES:
            a, d = np.array(a) / 4096.0, np.array(d) / 4096.0
            sl += [a, a + 3 * d, a + 4 * d]
        f = np.concatenate([f, len(v) + np.arange(len(sl)).reshape(-1, 3)])
        v = np.concatenate([v, np.array(sl, np.float64)])
        f = f[g.permutation(len(f))]
    elif name == 'far':
        v, f = soup(g, 200, lo, hi)
        v = v + np.array([0.0, 10.0, 0.0])
    elif name == 'unreferenced':                      # the mesh 0.5 m off the box; vertices no face uses INSIDE the box
        v, f = soup(g, 50, lo, hi)
        v = np.concatenate([v + np.array([0.0, 0.0, ext[2] + 0.5]), g.uniform(lo, hi, (50, 3))])
        order = g.permutation(len(v))                 # (scattered through the rows)
        inv = np.argsort(order)
        v, f = v[order], inv[f]
    else:
        raise KeyError(name)
    return v.astype(np.float32), np.ascontiguousarray(f, np.int64).astype(np.int32), origin, step


def body_sphere(rings=84, segments=82):
    """A closed UV-sphere connectivity of `rings` x `segments` plus two poles — 6890 vertices and 13776 faces at the defaults, SMPL's
    counts — warped to body extents (about 1.9 x 1.8 x 0.5 m) -> (verts float32, faces int32)."""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    T, Pp = np.meshgrid(th, ph, indexing='ij')
    x, y, z = np.sin(T) * np.cos(Pp), np.cos(T), np.sin(T) * np.sin(Pp)
    ring = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]])
    v = v * (1.0 + 0.15 * np.sin(5 * v[:, 1:2]) * np.cos(3 * v[:, 0:1]))          # bumps: no two tiles see the same geometry
    v = v * np.array([0.95, 0.9, 0.25]) + np.array([0.02, -0.25, 0.05])
    idx = lambda r, s: 1 + r * segments + (s % segments)
    south = 1 + rings * segments
    f = []
    for s in range(segments):
        f.append([0, idx(0, s + 1), idx(0, s)])
        f.append([south, idx(rings - 1, s), idx(rings - 1, s + 1)])
    for r in range(rings - 1):
        for s in range(segments):
            f.append([idx(r, s), idx(r, s + 1), idx(r + 1, s)])
            f.append([idx(r, s + 1), idx(r + 1, s + 1), idx(r + 1, s)])
    return v.astype(np.float32), np.array(f, np.int32)
