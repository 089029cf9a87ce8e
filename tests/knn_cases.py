"""Test infrastructure: adversarial vertex sets for the 4-nearest-neighbour kernels (csrc/k_knn.hip) and an EXACT reference.

The production tests pin k_knn_pairs on one regime — the synthetic body of scene.make_scene: 6890 well-spread vertices, at most 58
clusters per part, a 0.025 m lattice.  The builders here return the same `batch` contract with only part_pts / part_pbw / lengths2 /
pbw / pbounds (and, where stated, R / Th) replaced, and a ray list of their own (`rays`):

  dup(k, layout)   every k-th vertex of each body part repeated k times, rows interleaved or appended as a block: every query has
                   exact distance ties, decided by the row half of the (distance,row) key
  lattice          vertices on the dyadic lattice 2^-5 m: two box shells (every point three times), a coplanar part, a collinear
                   part (zero-extent AABB axes: the Morton sort's e > 0 ? .. : 0 branch) and ONE point repeated 70 times (all keys
                   in one of the 4096 buckets)
  edges_a/b/c      part lengths (4, 17, 64, 65, 4033) / (3, 16, 63, 128, 4096) / (5, 4097, 129, 1000, 2000): the 64- and the
                   65-cluster part (candidate masks off), sentinel tails, the len < 4 skip, sub-clusters with < 4 real vertices
  carve_fit/spill  5 x 1536 vertices (7680 LDS slots: the largest index that fits) / one vertex more (7744: device-side brute force)
  offset           edges_c with pose space translated by (+8, -8, +8) m: the prefilter's delta = 2^-19 (|q| + max |v|)^2
  coarse(_tight)   the original body under a 7 x 19 x 5 distance lattice (voxel ~0.1 m, not cubic), and with pbounds shrunk so that
                   part of the ray samples fall outside the lattice

Exactness: for vertices on k 2^-5 m with |k| <= 64 and queries on k 2^-6 m every fp32 dx, dx*dx and every partial sum of
dx*dx + dy*dy + dz*dz is an integer multiple of 2^-12 below 2^24 * 2^-12 — exact in fp32 in any association, with or without FMA
contraction.  `exact_knn` therefore works in integers and its rows and squared distances are compared with NO tolerance.

NumPy / SciPy only: no GPU, no HIP import."""
import functools

import numpy as np

Q5, Q6 = 2.0 ** -5, 2.0 ** -6
KMAX = 64                      # vertices: |k| <= 64 lattice units of 2^-5 m
TWO_R2 = 2.0 * 0.075 * 0.075   # blend_utils.py:741,747
KNN_EPS = 1e-8

EDGES = {'edges_a': (4, 17, 64, 65, 4033), 'edges_b': (3, 16, 63, 128, 4096), 'edges_c': (5, 4097, 129, 1000, 2000),
         'carve_fit': (1536,) * 5, 'carve_spill': (1536, 1536, 1536, 1536, 1537)}
LDS_SLOTS = 7680               # KNN_LDS_MAX_V (csrc/k_knn.hip): padded vertex slots that fit the LDS-resident index


def padded_slots(lengths):
    return int(sum((int(n) + 63) // 64 * 64 for n in lengths))


# ---- exact reference -------------------------------------------------------------------------------------------------------------
def to_units(x, unit):
    """float coordinates -> integer multiples of `unit`, asserting that they ARE such multiples (and fp32-representable)."""
    x = np.asarray(x, np.float64)
    k = np.rint(x / unit)
    assert np.array_equal(k * unit, x) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return k.astype(np.int64)


def exact_knn(queries, part_pts, lengths, k_out=5):
    """queries (n,3) on the 2^-6 m lattice, part_pts (P,M,3) on the 2^-5 m lattice, lengths (P,): for every (point, part) the
    `k_out` smallest (d^2, row) keys over the first lengths[p] rows, ties ordered by row -> rows (n,P,k_out) int64 and d2 (n,P,k_out)
    float64 (every value fp32-representable: asserted); missing entries (lengths[p] < k_out) are row 0 at +inf, the kernels' empty
    marker."""
    q = to_units(queries, Q6)
    P = part_pts.shape[0]
    n = q.shape[0]
    rows = np.zeros((n, P, k_out), np.int64)
    d2 = np.full((n, P, k_out), np.inf)
    for p in range(P):
        L = int(lengths[p])
        if L == 0:
            continue
        v = to_units(part_pts[p, :L], Q5) * 2                                  # in units of 2^-6 m
        assert np.abs(v).max() <= 2 * KMAX
        for c0 in range(0, n, 256):
            qq = q[c0:c0 + 256]
            dd = ((qq[:, None, :] - v[None, :, :]) ** 2).sum(-1)               # (c,L) exact integers, units of 2^-12 m^2
            assert dd.max() < 2 ** 24                                          # every partial sum is below it too: exact in fp32
            key = dd * 8192 + np.arange(L)[None, :]                            # (d^2, row): rows < 8192
            kk = min(k_out, L)
            part = np.partition(key, kk - 1, axis=1)[:, :kk] if L > kk else key
            part = np.sort(part, axis=1)
            rows[c0:c0 + 256, p, :kk] = part % 8192
            d2[c0:c0 + 256, p, :kk] = (part // 8192) * 2.0 ** -12
    fin = np.isfinite(d2)
    assert np.array_equal(d2[fin].astype(np.float32).astype(np.float64), d2[fin])
    return rows, d2


def blend_reference(d2, rows, part_pbw):
    """float64 evaluation of blend_utils.py:745-763 on exact squared distances d2 (n,P,4) / rows (n,P,4): -> w (n,P,4), dist (n,P),
    bw (n,P,24), x = -d^2 / 0.01125 (n,P,4).  A part with fewer than 4 vertices has an infinite distance: w = 0, dist = NaN."""
    d2 = np.asarray(d2, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.sqrt(d2)
        x = -d2 / TWO_R2
        e = np.exp(x)
        w = e / (e.sum(-1, keepdims=True) + KNN_EPS)
        dist = (d * w).sum(-1)
        P = d2.shape[1]
        bw = np.stack([(np.asarray(part_pbw[p], np.float64)[rows[:, p]] * w[:, p, :, None]).sum(1) for p in range(P)], 1)
    return w, dist, bw, x


def tie_45(rows4, part_pts, lengths):
    """From a COMPLETE (distance,row)-ordered 4-list alone: does the part hold a vertex outside the list with the coordinates of the
    list's 4th vertex?  Then the 4th and 5th nearest distances are bit-equal whatever the query.  rows4 (n,P,4) -> bool (n,P)."""
    rows4 = np.asarray(rows4, np.int64)
    out = np.zeros(rows4.shape[:2], bool)
    for p in range(rows4.shape[1]):
        L = int(lengths[p])
        if L < 5:
            continue
        _, inv, cnt = np.unique(np.asarray(part_pts[p, :L]), axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        g = inv[np.clip(rows4[:, p], 0, L - 1)]                                 # (n,4) coordinate class of every listed row
        out[:, p] = cnt[g[:, 3]] > (g == g[:, 3:4]).sum(1)
    return out


# ---- scene assembly --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def base(seed=0):
    """(batch, extras) of scene.make_scene(64, 64): shared, the builders copy what they replace"""
    from invr import scene
    return scene.make_scene(64, 64, seed=seed, cam_dist=1.8)


def body_parts(b):
    L = b['lengths2'][0]
    return [np.array(b['part_pts'][0, p, :L[p]]) for p in range(len(L))]


def finish(b, parts, seed, voxel=0.04, dims=None, all_survive=False, pad_rows=5, shrink=0.0, keep_bounds=False, dyadic=False):
    """The batch `b` with the five vertex sets `parts` (list of (len,3) float32) in place of the body's: part_pts (rows behind a
    part's length hold DECOYS inside the part's box — nearer than the real rows for many queries, never to be read), random positive
    part_pbw rows summing to 1, lengths2, and the distance volume: a lattice of `voxel` metres (or of `dims` corners) over the
    vertices' box + 0.05 m (keep_bounds: over the batch's pbounds; shrink: that box pulled in by `shrink` metres per side), 24 weight
    channels of the nearest vertex and, as the distance channel, the nearest-vertex distance of the NEW sets (all_survive: 0, every
    ray-sample inside the lattice survives the cull)."""
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(seed + 77)
    b = dict(b)
    P = len(parts)
    lens = np.array([len(x) for x in parts], np.int64)
    M = int(lens.max()) + pad_rows
    pp = np.zeros((P, M, 3), np.float32)
    pb = rng.uniform(0.05, 1.0, (P, M, 24))
    pb = (pb / pb.sum(-1, keepdims=True)).astype(np.float32)
    allv = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in parts])
    lo_all, hi_all = allv.min(0), allv.max(0)
    for p in range(P):
        pp[p, :lens[p]] = parts[p]
        lo, hi = (parts[p].min(0), parts[p].max(0)) if lens[p] else (lo_all, hi_all)
        dec = rng.uniform(0, 1, (M - lens[p], 3)) * (hi - lo) + lo
        pp[p, lens[p]:] = np.rint(dec / Q5) * Q5 if dyadic else dec
    b['part_pts'], b['part_pbw'], b['lengths2'] = pp[None], pb[None], lens[None]
    if keep_bounds:
        lo, hi = b['pbounds'][0].astype(np.float64)
    else:
        lo, hi = lo_all.astype(np.float64) - 0.05, hi_all.astype(np.float64) + 0.05
    lo, hi = lo + shrink, hi - shrink
    if dims is None:
        dims = np.ceil((hi - lo) / voxel).astype(int) + 1
        hi = lo + voxel * (dims - 1)
    axes = [np.linspace(lo[a], hi[a], int(dims[a])).astype(np.float32) for a in range(3)]
    g = np.stack(np.meshgrid(*axes, indexing='ij'), -1).astype(np.float32)
    dist, idx = cKDTree(allv.astype(np.float64)).query(g.reshape(-1, 3).astype(np.float64))
    wts = rng.uniform(0.05, 1.0, (len(allv), 24))
    wts /= wts.sum(-1, keepdims=True)
    if all_survive:
        dist = np.zeros_like(dist)
    b['pbw'] = np.concatenate([wts[idx], dist[:, None]], 1).reshape(g.shape[:3] + (25,)).astype(np.float32)[None]
    b['pbounds'] = np.stack([[ax[0] for ax in axes], [ax[-1] for ax in axes]]).astype(np.float32)[None]
    return b


def cells(b):
    return int(np.prod(b['pbw'].shape[1:4]))


def rays_pose(b, n, seed=0, window=None, cam=(0.3, 0.25, 2.0), inner=False):
    """-> eye (3,), directions (n,3), near (n,), far (n,) in POSE space (float64): see rays()"""
    rng = np.random.RandomState(seed + 4242)
    lo, hi = b['pbounds'][0].astype(np.float64)
    wlo, whi = (lo, hi) if window is None else (np.asarray(window[0], np.float64), np.asarray(window[1], np.float64))
    eye = 0.5 * (lo + hi) + np.asarray(cam)
    tgt = rng.uniform(0, 1, (n, 3)) * (whi - wlo) + wlo
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[np.abs(d) < 1e-5] = 1e-5
    t0, t1 = (lo - 0.02 - eye) / d, (hi + 0.02 - eye) / d
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    assert bool((near < far).all())
    if inner:
        u = np.sort(rng.uniform(0, 1, (n, 2)), axis=1)
        near, far = near + u[:, 0] * (far - near), near + u[:, 1] * (far - near)
    return eye, d, near, far


def rays(b, n, **kw):
    """n rays from one pose-space eye point through targets drawn uniformly from `window` = (lo, hi) in pose space (default: the
    lattice box), clipped to the lattice box + 0.02 m by the slab test, expressed in world space with the batch's R / Th
    (pose = (world - Th) @ R, blend_utils.py:366-382) -> the batch with ray_o / ray_d / near / far replaced.  inner: near < far are
    drawn uniformly from inside the slab interval — the two samples of an S = 2 call then sit at random depths instead of on the box
    faces."""
    eye, d, near, far = rays_pose(b, n, **kw)
    R, Th = b['R'][0].astype(np.float64), b['Th'][0].astype(np.float64)
    b = dict(b)
    b['ray_o'] = np.broadcast_to((eye @ R.T + Th.reshape(1, 3)), (n, 3)).astype(np.float32)[None]
    b['ray_d'] = (d @ R.T).astype(np.float32)[None]
    b['near'], b['far'] = near.astype(np.float32)[None], far.astype(np.float32)[None]
    for k in ('rgb', 'occupancy', 'mask_at_box'):
        b.pop(k, None)
    return b


def world_points(b, n, seed=0):
    """n world-space points (float32) whose pose-space positions are uniform in the lattice box + 0.02 m, and unit view directions:
    the inputs of Network.forward (a frame of ONE sample per point)"""
    rng = np.random.RandomState(seed + 515)
    lo, hi = b['pbounds'][0].astype(np.float64)
    p = rng.uniform(0, 1, (n, 3)) * (hi - lo + 0.04) + lo - 0.02
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R, Th = b['R'][0].astype(np.float64), b['Th'][0].astype(np.float64)
    return (p @ R.T + Th.reshape(1, 3)).astype(np.float32), (d @ R.T).astype(np.float32)


def far_dist2(b):
    """csrc/k_knn.hip:knn_far_dist2 restated: the far-fold distance^2 of a frame from the largest |entry| m of its A / big_A matrices —
    (0.68 m)^2 for m <= 2, the distance at which 4 exp(-d^2 / 0.01125) / 1e-8 * m falls to 1.12e-9 beyond, +inf for absurd matrices"""
    m = max(float(np.abs(b['A']).max()), float(np.abs(b['big_A']).max()))
    if not m <= 1e6:
        return np.inf
    return max(0.4624, 0.01125 * np.log(4.0 * m / 1.12e-17)) if m > 2.0 else 0.4624


def snap(x):
    """onto the 2^-5 m lattice, |k| <= 64"""
    return (np.clip(np.rint(np.asarray(x, np.float64) / Q5), -KMAX, KMAX) * Q5).astype(np.float32)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def dup(k, layout, seed=0, dyadic=False, **kw):
    """Every k-th vertex of each body part, k times: 'interleaved' rows (a a b b ..) or appended as a 'block' (a b .. a b ..)."""
    b, _ = base(seed)
    parts = []
    for v in body_parts(b):
        sub = snap(v[::k]) if dyadic else v[::k]
        parts.append(np.repeat(sub, k, axis=0) if layout == 'interleaved' else np.tile(sub, (k, 1)))
    return finish(b, parts, seed, dyadic=dyadic, **kw)


def _shell(c, h):
    """lattice points (integer units) on the surface of the box c +- h"""
    ax = [np.arange(c[a] - h[a], c[a] + h[a] + 1) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    on = (np.abs(g - np.asarray(c)) == np.asarray(h)).any(1)
    return g[on]


def _take(pool, n):
    """the first n rows of the pool repeated cyclically (a pool shorter than n: every point several times, appended as blocks)"""
    return pool[np.arange(n) % len(pool)]


LATTICE_LENGTHS = (2047, 2049, 2048, 200, 70)


def lattice_parts(lengths=LATTICE_LENGTHS):
    """[shell (1026 points, up to three times each), shell 0.7 m below it, coplanar plate z = const, collinear x = const / z = const,
    one point] in lattice units of 2^-5 m, |k| <= 64"""
    pools = [_shell((0, 10, 0), (8, 8, 4)), _shell((2, -20, 1), (6, 6, 3)),
             np.stack(np.meshgrid(np.arange(-16, 17), np.arange(-12, 5), [2], indexing='ij'), -1).reshape(-1, 3),
             np.stack([np.full(129, 20), np.arange(-64, 65), np.zeros(129, int)], 1),
             np.array([[-20, 10, 0]])]
    rng = np.random.RandomState(5)
    out = []
    for pool, n in zip(pools, lengths):
        pool = pool[rng.permutation(len(pool))]                                 # rows in no spatial order
        assert np.abs(pool).max() <= KMAX
        out.append((_take(pool, n) * Q5).astype(np.float32))
    return out


def lattice(seed=0, lengths=LATTICE_LENGTHS, **kw):
    b, _ = base(seed)
    return finish(b, lattice_parts(lengths), seed, dyadic=True, **kw)


def _surface_parts(b, lengths, seed):
    """Generic float positions from the body surface: part p = the lengths[p] body vertices nearest to a seed vertex of its own
    (head, a hand, a foot, pelvis, the other hand), each moved by up to 2 mm — spatially compact parts, so near, band and far pairs
    all occur; a longer part contains the shorter one around the same seed vertex (up to its last rows, below)."""
    from scipy.spatial import cKDTree
    v = np.array(b['ppts'][0], np.float64)
    tree = cKDTree(v)
    c = v.mean(0)
    seeds = [v[:, 1].argmax(), v[:, 0].argmax(), v[:, 1].argmin(), np.linalg.norm(v - c, axis=1).argmin(), v[:, 0].argmin()]
    parts = []
    for p, n in enumerate(lengths):
        idx = np.atleast_1d(tree.query(v[seeds[p]], k=int(n))[1])
        jit = np.random.RandomState(seed * 31 + p).uniform(-0.002, 0.002, (4100, 3))[:len(idx)]      # (same draws for a prefix)
        x = v[idx] + jit
        r = int(n) % 16
        if n >= 17 and 1 <= r <= 3:
            # the part's last r rows become OUTLIERS beyond the body's box in every axis: they take the largest Morton keys, i.e. they
            # are alone in the part's last 16-vertex sub-cluster — whose box (a point) must not bound any cell's 4th-nearest distance
            x[-r:] = v.max(0) + 0.15 + 0.01 * np.arange(r)[:, None]
        parts.append(x.astype(np.float32))
    return parts


def edges(name, seed=0, **kw):
    b, _ = base(seed)
    return finish(b, _surface_parts(b, EDGES[name], seed), seed, **kw)


def offset(seed=0, shift=(8.0, -8.0, 8.0), **kw):
    """edges_c with pose space translated: vertices and lattice move by `shift`, Th is adjusted so that the same world rays hit it"""
    b, _ = base(seed)
    t = np.asarray(shift, np.float64)
    parts = [(x.astype(np.float64) + t).astype(np.float32) for x in _surface_parts(b, EDGES['edges_c'], seed)]
    b = finish(b, parts, seed, **kw)
    R = b['R'][0].astype(np.float64)
    b['Th'] = (b['Th'][0].astype(np.float64) - (t @ R.T).reshape(1, 3)).astype(np.float32)[None]       # (x - Th') @ R = (x - Th) @ R + t
    return b


def coarse(seed=0, tight=False, **kw):
    b, _ = base(seed)
    return finish(b, body_parts(b), seed, dims=np.array([7, 19, 5]), keep_bounds=True, shrink=0.12 if tight else 0.0, **kw)


def build(name, **kw):
    if name in EDGES:
        return edges(name, **kw)
    if name.startswith('dup'):                                                   # dup2-interleaved, dup4-block, dup2-interleaved-dyadic ..
        f = name.split('-')
        return dup(int(f[0][3:]), f[1], dyadic='dyadic' in f[2:], **kw)
    return {'lattice': lattice, 'offset': offset, 'coarse': coarse,
            'coarse_tight': lambda **k: coarse(tight=True, **k)}[name](**kw)


SCENES = ['dup2-interleaved', 'dup2-block-dyadic', 'dup4-block', 'dup4-interleaved-dyadic', 'lattice', 'edges_a', 'edges_b', 'edges_c',
          'carve_fit', 'carve_spill', 'offset', 'coarse', 'coarse_tight']


def query_block(lo, hi, n=None, seed=0):
    """Queries on the 2^-6 m lattice: all 2^-5 lattice points and cell mid-points (odd multiples of 2^-6 in every axis) of the block
    [lo, hi] (units of 2^-5 m), in a seeded random order; the first n of them."""
    ax = [np.arange(2 * lo[a], 2 * hi[a] + 1) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    par = g % 2
    g = g[(par == 0).all(1) | (par == 1).all(1)]
    g = g[np.random.RandomState(seed + 9).permutation(len(g))]
    return (g[:n] * Q6).astype(np.float32)
