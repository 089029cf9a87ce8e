"""CPU: the checker of include/invr_surface.h (tests/surface_reference.py) against hand-worked points of a single triangle, one in each
of Ericson's seven regions (every value below is exact in binary), the vectorised form against the header's walk read line by line,
the winner rules, the interpolation, and — with the restatement alone — that each mesh family of tests/test_gpu_surface_volume.py
reaches the branch it is named for."""
import numpy as np
import pytest

from tests import surface_reference as S

A, B, C = [0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]
# (point, region, (u, v, w), key) — worked by hand from the header's formulas
HAND = [([-1.0, -1.0, 2.0], 1, (1.0, 0.0, 0.0), 6.0),          # d1 = -4, d2 = -4
        ([6.0, -1.0, 0.0], 2, (0.0, 1.0, 0.0), 5.0),           # d3 = 8, d4 = -4
        ([1.0, -2.0, 1.0], 3, (0.75, 0.25, 0.0), 5.0),         # d1 = 4, d3 = -12, vc = -128: v = 4 / 16, q = (1, 0, 0)
        ([-1.0, 6.0, 0.0], 4, (0.0, 0.0, 1.0), 5.0),           # vc = 384, d5 = -4, d6 = 8
        ([-2.0, 1.0, 1.0], 5, (0.75, 0.0, 0.25), 5.0),         # vc = 64, d2 = 4, d6 = -12, vb = -128: w = 4 / 16, q = (0, 1, 0)
        ([3.0, 3.0, 1.0], 6, (0.0, 0.5, 0.5), 3.0),            # vc = vb = 192, va = -128, e = g = 16: w = 16 / 32, q = (2, 2, 0)
        ([1.0, 1.0, 3.0], 7, (0.5, 0.25, 0.25), 9.0)]          # va = 128, vb = vc = 64: den = 1 / 256, q = (1, 1, 0)


def test_hand_worked_points_of_one_triangle_in_each_region():
    verts = np.array([A, B, C], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    pts = np.array([h[0] for h in HAND])
    face, bary, dist, region = S.brute_force(verts, faces, pts)
    assert region.tolist() == [1, 2, 3, 4, 5, 6, 7] and (face == 0).all()
    for i, (p, r, uvw, key) in enumerate(HAND):
        assert tuple(bary[i]) == uvw, (i, bary[i])
        assert dist[i] == np.float32(np.sqrt(key)), (i, dist[i])
        k, b, reg = S.closest_scalar(p, A, B, C)
        assert (k, b, reg) == (key, uvw, r), (i, k, b, reg)


def test_vectorised_form_is_the_walk_read_line_by_line():
    g = np.random.RandomState(3)
    for name in ('soup65', 'sliver', 'degenerate', 'dyadic_octahedron'):
        dims = (17, 9, 33)
        v, f, o, s = S.mesh(name, dims)
        ok = ((f >= 0) & (f < len(v))).all(axis=1)
        v64, f = v.astype(np.float64), f[ok]
        pts = S.lattice_points(o, s, dims)[g.randint(0, int(np.prod(dims)), 40)]
        fi = g.randint(0, len(f), 25)
        a, b, c = (v64[f[fi, k]][None] for k in range(3))
        key, u, vv, w, reg = S.closest_on_faces(pts[:, None, :], a, b, c)
        for i, p in enumerate(pts):
            for j in range(len(fi)):
                k, (su, sv, sw), r = S.closest_scalar(p, a[0, j], b[0, j], c[0, j])
                got = np.array([key[i, j], u[i, j], vv[i, j], w[i, j]])
                assert np.array_equal(got.view(np.int64), np.array([k, su, sv, sw]).view(np.int64)) and r == reg[i, j], (name, i, j)


def test_winner_rules():
    verts = np.array([A, B, C, [0, 0, 1], [4, 0, 1], [0, 4, 1]], np.float32)
    pts = np.array([[1.0, 1.0, 0.5], [1.0, 1.0, 0.25], [1.0, 1.0, 3.0]])
    # equal keys go to the lowest face, whatever the order of the rows; a copy of a face never beats it
    face, bary, dist, _, ties = S.brute_force(verts, np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2]]), pts, with_ties=True)
    assert face.tolist() == [0, 1, 0] and ties.tolist() == [3, 2, 1] and dist.tolist() == [0.5, 0.25, 2.0]
    # faces with a corner outside [0, V) take no part; with none left: -1, zeros, +inf
    face, bary, dist, region = S.brute_force(verts, np.array([[0, 1, 6], [-1, 1, 2], [3, 4, 5]]), pts)
    assert face.tolist() == [2, 2, 2]
    face, bary, dist, region = S.brute_force(verts, np.array([[0, 1, 6], [-1, 1, 2]]), pts)
    assert (face == -1).all() and not bary.any() and np.isposinf(dist).all() and not region.any()
    # a == b with c elsewhere: 0 / 0 in region 3 for points abeam of a — a NaN key that never wins against a proper face far away
    verts = np.array([[0, 0, 0], [0, 0, 0], [0, 4, 0], [50, 0, 0], [54, 0, 0], [50, 4, 0]], np.float32)
    p = np.array([[1.0, 1.0, 1.0]])
    key = S.closest_on_faces(p[:, None, :], *(verts[None, [k]].astype(np.float64) for k in range(3)))[0]
    assert np.isnan(key).all()
    face, bary, dist, region = S.brute_force(verts, np.array([[0, 1, 2], [3, 4, 5]]), p)
    assert face.tolist() == [1] and np.isfinite(bary).all()


def test_interpolation():
    attr = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 2, 3], [0, 1, 4]])
    bary = np.array([[0.5, 0.25, 0.25], [0.0, 0.5, 0.5], [1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.2, 0.3, 0.5]])
    out = S.interpolate(attr, faces, np.array([0, 1, 0, -1, 2]), bary)
    assert out.dtype == np.float32 and out.tolist() == [[2.0, 20.0], [6.0, 60.0], [1.0, 10.0], [0.0, 0.0], [0.0, 0.0]]
    third = np.float32(1) / np.float32(3)
    out = S.interpolate(np.array([[third], [third], [third]]), faces[:1], np.array([0]), np.array([[0.1, 0.2, 0.7]]))
    want = np.float32((0.1 * np.float64(third) + 0.2 * np.float64(third)) + 0.7 * np.float64(third))
    assert out[0, 0] == want


def test_body_sphere_has_the_counts_of_smpl():
    v, f = S.body_sphere()
    assert v.shape == (6890, 3) and f.shape == (13776, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert len(np.unique(f)) == 6890
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()          # closed: every edge has two faces
    ext = v.max(0) - v.min(0)
    assert 1.7 < ext[0] < 2.2 and 1.7 < ext[1] < 2.0 and 0.4 < ext[2] < 0.65


@pytest.fixture(scope='module')
def families():
    dims = (17, 9, 33)
    out = {}
    for name in S.MESHES:
        v, f, o, s = S.mesh(name, dims)
        out[name] = (v, f) + S.brute_force(v, f, S.lattice_points(o, s, dims), with_ties=True)
    return out


def test_each_mesh_family_reaches_its_branch(families):
    regions = lambda name: set(np.unique(families[name][5]).tolist())
    assert regions('tri1') == {1, 2, 3, 4, 5, 6, 7}
    assert len(families['tet'][1]) == 4 and [len(families['soup%d' % n][1]) for n in (63, 64, 65, 1000)] == [63, 64, 65, 1000]
    v, f, face, bary, dist, region, ties = families['identical']
    assert len(f) == 1000 and (face == 0).all() and (ties == 1000).all()
    v, f, face, bary, dist, region, ties = families['dyadic_octahedron']
    assert (ties[dist == 0] >= 2).all() and (dist == 0).sum() >= 6 and (ties >= 4).any()
    v, f, face, bary, dist, region, ties = families['degenerate']
    bad = ~((f >= 0) & (f < len(v))).all(axis=1)
    same = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    assert bad.sum() >= 8 and (same & ~bad).sum() >= 5 and (f == len(v)).any() and (f == -1).any()
    assert not bad[face].any() and np.isfinite(bary).all() and np.isfinite(dist).all()
    v, f, face, bary, dist, region, ties = families['all_degenerate']
    assert (face == -1).all() and not bary.any() and np.isposinf(dist).all()
    assert S.CLAMPED in regions('sliver')
    assert families['far'][4].min() > 9.0
    v, f, face, bary, dist, region, ties = families['unreferenced']
    unused = np.setdiff1d(np.arange(len(v)), f)
    o, s = S.ORIGIN, S.STEP
    assert len(unused) == 50 and (v[unused] >= o - 1e-6).all() and (v[unused] <= o + (np.array([17, 9, 33]) - 1) * s + 1e-6).all() and dist.min() > 0.4


def test_big_triangles_pass_every_tile_and_identical_faces_overflow_the_list():
    """The kernel's sphere test restated loosely (no widening needed for a margin this large): every face of `big` lies within reach of
    every tile centre, so its candidate list (128 records, drained when more than 64 are held) is drained repeatedly."""
    dims = (17, 9, 33)
    v, f, o, s = S.mesh('big', dims)
    c = v.astype(np.float64)[f]
    centre = c.mean(axis=1)
    radius = np.linalg.norm(c - centre[:, None], axis=2).max(axis=1)
    tiles = S.lattice_points(o + 1.5 * s, 4 * s, [(d + 3) // 4 for d in dims])
    gap = np.linalg.norm(tiles[:, None] - centre[None], axis=2) - radius[None]
    assert len(f) == 300 and (gap < 0).all()
