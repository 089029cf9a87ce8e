"""GPU: invr_surface_volume and invr_surface_interpolate (csrc/k_surface.hip) through the C ABI of include/invr_surface.h against the
NumPy float64 brute force of the contract (tests/surface_reference.py): `face`, `bary` (as int64 bits) and `dist` bit for bit, on
lattices that straddle the kernel's 4 x 4 x 4 tile and on meshes that each exercise one thing that can go wrong (MESHES; that each
family reaches its branch is pinned on the CPU by tests/test_surface_reference_cpu.py).  The production shape (a closed mesh with
SMPL's counts at body extents on the tool's lattice) is checked bit for bit on seeded points and by properties on all of them.

Outputs and the workspace are pre-filled with 0xFF bytes.  tests/test_hostsim_surface_cpu.py runs the same bodies on the CPU wave
machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import surface_reference as S             # noqa: E402  (checker only)
from tests.test_gpu_distance_volume import LATTICES as DV_LATTICES          # noqa: E402
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
LATTICES = DV_LATTICES[:5]
LARGE, LARGE_MAX_FACES = DV_LATTICES[5], 100         # 33 x 16 x 65, only where a mesh has at most 100 faces
MAX_POINTS = None                                    # the wave machine drops lattices above this many points
PRODUCTION_CROP = None                               # the wave machine keeps the lattice's first (cx, cy, cz) points per axis


def lattices(n_faces):
    ls = LATTICES + ([LARGE] if n_faces <= LARGE_MAX_FACES else [])
    return [d for d in ls if MAX_POINTS is None or d[0] * d[1] * d[2] <= MAX_POINTS]


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def run_raw(verts, faces, origin, step, dims, fill=0xFF, want_bary=True, want_dist=True):
    """invr_surface_volume over a fresh workspace and fresh outputs of `fill` bytes -> (face int32, bary (n,3) float64 or None,
    dist float32 or None), flat."""
    L = _abi.lib()
    n = int(np.prod(dims))
    nbytes = L.invr_surface_volume_workspace_bytes(len(faces))
    assert nbytes >= 80 * len(faces)
    ws = aligned_bytes(nbytes, fill)
    v, f = dev(verts, np.float32), dev(faces, np.int32)
    face = aligned_bytes(4 * n, fill).view(torch.int32)
    bary = aligned_bytes(24 * n, fill).view(torch.float64) if want_bary else None
    dist = aligned_bytes(4 * n, fill).view(torch.float32) if want_dist else None
    _abi.check(L.invr_surface_volume(_abi.ptr(v), len(verts), _abi.ptr(f, torch.int32), len(faces), (C.c_double * 3)(*origin), (C.c_double * 3)(*step),
                                     (C.c_int32 * 3)(*dims), _abi.ptr(face, torch.int32), _abi.ptr(bary, torch.float64), _abi.ptr(dist),
                                     _abi.ptr(ws, torch.uint8), ws.numel(), _abi.stream_ptr()))
    sync()
    return (face.cpu().numpy().copy(), bary.cpu().numpy().reshape(n, 3).copy() if want_bary else None,
            dist.cpu().numpy().copy() if want_dist else None)


def run_interpolate(attr, n_verts, faces, face, bary, out, stride, offset):
    """invr_surface_interpolate into the device tensor `out` (flat float32)."""
    a, f = dev(attr, np.float32), dev(faces, np.int32)
    fc, b = dev(face, np.int32), dev(bary, np.float64)
    _abi.check(_abi.lib().invr_surface_interpolate(_abi.ptr(a), n_verts, a.shape[1], _abi.ptr(f, torch.int32), len(faces), _abi.ptr(fc, torch.int32),
                                                   _abi.ptr(b, torch.float64), len(face), _abi.ptr(out), stride, offset, _abi.stream_ptr()))
    sync()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(name, dims):
    """-> (verts, faces, origin, step, face, bary, dist, region, ties) of the contract on mesh `name` over the lattice `dims`: computed
    once, shared by the tests, never written to."""
    verts, faces, origin, step = S.mesh(name, dims)
    return (verts, faces, origin, step) + S.brute_force(verts, faces, S.lattice_points(origin, step, dims), with_ties=True)


def assert_same(got, want, what):
    for g, w, k in zip(got, want, ('face', 'bary', 'dist')):
        assert same_bits(g, w), (what, k, int((bits(g) != bits(w)).reshape(len(g), -1).any(axis=1).sum()))


@pytest.mark.parametrize('name', S.MESHES)
def test_face_bary_and_distance_are_the_brute_force_bit_for_bit(name):
    seen = set()
    for dims in lattices(len(S.mesh(name, (1, 1, 1))[1])):
        verts, faces, origin, step, face, bary, dist, region, ties = reference(name, tuple(dims))
        got = run_raw(verts, faces, origin, step, dims)
        assert_same(got, (face, bary, dist), (name, dims))
        seen |= set(np.unique(region).tolist())
        large = dims[0] >= 17 and dims[1] >= 9 and dims[2] >= 33
        if name == 'identical':
            assert len(faces) == 1000 and (got[0] == 0).all()
        if name == 'dyadic_octahedron' and large:      # exact ties across the faces of a shared corner or edge go to the lowest face
            tied = ties > 1
            assert tied.sum() > 1000 and (got[2] == 0).any() and (ties[got[2] == 0] >= 2).all()
            v64 = verts.astype(np.float64)
            pts = S.lattice_points(origin, step, dims)[tied][:200]
            key = S.closest_on_faces(pts[:, None, :], *(v64[faces[:, k]][None] for k in range(3)))[0]
            assert np.array_equal(got[0][tied][:200], np.argmin(key, axis=1))          # (argmin: the first of equal minima)
        if name == 'degenerate':
            assert not np.isnan(got[1]).any() and not np.isnan(got[2]).any() and (got[0] >= 0).all()
        if name == 'all_degenerate':
            assert (got[0] == -1).all() and not got[1].any() and np.isposinf(got[2]).all()
        if name == 'sliver' and large:
            assert (region == S.CLAMPED).any()
        if name == 'far':
            assert got[2].min() > 9.0
        if name == 'unreferenced':
            assert got[2].min() > 0.4
    if name == 'tri1' and (MAX_POINTS is None or MAX_POINTS >= 17 * 9 * 33):
        assert seen == {1, 2, 3, 4, 5, 6, 7}


@functools.lru_cache(maxsize=None)
def production():
    """-> (verts (6890,3) float32, faces (13776,3) int32, origin, step, dims): the body-sized closed mesh and the tool's lattice over it."""
    verts, faces = S.body_sphere()
    origin, step, dims = S.lattice(verts)
    if PRODUCTION_CROP is not None:
        dims = [min(d, c) for d, c in zip(dims, PRODUCTION_CROP)]
    return verts, faces, origin, step, dims


@functools.lru_cache(maxsize=None)
def production_run(dev_name):
    verts, faces, origin, step, dims = production()
    return run_raw(verts, faces, origin, step, dims)


def test_production_shape_against_the_brute_force_on_seeded_points():
    verts, faces, origin, step, dims = production()
    assert verts.shape == (6890, 3) and faces.shape == (13776, 3) and np.allclose(step, 0.025, rtol=0, atol=1e-12)
    face, bary, dist = production_run(DEV)
    n = int(np.prod(dims))
    corners = [np.ravel_multi_index((i, j, k), dims) for i in (0, dims[0] - 1) for j in (0, dims[1] - 1) for k in (0, dims[2] - 1)]
    index = np.concatenate([np.random.RandomState(7).randint(0, n, 2048), corners])
    want = S.brute_force(verts, faces, S.lattice_points(origin, step, dims, index))
    assert_same((face[index], bary[index], dist[index]), want[:3], 'production')


def test_production_shape_properties_on_all_points():
    from invr import prep
    verts, faces, origin, step, dims = production()
    face, bary, dist = production_run(DEV)
    assert face.min() >= 0 and face.max() < len(faces)
    assert bary.min() >= 0.0 and bary.max() <= 1.0
    total = np.abs((bary[:, 0] + bary[:, 1]) + bary[:, 2] - 1.0).max()
    print('points %d: max |u + v + w - 1| = %.3g' % (len(face), total))
    assert total <= 4e-16
    # the distance recomputed from the barycentric coordinates, in float64: one float32 ulp
    corner = verts.astype(np.float64)[faces[face]]
    q = (bary[:, :, None] * corner).sum(axis=1)
    again = np.sqrt(((S.lattice_points(origin, step, dims) - q) ** 2).sum(axis=1))
    err = np.abs(dist.astype(np.float64) - again)
    ulp = np.spacing(again.astype(np.float32)).astype(np.float64)
    print('max |dist - recomputed| / ulp = %.3f' % float((err / ulp).max()))
    assert (err <= ulp).all()
    # no farther than the nearest vertex (every vertex is a corner of some face): the existing distance volume on the same lattice
    to_vertex = prep.distance_volume(dev(verts, np.float32), origin, step, dims)
    sync()
    assert (dist <= to_vertex.cpu().numpy().reshape(-1)).all()


@pytest.mark.parametrize('name,dims', [('soup1000', (17, 9, 33)), ('identical', (3, 5, 4)), ('degenerate', (17, 9, 33)), ('all_degenerate', (3, 5, 4))])
def test_same_bits_over_dirty_memory_and_without_optional_outputs(name, dims):
    verts, faces, origin, step, face, bary, dist = reference(name, dims)[:7]
    a = run_raw(verts, faces, origin, step, dims, fill=0xFF)
    assert_same(a, (face, bary, dist), (name, dims))
    assert_same(run_raw(verts, faces, origin, step, dims, fill=0xFF), a, 'again')
    assert_same(run_raw(verts, faces, origin, step, dims, fill=0x5A), a, '0x5A')
    for want_bary, want_dist in ((False, True), (True, False), (False, False)):
        f, b, d = run_raw(verts, faces, origin, step, dims, want_bary=want_bary, want_dist=want_dist)
        assert np.array_equal(f, a[0]) and (b is None) == (not want_bary) and (d is None) == (not want_dist)
        assert (b is None or same_bits(b, a[1])) and (d is None or same_bits(d, a[2]))


def test_interpolation_is_the_restatement_bit_for_bit():
    dims = (17, 9, 33)
    verts, faces, origin, step, face, bary, dist = reference('degenerate', dims)[:7]
    g = np.random.RandomState(5)
    face = face.copy()
    bary = bary.copy()
    none = g.permutation(len(face))[:300]
    face[none] = -1                                   # rows without a face give 0 whatever their coordinates hold
    bary[none[:100]] = np.nan
    n, V = len(face), len(verts)
    for nc in (1, 2, 24):
        attr = g.uniform(-1, 1, (V, nc)).astype(np.float32)
        out = aligned_bytes(4 * n * nc, 0xFF).view(torch.float32)
        run_interpolate(attr, V, faces, face, bary, out, nc, 0)
        got = out.cpu().numpy().reshape(n, nc)
        assert same_bits(got, S.interpolate(attr, faces, face, bary)), nc
        assert not got[none].any() and np.abs(got).max() > 0.5
    # 24 + 1 channels into one (n, 25) buffer
    weights, last = g.uniform(0, 1, (V, 24)).astype(np.float32), g.uniform(0, 1, (V, 1)).astype(np.float32)
    out = aligned_bytes(4 * n * 25, 0xFF).view(torch.float32)
    run_interpolate(weights, V, faces, face, bary, out, 25, 0)
    got = out.cpu().numpy().reshape(n, 25).copy()
    assert same_bits(got[:, :24], S.interpolate(weights, faces, face, bary)) and (bits(got[:, 24]) == -1).all()          # channel 24 untouched
    run_interpolate(last, V, faces, face, bary, out, 25, 24)
    got2 = out.cpu().numpy().reshape(n, 25)
    assert same_bits(got2[:, :24], got[:, :24]) and same_bits(got2[:, 24:], S.interpolate(last, faces, face, bary))


def test_prep_wrappers_are_the_abi_calls():
    from invr import prep
    dims = (17, 9, 33)
    for name in ('soup65', 'soup1000', 'tet'):        # (the cached workspace grows, then serves a smaller call)
        verts, faces, origin, step, face, bary, dist = reference(name, dims)[:7]
        v, f = dev(verts, np.float32), dev(faces, np.int32)
        got = prep.surface_volume(v, f, origin, step, dims)
        only = prep.surface_volume(v, f, origin, step, dims, bary=False, dist=False)
        fd = prep.surface_volume(v, f, origin, step, dims, bary=False)
        attr = np.random.RandomState(1).uniform(-1, 1, (len(verts), 2)).astype(np.float32)
        uv = prep.surface_interpolate(dev(attr, np.float32), f, got[0], got[1])
        buf = torch.full(tuple(dims) + (3,), 7.0, device=DEV)
        same = prep.surface_interpolate(dev(attr, np.float32), f, got[0], got[1], out=buf, offset=1)
        sync()
        assert [tuple(t.shape) for t in got] == [tuple(dims), tuple(dims) + (3,), tuple(dims)]
        assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.float32]
        assert_same([t.cpu().numpy().reshape(len(face), -1).squeeze() for t in got], (face, bary, dist), name)
        assert len(only) == 1 and torch.equal(only[0], got[0]) and len(fd) == 2 and torch.equal(fd[0], got[0]) and torch.equal(fd[1], got[2])
        want = S.interpolate(attr, faces, face, bary)
        assert uv.shape == tuple(dims) + (2,) and same_bits(uv.cpu().numpy().reshape(-1, 2), want)
        assert same is buf and same_bits(buf.cpu().numpy().reshape(-1, 3)[:, 1:], want) and (buf[..., 0] == 7.0).all()
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    for bad in (lambda: prep.surface_volume(z(0, 3), f, origin, step, dims), lambda: prep.surface_volume(v, z(0, 3, dtype=torch.int32), origin, step, dims),
                lambda: prep.surface_volume(z(5, 2), f, origin, step, dims), lambda: prep.surface_volume(v, f[:, :2], origin, step, dims),
                lambda: prep.surface_volume(v, f, origin, step, (3, 0, 4)), lambda: prep.surface_volume(v, f, origin, step, (3, 4)),
                lambda: prep.surface_interpolate(z(len(verts), 65), f, got[0], got[1]),
                lambda: prep.surface_interpolate(z(len(verts), 2), f, got[0], got[1][..., :2]),
                lambda: prep.surface_interpolate(z(len(verts), 2), f, got[0], got[1], out=buf, offset=2),
                lambda: prep.surface_interpolate(z(len(verts), 2), f, got[0], got[1], offset=1)):
        with pytest.raises(ValueError):
            bad()
