"""GPU: the surface-extraction kernels (csrc/k_mesh.hip) through the C ABI of include/invr_mesh.h against the NumPy / float64
restatement of the contract (tests/mesh_reference.py).

Exact: the totals, the per-point masks, the per-cell triangle counts, both prefix sums, the tetrahedron every triangle lies on, the
closedness and orientation of the index list, the Euler characteristic.  Positions: each coordinate within
8 * 2^-24 * (|pa| + |pb|) of the float64 interpolation of the same fp32 inputs (3 roundings in t, 3 in the lerp, a margin) and
between its edge's ends up to that bound.  Orientation: normal . gradient <= 0 on the exact positions (degenerate triangles give 0).

Outputs and the workspace are pre-filled: NaN bytes where a kernel must write, a marker where it must not.
tests/test_hostsim_mesh_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mesh_reference as R                # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
MARK = -0x365A5A5B                                   # int32 bit pattern no kernel produces here (as a float: -5.4e-6 is no grid coordinate)
LEVEL = 0.1
ORIGIN, VOXEL = (-0.37, 0.11, 1.03), (0.05, 0.04, 0.03)
EPS = 2.0 ** -24

SMALL = ['1x1x1', '1x1x70', '70x1x1', '3x5x4', '17x9x33', 'sphere', 'torus', 'full4', 'onlevel', 'nan']
LARGE = ['33x16x65']
CASES = SMALL + LARGE
EULER = {'1x1x1': 2, 'sphere': 2, 'torus': 0}


def smooth(shape, seed):
    """A random smooth field in about [-0.4, 1.2]: a few low-frequency waves, so that the level set is a handful of blobs."""
    g = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    f = np.zeros(shape)
    for _ in range(5):
        k = g.uniform(-0.9, 0.9, 3)
        f += np.sin(k[0] * x + k[1] * y + k[2] * z + g.uniform(0, 6.28))
    return (0.4 + 0.35 * f).astype(np.float32)


@functools.lru_cache(maxsize=None)
def volume(case):
    """-> fp32 ndarray (Dx, Dy, Dz), seeded by the case."""
    g = np.random.RandomState(sum(map(ord, case)))
    if case == '1x1x1':
        return np.full((1, 1, 1), 0.8, dtype=np.float32)
    if case in ('1x1x70', '70x1x1', '3x5x4'):
        return g.uniform(0.0, 0.2, tuple(int(n) for n in case.split('x'))).astype(np.float32)
    if case in ('17x9x33', '33x16x65'):
        return smooth(tuple(int(n) for n in case.split('x')), g.randint(1 << 30))
    if case in ('sphere', 'torus'):
        x, y, z = np.meshgrid(*[np.arange(15, dtype=np.float64) - 7.0] * 3, indexing='ij')
        if case == 'sphere':
            d = np.sqrt(x * x + y * y + z * z) - 5.3
        else:
            d = np.sqrt((np.sqrt(x * x + y * y) - 4.6) ** 2 + z * z) - 1.7
        return (LEVEL - 0.2 * d).astype(np.float32)
    if case == 'full4':
        return g.uniform(0.6, 1.0, (4, 4, 4)).astype(np.float32)
    v = g.uniform(0.0, 0.2, (5, 6, 7)).astype(np.float32)
    sel = g.uniform(size=v.shape) < 0.3
    v[sel] = np.float32(LEVEL) if case == 'onlevel' else np.float32('nan')          # a value ON the level is inside; a NaN is outside
    return v


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


def c3(v, t):
    return (t * 3)(*v)


def marked(rows, written, dtype):
    """(rows, 3) on DEV: NaN bytes (0xFF) in the first `written` rows, MARK behind them."""
    t = torch.full((rows, 3), MARK, dtype=torch.int32)
    t[:written] = -1
    return t.view(dtype).to(DEV)


def count(vol_d, dims, level, ws, counts):
    L = _abi.lib()
    _abi.check(L.invr_mesh_count(_abi.ptr(vol_d), c3(dims, C.c_int32), level, _abi.ptr(ws, torch.uint8), ws.numel(), _abi.ptr(counts, torch.int64),
                                 _abi.stream_ptr()))


def emit(vol_d, dims, origin, voxel, level, ws, verts, vcap, tris, tcap, counts):
    L = _abi.lib()
    _abi.check(L.invr_mesh_emit(_abi.ptr(vol_d), c3(dims, C.c_int32), c3(origin, C.c_float), c3(voxel, C.c_float), level, _abi.ptr(ws, torch.uint8),
                                ws.numel(), _abi.ptr(verts), vcap, _abi.ptr(tris, torch.int32), tcap, _abi.ptr(counts, torch.int64), _abi.stream_ptr()))


def run_raw(vol, fill=0xFF, short=0, origin=ORIGIN, voxel=VOXEL, level=LEVEL):
    """invr_mesh_count + invr_mesh_emit over a fresh workspace of `fill` bytes with capacities `short` below the totals -> dict of
    CPU tensors.  Rows behind the capacities are asserted to keep their marker."""
    L = _abi.lib()
    dims = vol.shape
    nbytes = L.invr_mesh_workspace_bytes(c3(dims, C.c_int32))
    assert nbytes > 0
    ws = aligned_bytes(nbytes, fill)
    vol_d = torch.from_numpy(vol).to(DEV)
    counts = torch.full((8,), MARK, dtype=torch.int64, device=DEV)
    count(vol_d, dims, level, ws, counts)
    sync()
    c0 = counts.cpu()
    nv, nt = int(c0[0]), int(c0[1])
    assert c0[2:4].tolist() == [0, 0] and (c0[4:] == MARK).all()
    vcap, tcap = max(nv - short, 0), max(nt - short, 0)
    verts, tris = marked(nv + 4, vcap, torch.float32), marked(nt + 4, tcap, torch.int32)
    emit(vol_d, dims, origin, voxel, level, ws, verts, vcap, tris, tcap, counts)
    sync()
    v = _abi.mesh_views(ws, dims)
    v.pop('layout')
    r = {k: t.cpu().clone() for k, t in v.items()}
    verts, tris, c1 = verts.cpu(), tris.cpu(), counts.cpu()
    assert (verts[vcap:].contiguous().view(torch.int32) == MARK).all() and (tris[tcap:] == MARK).all(), 'written past a capacity'
    assert (c1[4:] == MARK).all() and c1[:2].tolist() == [nv, nt] and r['counts'].tolist() == [nv, nt, 0, 0]
    r.update(n_vertices=nv, n_triangles=nt, overflow=int(c1[2]), vertices=verts[:vcap], triangles=tris[:tcap], out_counts=c1[:4])
    return r


@functools.lru_cache(maxsize=None)
def run(case, dev):
    return run_raw(volume(case))


@functools.lru_cache(maxsize=None)
def reference(case):
    return R.Reference(volume(case), ORIGIN, VOXEL, LEVEL)


def check_counts(r, ref):
    assert (r['n_vertices'], r['n_triangles'], r['overflow']) == (ref.n_vertices, ref.n_triangles, 0)
    assert np.array_equal(r['masks'].numpy(), ref.masks)
    assert np.array_equal(r['tcounts'].numpy(), ref.tcounts)
    assert np.array_equal(r['voffsets'].numpy(), ref.voffsets) and np.array_equal(r['toffsets'].numpy(), ref.toffsets)


def check_vertices(r, ref):
    got = r['vertices'].numpy().astype(np.float64)
    assert got.shape == ref.positions.shape
    pa, pb = ref.pa.astype(np.float64), ref.pb.astype(np.float64)
    bound = 8 * EPS * (np.abs(pa) + np.abs(pb))
    err = np.abs(got - ref.positions)
    print('vertices %d: max error / bound = %.3f' % (len(got), float((err / bound).max()) if len(got) else 0.0))
    assert (err <= bound).all()
    assert (got >= np.minimum(pa, pb) - bound).all() and (got <= np.maximum(pa, pb) + bound).all()


def check_triangles(r, ref, euler=None):
    tri = r['triangles'].numpy().astype(np.int64)
    assert tri.shape == (ref.n_triangles, 3)
    if len(tri):
        assert tri.min() >= 0 and tri.max() < ref.n_vertices
    # the triangles of cell g are the rows [toffsets[g], toffsets[g] + tcounts[g]); each lies on one tetrahedron of that cell, and every
    # tetrahedron gets as many as the contract gives it
    cells = np.repeat(np.arange(len(ref.tcounts)), ref.tcounts)
    tet = ref.triangle_tets(tri, cells)
    assert (tet >= 0).all()
    per_tet = np.zeros_like(ref.tet_counts)
    np.add.at(per_tet, (cells, tet), 1)
    assert np.array_equal(per_tet, ref.tet_counts)
    closed, chi = R.mesh_facts(ref.n_vertices, tri)
    assert closed, 'the index list is not a closed, consistently oriented surface'
    if euler is not None:
        assert chi == euler, chi
    p = ref.positions
    normal = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    dot = (normal * ref.gradient(cells, tet)).sum(1)
    assert (dot <= 0).all(), float(dot.max())
    if len(tri):
        # positive signed volume: the surface faces away from what it encloses
        assert (np.cross(p[tri[:, 0]], p[tri[:, 1]]) * p[tri[:, 2]]).sum() > 0


@pytest.mark.parametrize('case', CASES)
def test_mesh_against_the_contract(case):
    r, ref = run(case, DEV), reference(case)
    if case == '1x1x1':
        assert (ref.n_vertices, ref.n_triangles) == (14, 24)
    assert ref.n_triangles > 0
    check_counts(r, ref)
    check_vertices(r, ref)
    check_triangles(r, ref, EULER.get(case))


def config_volume(cfg):
    """2 x 2 x 2 volume of sign configuration cfg: inside values in [0.6, 1], outside values in [0, 0.09)."""
    g = np.random.RandomState(1000 + cfg)
    bits = ((cfg >> np.arange(8)) & 1).astype(bool).reshape(2, 2, 2)
    return np.where(bits, g.uniform(0.6, 1.0, (2, 2, 2)), g.uniform(0.0, 0.09, (2, 2, 2))).astype(np.float32)


def test_all_256_sign_configurations_of_a_2x2x2_volume():
    for cfg in range(256):
        vol = config_volume(cfg)
        r, ref = run_raw(vol), R.Reference(vol, ORIGIN, VOXEL, LEVEL)
        check_counts(r, ref)
        if cfg == 0:
            assert (r['n_vertices'], r['n_triangles']) == (0, 0) and r['vertices'].shape[0] == 0 and r['triangles'].shape[0] == 0
            continue
        check_vertices(r, ref)
        check_triangles(r, ref)
        _, chi = R.mesh_facts(ref.n_vertices, r['triangles'].numpy())
        assert chi % 2 == 0, (cfg, chi)


@pytest.mark.parametrize('case', ['onlevel', 'nan'])
def test_values_on_the_level_and_nans_follow_the_rule(case):
    vol, r, ref = volume(case), run(case, DEV), reference(case)
    special = (vol == np.float32(LEVEL)) if case == 'onlevel' else np.isnan(vol)
    assert special.sum() > 10
    inside = (r['masks'].numpy().reshape(ref.shape) >> 7).astype(bool)[1:-1, 1:-1, 1:-1]
    assert inside[special].all() if case == 'onlevel' else not inside[special].any()
    assert np.isfinite(r['vertices'].numpy()).all()


@pytest.mark.parametrize('case', ['3x5x4', 'sphere'])
def test_capacity_one_short_sets_the_overflow_flag(case):
    full = run(case, DEV)
    r = run_raw(volume(case), short=1)               # (run_raw asserts the markers behind the capacities)
    assert r['overflow'] == 1 and r['out_counts'].tolist() == [full['n_vertices'], full['n_triangles'], 1, 0]
    assert torch.equal(r['vertices'], full['vertices'][:-1]) and torch.equal(r['triangles'], full['triangles'][:-1])


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize('case', ['17x9x33', 'torus'])
def test_same_bits_over_any_dirty_workspace(case):
    a, b = run(case, DEV), run_raw(volume(case), fill=0x5A)
    assert same_bits(a['vertices'], b['vertices']) and same_bits(a['triangles'], b['triangles'])
    for k in ('masks', 'tcounts', 'voffsets', 'toffsets', 'counts', 'partials'):
        assert torch.equal(a[k], b[k]), k


GRID_CASES = [((3, 5, 4), 0, 60), ((3, 5, 4), 7, 31), ((17, 9, 33), 1000, 257), ((17, 9, 33), 17 * 9 * 33 - 300, 300), ((1, 1, 70), 69, 1)]


@pytest.mark.parametrize('dims,first,n', GRID_CASES)
def test_grid_points_are_the_fp32_formula(dims, first, n):
    L = _abi.lib()
    xyz = marked(n + 2, n, torch.float32)
    _abi.check(L.invr_grid_points(c3(ORIGIN, C.c_float), c3(VOXEL, C.c_float), c3(dims, C.c_int32), first, n, _abi.ptr(xyz), _abi.stream_ptr()))
    sync()
    xyz = xyz.cpu()
    idx = np.stack(np.unravel_index(np.arange(first, first + n), dims), axis=1)
    want = R.coords(ORIGIN, VOXEL, idx + 1)          # (the checker's indices are padded ones)
    assert np.array_equal(xyz[:n].numpy().view(np.int32), want.view(np.int32))
    assert (xyz[n:].contiguous().view(torch.int32) == MARK).all()
