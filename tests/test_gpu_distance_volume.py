"""GPU: invr_distance_volume (csrc/k_posescene.hip) through the C ABI of include/invr_posescene.h against the NumPy float64 brute
force of the contract (tests/posescene_reference.py): `dist` and `nearest` bit for bit, on lattices that straddle the kernel's
4 x 4 x 4 tile and on vertex sets that exercise ties, exact zeros, a candidate list longer than its LDS buffer (1000 identical
vertices) and bounds far larger than the lattice.  The production shape (the 6890 posed vertices of scene.make_scene and the lattice
np.arange gives for them) is checked bit for bit on seeded points and against cKDTree on all of them.

Outputs and the workspace are pre-filled with 0xFF bytes.  tests/test_hostsim_posescene_cpu.py runs the same bodies on the CPU wave
machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import posescene_reference as R           # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
LATTICES = [(1, 1, 1), (1, 1, 70), (70, 1, 1), (3, 5, 4), (17, 9, 33), (33, 16, 65)]
MAX_POINTS = None                                    # the wave machine drops lattices above this many points
ORIGIN, STEP = np.array([-0.37, 0.11, 1.03]), np.array([0.025, 0.03, 0.02])
DYADIC_ORIGIN, DYADIC_STEP = np.array([-1.0, 0.5, 2.0]), np.array([0.125, 0.125, 0.125])
VERTEX_SETS = ['rand1', 'rand4', 'rand63', 'rand64', 'rand65', 'rand1000', 'identical', 'collinear', 'duplicated', 'dyadic', 'far', 'cluster']
PRODUCTION_CROP = None                               # the wave machine keeps the lattice's first (cx, cy, cz) points per axis


def lattices():
    return [d for d in LATTICES if MAX_POINTS is None or d[0] * d[1] * d[2] <= MAX_POINTS]


def case(name, dims):
    """-> (verts (n,3) float32, origin, step) of vertex set `name` over the lattice `dims`, seeded by both."""
    g = np.random.RandomState(sum(map(ord, name)) * 1000 + dims[0] * 97 + dims[1] * 13 + dims[2])
    origin, step = (DYADIC_ORIGIN, DYADIC_STEP) if name == 'dyadic' else (ORIGIN, STEP)
    lo, hi = origin, origin + (np.array(dims) - 1) * step
    box = lambda n, pad=0.05: g.uniform(lo - pad, hi + pad, (n, 3))
    if name.startswith('rand'):
        v = box(int(name[4:]))
    elif name == 'identical':
        v = np.repeat(box(1), 1000, axis=0)           # every vertex passes every tile's bound: the candidate list is drained twice
    elif name == 'collinear':
        v = (lo - 0.05)[None] + np.sort(g.uniform(0, 1, 100))[:, None] * (hi - lo + 0.1)[None]
    elif name == 'duplicated':
        half = box(300)
        v = np.concatenate([half, half])[g.permutation(600)]          # ties between a vertex and its copy: the lower row wins
    elif name == 'dyadic':
        # vertices ON the lattice points of even index: distance exactly 0 there, exact ties between symmetric neighbours elsewhere
        ijk = np.stack(np.meshgrid(*[np.arange(0, d, 2) for d in dims], indexing='ij'), -1).reshape(-1, 3)
        ijk = ijk[g.permutation(len(ijk))[:500]]
        v = origin[None] + ijk * step[None]
    elif name == 'far':
        v = box(200) + np.array([0.0, 10.0, 0.0])
    elif name == 'cluster':
        v = np.concatenate([(lo + 0.3 * (hi - lo))[None] + g.uniform(-1e-3, 1e-3, (200, 3)), (hi + 0.04)[None]])[g.permutation(201)]
    else:
        raise KeyError(name)
    return v.astype(np.float32), origin, step


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


def run_raw(verts, origin, step, dims, fill=0xFF, want_nearest=True):
    """invr_distance_volume over a fresh workspace and fresh outputs of `fill` bytes -> (dist float32, nearest int32 or None), flat."""
    L = _abi.lib()
    n = int(np.prod(dims))
    nbytes = L.invr_distance_volume_workspace_bytes(len(verts))
    assert nbytes >= 16 * len(verts)
    ws = aligned_bytes(nbytes, fill)
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV)
    dist = aligned_bytes(4 * n, fill).view(torch.float32)
    near = aligned_bytes(4 * n, fill).view(torch.int32) if want_nearest else None
    _abi.check(L.invr_distance_volume(_abi.ptr(v), len(verts), (C.c_double * 3)(*origin), (C.c_double * 3)(*step), (C.c_int32 * 3)(*dims),
                                      _abi.ptr(dist), _abi.ptr(near, torch.int32), _abi.ptr(ws, torch.uint8), ws.numel(), _abi.stream_ptr()))
    sync()
    return dist.cpu().numpy().copy(), (near.cpu().numpy().copy() if want_nearest else None)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('name', VERTEX_SETS)
def test_distance_and_row_are_the_brute_force_bit_for_bit(name):
    for dims in lattices():
        verts, origin, step = case(name, dims)
        dist, near = run_raw(verts, origin, step, dims)
        want_d, want_n = R.brute_force(verts, R.lattice_points(origin, step, dims))
        assert np.array_equal(near, want_n), (name, dims, int((near != want_n).sum()))
        assert same_bits(dist, want_d), (name, dims, int((dist.view(np.int32) != want_d.view(np.int32)).sum()))
        if name == 'dyadic':
            assert (dist == 0).sum() >= min(500, int(np.prod([(d + 1) // 2 for d in dims])))
            if min(dims) >= 3 and np.prod(dims) <= 6000:          # the point between two vertices on an axis ties: the reference resolved it to the lower row
                d2 = ((R.lattice_points(origin, step, dims)[:, None] - verts[None].astype(np.float64)) ** 2).sum(-1)
                assert ((d2 == d2.min(1, keepdims=True)).sum(1) > 1).any()
        if name == 'far':
            assert dist.min() > 9.0


@functools.lru_cache(maxsize=None)
def production():
    """-> (ppts (6890,3) float32, origin, step, dims) of scene.make_scene's posed body and the tool's lattice over it."""
    from invr import scene
    batch, _ = scene.make_scene(H=8, W=8)
    ppts = np.ascontiguousarray(batch['ppts'][0], np.float32)
    origin, step, dims = R.lattice(ppts)
    if PRODUCTION_CROP is not None:
        dims = [min(d, c) for d, c in zip(dims, PRODUCTION_CROP)]
    return ppts, origin, step, dims


@functools.lru_cache(maxsize=None)
def production_run(dev):
    ppts, origin, step, dims = production()
    return run_raw(ppts, origin, step, dims)


def test_production_shape_against_the_brute_force_on_seeded_points():
    ppts, origin, step, dims = production()
    assert len(ppts) == 6890 and np.allclose(step, 0.025, rtol=0, atol=1e-12)
    dist, near = production_run(DEV)
    n = int(np.prod(dims))
    corners = [np.ravel_multi_index((i, j, k), dims) for i in (0, dims[0] - 1) for j in (0, dims[1] - 1) for k in (0, dims[2] - 1)]
    index = np.concatenate([np.random.RandomState(7).randint(0, n, 2048), corners])
    want_d, want_n = R.brute_force(ppts, R.lattice_points(origin, step, dims, index))
    assert np.array_equal(near[index], want_n)
    assert same_bits(dist[index], want_d)


def test_production_shape_against_the_tree_on_all_points():
    from scipy.spatial import cKDTree
    ppts, origin, step, dims = production()
    dist, near = production_run(DEV)
    tree, _ = cKDTree(ppts.astype(np.float64)).query(R.lattice_points(origin, step, dims))
    # the tree's own distance may differ from the contract's operation order in the last double bit: one float32 ulp of the value
    err = np.abs(dist.astype(np.float64) - tree)
    ulp = np.spacing(tree.astype(np.float32)).astype(np.float64)
    print('points %d: max |dist - tree| / ulp = %.3f' % (len(tree), float((err / ulp).max())))
    assert (err <= ulp).all()
    assert near.min() >= 0 and near.max() < len(ppts)


@pytest.mark.parametrize('name,dims', [('rand1000', (17, 9, 33)), ('identical', (3, 5, 4)), ('duplicated', (17, 9, 33))])
def test_same_bits_over_dirty_memory_and_without_nearest(name, dims):
    verts, origin, step = case(name, dims)
    a_d, a_n = run_raw(verts, origin, step, dims, fill=0xFF)
    b_d, b_n = run_raw(verts, origin, step, dims, fill=0xFF)
    c_d, c_n = run_raw(verts, origin, step, dims, fill=0x5A)
    assert same_bits(a_d, b_d) and same_bits(a_d, c_d) and np.array_equal(a_n, b_n) and np.array_equal(a_n, c_n)
    assert np.isfinite(a_d).all()
    d_d, d_n = run_raw(verts, origin, step, dims, want_nearest=False)          # nearest = NULL
    assert d_n is None and same_bits(a_d, d_d)


def test_prep_distance_volume_is_the_abi_call():
    from invr import prep
    dims = (17, 9, 33)
    for name in ('rand65', 'rand1000', 'rand4'):      # (the cached workspace grows, then serves a smaller call)
        verts, origin, step = case(name, dims)
        want_d, want_n = run_raw(verts, origin, step, dims)
        v = torch.from_numpy(verts).to(DEV)
        dist, near = prep.distance_volume(v, origin, step, dims, nearest=True)
        only = prep.distance_volume(v, origin, step, dims)
        sync()
        assert dist.shape == tuple(dims) and near.shape == tuple(dims) and dist.dtype == torch.float32 and near.dtype == torch.int32
        assert same_bits(dist.cpu().numpy().reshape(-1), want_d) and np.array_equal(near.cpu().numpy().reshape(-1), want_n)
        assert torch.equal(only, dist)
    with pytest.raises(ValueError):
        prep.distance_volume(torch.zeros(0, 3, device=DEV), origin, step, dims)
