"""GPU: a subject set up from its SMPL mesh alone — invr.posescene.canonical_volumes and PoseScenes.from_smpl.

The vertices are scene.make_scene's big-pose body, which has no connectivity: a deterministic set of small faces joins each vertex to its
two nearest neighbours (not a manifold; the contract of include/invr_surface.h does not ask for one).  The device-built `tuv` and `tbw`
must be the restatement's (tests/surface_reference.py) bit for bit on seeded lattice points, and a posed frame rendered from
PoseScenes.from_smpl must equal, bit for bit, the render from a PoseScenes that is handed the device-built volume, and — on a lattice
cropped small enough for the host — the render from a volume the restatement built alone.

tests/test_hostsim_surface_cpu.py runs TENSOR_TESTS on the CPU wave machine, on a lattice cut to LATTICE_CROP."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import posescene_reference as R           # noqa: E402  (checker only)
from tests import surface_reference as S             # noqa: E402  (checker only)
from tests.test_gpu_posescene import KEYS, big_poses, frame_args, render, small_net          # noqa: E402,F401  (small_net: a fixture)

DEV = 'cuda:0'
LATTICE_CROP = None                                  # the wave machine: keep the canonical lattice's first (cx, cy, cz) points per axis
HOST_CROP = (12, 12, 10)                             # the lattice of the volume the restatement builds alone (1440 points x 6890 faces)
TENSOR_TESTS = ['test_canonical_volumes_are_the_restatement_on_seeded_points', 'test_canonical_volumes_refuse_wrong_shapes']


@contextlib.contextmanager
def cropped_lattice(crop):
    """PoseScenes.lattice cut to its first `crop` points per axis while the block runs (None: as it is)."""
    from invr.posescene import PoseScenes
    full = PoseScenes.lattice
    if crop is not None:
        PoseScenes.lattice = staticmethod(lambda ppts: (lambda o, s, d: (o, s, [min(a, b) for a, b in zip(d, crop)]))(*full(ppts)))
    try:
        yield
    finally:
        PoseScenes.lattice = staticmethod(full)


@functools.lru_cache(maxsize=None)
def subject():
    """-> (tpose (6890,3) float32, faces (6890,3) int32, vertex_uv (6890,2) float32, weights (6890,24) float32)."""
    from scipy.spatial import cKDTree
    from invr import scene
    _, extras = scene.make_scene(H=8, W=8)
    tpose = np.ascontiguousarray(extras['tpose'], np.float32)
    _, nn = cKDTree(tpose.astype(np.float64)).query(tpose.astype(np.float64), k=3)
    rows = np.arange(len(tpose))
    others = np.stack([np.where(nn[:, k] == rows, nn[:, 0], nn[:, k]) for k in (1, 2)], axis=1)          # (a coincident vertex may come first)
    faces = np.concatenate([rows[:, None], others], axis=1).astype(np.int32)
    vuv = np.ascontiguousarray(scene.make_body(0)[3], np.float32)
    return tpose, faces, vuv, np.ascontiguousarray(extras['weights'], np.float32)


def canonical(crop, weights=True):
    from invr.posescene import canonical_volumes
    tpose, faces, vuv, w = subject()
    with cropped_lattice(crop):
        vol = canonical_volumes(tpose, faces, vuv, weights=w if weights else None, device=DEV)
    if DEV != 'cpu':
        torch.cuda.synchronize()
    return vol


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_canonical_volumes_are_the_restatement_on_seeded_points():
    tpose, faces, vuv, weights = subject()
    assert tpose.shape == (6890, 3) and faces.shape == (6890, 3) and vuv.shape == (6890, 2) and weights.shape == (6890, 24)
    vol = canonical(LATTICE_CROP)
    origin, step, dims = R.lattice(tpose)
    if LATTICE_CROP is not None:
        dims = [min(a, b) for a, b in zip(dims, LATTICE_CROP)]
    assert set(vol) == {'tuv', 'tbw', 'tbounds', 'origin', 'step', 'dims'}
    assert np.array_equal(vol['origin'], origin) and np.array_equal(vol['step'], step) and list(vol['dims']) == list(dims)
    assert vol['tuv'].shape == tuple(dims) + (2,) and vol['tbw'].shape == tuple(dims) + (25,)
    assert vol['tuv'].dtype == vol['tbw'].dtype == torch.float32 and vol['tuv'].device.type == torch.device(DEV).type
    want_b = R.get_bounds(tpose, 0.05)
    assert vol['tbounds'].dtype == np.float32 and np.array_equal(bits(vol['tbounds']), bits(want_b))
    n = int(np.prod(dims))
    index = np.unique(np.random.RandomState(13).randint(0, n, 2048))
    face, bary, dist, _ = S.brute_force(tpose, faces, R.lattice_points(origin, step, dims, index))
    tuv = vol['tuv'].cpu().numpy().reshape(n, 2)[index]
    tbw = vol['tbw'].cpu().numpy().reshape(n, 25)[index]
    assert np.array_equal(bits(tuv), bits(S.interpolate(vuv, faces, face, bary)))
    assert np.array_equal(bits(tbw[:, :24]), bits(S.interpolate(weights, faces, face, bary)))
    assert np.array_equal(bits(tbw[:, 24]), bits(dist))
    assert (face >= 0).all() and np.abs(tbw[:, :24].sum(axis=1) - 1).max() < 1e-5          # (interpolated skinning weights still sum to 1)
    assert 'tbw' not in canonical(LATTICE_CROP if LATTICE_CROP is not None else (8, 8, 8), weights=False)


def test_canonical_volumes_refuse_wrong_shapes():
    from invr.posescene import canonical_volumes
    tpose, faces, vuv, weights = subject()
    for bad in (lambda: canonical_volumes(tpose[:, :2], faces, vuv, device=DEV), lambda: canonical_volumes(tpose, faces, vuv[:100], device=DEV),
                lambda: canonical_volumes(tpose, faces, vuv, weights=weights[:, :23], device=DEV),
                lambda: canonical_volumes(tpose, faces[:, :2], vuv, device=DEV)):
        with pytest.raises(ValueError):
            bad()


def posed_render(net, ps, batch, extras):
    """One posed frame of `ps` at 32 x 32 rays."""
    f = ps.frame(**frame_args(batch, extras))
    K = np.array(extras['K'], np.float64)
    K[:2] *= 32.0 / float(batch['H'])
    eb = ps.eval_batch(f, 32, 32, K, extras['Rc'], extras['Tc'])
    assert eb['ray_o'].shape[1] > 100
    return render(net, eb)


def make(cfg, extras, tuv, tbounds):
    from invr import scene
    from invr.posescene import PoseScenes
    return PoseScenes(scene._J, scene.PARENTS, extras['weights'], extras['parts'], extras['tpose'], tuv, tbounds, big_poses(), cfg=cfg, device=DEV)


def test_from_smpl_renders_what_the_handed_volume_renders(small_net, small_setup):
    from invr import scene
    from invr.posescene import PoseScenes
    cfg, sd, batch, extras = small_setup
    tpose, faces, vuv, weights = subject()
    assert np.array_equal(tpose, np.ascontiguousarray(extras['tpose'], np.float32))
    ps = PoseScenes.from_smpl(scene._J, scene.PARENTS, extras['weights'], extras['parts'], extras['tpose'], faces, vuv, big_poses(), cfg=cfg, device=DEV)
    vol = canonical(None, weights=False)
    assert torch.equal(ps.tuv, vol['tuv']) and np.array_equal(ps.tbounds.cpu().numpy(), vol['tbounds'])
    assert all(abs(ps.tuv.shape[a] - batch['tuv'].shape[1 + a]) <= 1 for a in range(3)) and ps.tuv.shape[3] == 2
    one = posed_render(small_net, ps, batch, extras)
    two = posed_render(small_net, make(cfg, extras, vol['tuv'].cpu().numpy(), vol['tbounds']), batch, extras)
    assert float(one['rgb_map'].abs().max()) > 0 and float(one['occ'].max()) > 0.5
    for k in KEYS:
        assert torch.equal(one[k], two[k]), k


def test_host_built_volume_renders_the_same(small_net, small_setup):
    cfg, sd, batch, extras = small_setup
    tpose, faces, vuv, weights = subject()
    vol = canonical(HOST_CROP, weights=False)
    origin, step, dims = R.lattice(tpose)
    dims = [min(a, b) for a, b in zip(dims, HOST_CROP)]
    face, bary, dist, _ = S.brute_force(tpose, faces, R.lattice_points(origin, step, dims))
    host = S.interpolate(vuv, faces, face, bary).reshape(tuple(dims) + (2,))
    assert tuple(vol['tuv'].shape) == host.shape and np.array_equal(bits(vol['tuv'].cpu().numpy()), bits(host))
    one = posed_render(small_net, make(cfg, extras, vol['tuv'].cpu().numpy(), vol['tbounds']), batch, extras)
    two = posed_render(small_net, make(cfg, extras, host, R.get_bounds(tpose, 0.05)), batch, extras)
    for k in KEYS:
        assert torch.equal(one[k], two[k]), k
