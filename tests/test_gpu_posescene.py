"""GPU: invr.posescene.PoseScenes and driver.run_poses on the small model of the fixtures (64 x 64 x 32).

A posed frame built from scene.make_scene's SMPL-like output (world vertices, Th, R, poses) must give the host restatement's tensors
(tests/posescene_reference.py) bit for bit — `A` within the bar of test_gpu_parity.test_scene_prep_on_device — and its one-channel
distance volume must render exactly what the host-built 25-channel volume (weights[nearest] + distance) renders: the test that the
path reads nothing of `pbw` but its last channel.  run_poses with frames in flight returns the images of sequential renders.

tests/test_hostsim_posescene_cpu.py runs TENSOR_TESTS on the CPU wave machine, on a lattice cut to LATTICE_CROP."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import posescene_reference as R           # noqa: E402  (checker only)

DEV = 'cuda:0'
LATTICE_CROP = None                                  # the wave machine: keep the lattice's first (cx, cy, cz) points per axis
TENSOR_TESTS = ['test_frame_tensors_are_the_host_restatement', 'test_frame_A_is_the_reference_chain',
                'test_distance_channel_is_the_reference_volume', 'test_frame_refuses_device_vertices_and_wrong_shapes']
KEYS = ('rgb_map', 'acc_map', 'raw', 'occ')


def big_poses():
    big = np.zeros(72)
    big[5] = np.deg2rad(30)
    big[8] = np.deg2rad(-30)                          # tpose_dataset.py:278-283, as invr/scene.py:170-171
    return big


def make_scenes(cfg, batch, extras):
    from invr import scene
    from invr.posescene import PoseScenes
    ps = PoseScenes(scene._J, scene.PARENTS, extras['weights'], extras['parts'], extras['tpose'], batch['tuv'][0].numpy(),
                    batch['tbounds'][0].numpy(), big_poses(), cfg=cfg, device=DEV)
    if LATTICE_CROP is not None:
        full = PoseScenes.lattice
        ps.lattice = lambda ppts: (lambda o, s, d: (o, s, [min(a, b) for a, b in zip(d, LATTICE_CROP)]))(*full(ppts))
    return ps


def frame_args(batch, extras, latent_index=3):
    return dict(wxyz=extras['wpts'], Th=np.asarray(batch['Th'][0]), poses=extras['poses'], latent_index=latent_index, R=np.asarray(batch['R'][0]))


@pytest.fixture(scope='module')
def posed(small_setup):
    """-> (PoseScenes, the frame of the fixtures' scene as CPU tensors, its host values, batch, extras)."""
    cfg, sd, batch, extras = small_setup
    ps = make_scenes(cfg, batch, extras)
    f = ps.frame(**frame_args(batch, extras))
    if DEV != 'cpu':
        torch.cuda.synchronize()
    return ps, f, {k: v.cpu() for k, v in f.items()}, batch, extras


def bits(t):
    a = t.numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def same(t, want):
    want = np.asarray(want)
    return tuple(t.shape) == want.shape and np.array_equal(bits(t), bits(want))


def test_frame_tensors_are_the_host_restatement(posed):
    from invr.config import NUM_PARTS
    ps, f, c, batch, extras = posed
    Th, Rw = batch['Th'][0].numpy(), batch['R'][0].numpy()
    ppts = R.pose_points(extras['wpts'], Th, Rw)
    assert set(f) == {'A', 'big_A', 'pbw', 'pbounds', 'wbounds', 'R', 'Th', 'ppts', 'part_pts', 'part_pbw', 'lengths2', 'bounds', 'tuv',
                      'tbounds', 'frame_dim', 'latent_index'}
    assert all(v.device.type == torch.device(DEV).type for v in f.values())
    assert same(c['ppts'], ppts) and np.abs(ppts - batch['ppts'][0].numpy()).max() < 1e-6          # (the batch poses first, then places)
    assert same(c['pbounds'], R.get_bounds(ppts)) and same(c['wbounds'], R.get_bounds(extras['wpts']))
    assert same(c['wbounds'], batch['wbounds'][0]) and same(f.host['wbounds'], batch['wbounds'][0])
    pp, pb, l2, bd = R.part_sets(ppts, extras['weights'], extras['parts'], extras['tpose'], NUM_PARTS, 0.2)
    assert same(c['part_pts'], pp) and same(c['part_pbw'], pb) and same(c['bounds'], bd)
    assert c['lengths2'].dtype == torch.int64 and same(c['lengths2'], l2)
    assert same(c['part_pbw'], batch['part_pbw'][0]) and same(c['bounds'], batch['bounds'][0]) and same(c['lengths2'], batch['lengths2'][0])
    assert ps.max_length == int(l2.max()) and c['part_pts'].shape[1] == ps.max_length
    assert same(c['R'], Rw) and same(c['Th'], Th) and same(c['tuv'], batch['tuv'][0]) and same(c['tbounds'], batch['tbounds'][0])
    assert c['frame_dim'].dtype == torch.float32 and same(c['frame_dim'], np.float32(3 / 100)) and same(c['frame_dim'], batch['frame_dim'][0])
    assert c['latent_index'].dtype == torch.int64 and int(c['latent_index']) == 3


def test_frame_A_is_the_reference_chain(posed):
    from invr import scene
    ps, f, c, batch, extras = posed
    for got, poses in ((c['A'], extras['poses']), (c['big_A'], big_poses())):
        err = np.abs(got.numpy() - R.rigid_transformation(poses, scene._J, scene.PARENTS))
        assert err.max() <= 2.4e-7 and (err > 0).sum() <= 4, (err.max(), (err > 0).sum())
    assert np.abs(c['A'].numpy() - batch['A'][0].numpy()).max() < 1e-6 and np.abs(c['big_A'].numpy() - batch['big_A'][0].numpy()).max() < 1e-6


@pytest.fixture(scope='module')
def reference_volume(posed):
    """-> (dist (Dx,Dy,Dz) float32, nearest (Dx,Dy,Dz) int32) of the contract on the frame's lattice."""
    ps, f, c, batch, extras = posed
    h = f.host
    origin, step, dims = R.lattice(c['ppts'].numpy())
    assert np.array_equal(origin, h['origin']) and np.array_equal(step, h['step'])
    assert list(dims) == list(h['dims']) or LATTICE_CROP is not None
    dims = h['dims']
    points = R.lattice_points(origin, step, dims)
    dist, near = R.exact_volume(c['ppts'].numpy(), points)
    index = np.random.RandomState(11).randint(0, len(points), 1024)          # the proposals held the contract's winner: brute force agrees
    bd, bn = R.brute_force(c['ppts'].numpy(), points[index])
    assert np.array_equal(bits(dist[index]), bits(bd)) and np.array_equal(near[index], bn)
    return dist.reshape(dims), near.reshape(dims)


def test_distance_channel_is_the_reference_volume(posed, reference_volume):
    ps, f, c, batch, extras = posed
    dist, _ = reference_volume
    assert c['pbw'].shape == dist.shape + (1,) and c['pbw'].is_contiguous()
    assert same(c['pbw'][..., 0], dist)
    if LATTICE_CROP is None:                          # the volume spans the box of the body with the tool's padding
        assert all(abs(dist.shape[a] - batch['pbw'].shape[1 + a]) <= 1 for a in range(3))


def test_frame_refuses_device_vertices_and_wrong_shapes(posed):
    ps, f, c, batch, extras = posed
    args = frame_args(batch, extras)
    with pytest.raises(TypeError):
        ps.frame(**dict(args, wxyz=torch.from_numpy(extras['wpts']).to(DEV)))
    with pytest.raises(ValueError):
        ps.frame(**dict(args, wxyz=extras['wpts'][:100]))
    with pytest.raises(ValueError):
        ps.frame(**dict(args, R=None))


@pytest.fixture(scope='module')
def small_net(small_setup):
    from invr.network import Network
    cfg, sd, batch, extras = small_setup
    net = Network(cfg=cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


def render(net, batch, in_flight=1):
    from invr.renderer import Renderer
    r = Renderer(net)
    r.in_flight = in_flight
    with torch.no_grad():
        ret = r.render(dict(batch))
        out = {k: ret[k].clone() for k in KEYS}
    r.flush(release=True)
    return out


def test_one_channel_volume_renders_what_the_25_channel_volume_renders(posed, reference_volume, small_net, small_setup):
    ps, f, c, batch, extras = posed
    dist, near = reference_volume
    H, W = int(batch['H']), int(batch['W'])
    eb = ps.eval_batch(f, H, W, extras['K'], extras['Rc'], extras['Tc'])
    assert eb['pbw'].shape[-1] == 1 and eb['pbw'].data_ptr() == f['pbw'].data_ptr()          # by reference
    assert eb['ray_o'].shape[1] == int(eb['mask_at_box'].sum()) > 1000
    one = render(small_net, eb)
    assert float(one['rgb_map'].abs().max()) > 0 and float(one['occ'].max()) > 0.5
    pbw25 = np.concatenate([extras['weights'][near], dist[..., None]], axis=-1).astype(np.float32)
    assert pbw25.shape[-1] == 25
    eb25 = dict(eb, pbw=torch.from_numpy(pbw25).to(DEV)[None])
    full = render(small_net, eb25)
    for k in KEYS:
        assert torch.equal(one[k], full[k]), k


def test_run_poses_with_frames_in_flight_equals_sequential_renders(small_setup):
    from invr import driver, scene
    from invr.network import Network
    cfg, sd, batch0, _ = small_setup
    cfg16 = copy.deepcopy(cfg)
    cfg16['N_samples'] = 16
    net = Network(cfg=cfg16)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    H = W = 32
    frames, cams, ps = [], [], None
    for pose_seed in (0, 1, 2):
        b, e = scene.make_scene(H, W, seed=0, pose_seed=pose_seed)
        b = scene.to_torch(b)
        if ps is None:
            ps = make_scenes(cfg16, b, e)
        frames.append(frame_args(b, e, latent_index=pose_seed))
        cams.append((H, W, e['K'], e['Rc'], e['Tc']))
    got = driver.run_poses(net, ps, frames, lambda i: cams[i], in_flight=2)
    assert len(got) == 3
    seen = []
    from invr.renderer import Renderer
    mine = Renderer(net)                              # a caller's renderer keeps its own setting and its lanes
    driver.run_poses(net, ps, frames[:2], cams[0], in_flight=3, on_frame=lambda i, img, acc: seen.append((i, img, acc)), renderer=mine)
    assert [s[0] for s in seen] == [0, 1] and mine.in_flight == 1 and 1 <= len(mine._lanes) <= 3
    mine.flush(release=True)
    for i in range(3):
        eb = ps.eval_batch(ps.frame(**frames[i]), *cams[i])
        out = render(net, eb)
        img = driver.assemble_image(out['rgb_map'][0].cpu().numpy(), eb)
        mask = eb['mask_at_box'][0].cpu().numpy().reshape(H, W)
        assert got[i][0].shape == (H, W, 3) and got[i][1].shape == (H, W)
        assert np.array_equal(got[i][0], img) and np.array_equal(got[i][1][mask], out['acc_map'][0].cpu().numpy())
        assert float(np.abs(img).max()) > 0 and not got[i][1][~mask].any()
    assert np.array_equal(seen[0][1], got[0][0]) and not np.array_equal(got[0][0], got[1][0])
