"""GPU: invr.trainset.TrainSet — batches formed on the device from three resident synthetic frames (96 x 80, pose_seed 0..2,
patch_size 16) against the NumPy restatement of the path applied on the host with the same seed (tests/patch_reference.py): key by key
the same shapes, dtypes and bits, with and without prefetch; a yielded batch stays valid; scene tensors are referenced, not copied;
training steps fed by the set equal the same steps fed by host-built batches uploaded by hand; the eval batch equals
rays.rays_within_bounds + indexing."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import patch_reference as P              # noqa: E402  (checker only)
from invr import scene, params, driver, rays         # noqa: E402
from invr.config import make_cfg                     # noqa: E402
from invr.network import Network                     # noqa: E402
from invr.trainer import NetworkWrapper              # noqa: E402
from invr.trainset import TrainSet                   # noqa: E402

DEV = 'cuda:0'
H, W, PATCH = 96, 80, 16
SCENE_KEYS = ('A', 'big_A', 'pbw', 'pbounds', 'wbounds', 'R', 'Th', 'ppts', 'part_pts', 'part_pbw', 'lengths2', 'bounds')
SHARED_KEYS = ('tuv', 'tbounds')
ORDER = [0, 1, 2, 1, 0, 2, 2, 0]
CAM_DIST = (1.6, 2.4, 3.0)          # frame 0: the box covers every window; frames 1 and 2: its silhouette cuts some (count < w h)


@functools.lru_cache(maxsize=None)
def frames():
    """Three frames of one body: (img, msk, sem, K, R, T, scene items, latent index) each, and the shared items.  Read-only."""
    out, shared = [], None
    for f in range(3):
        b, ex = scene.make_scene(H, W, seed=0, frame=3 + 11 * f, cam_dist=CAM_DIST[f], pose_seed=f)
        msk, sem = P.synthetic_masks(H, W, cx=W / 2.0 + 3 * f, ay=0.40 * H)
        out.append(dict(img=P.synthetic_image(H, W, 20 + f, msk), msk=msk, sem=sem, K=ex['K'], R=ex['Rc'], T=ex['Tc'],
                        scene={k: b[k][0] for k in SCENE_KEYS}, latent=3 + 11 * f))
        shared = {k: b[k][0] for k in SHARED_KEYS}
    return out, shared


def make_set(cfg=None):
    fr, shared = frames()
    ts = TrainSet(cfg or make_cfg(patch_size=PATCH), device=DEV, shared=shared)
    for f in fr:
        ts.add_frame(f['img'], f['msk'], f['K'], f['R'], f['T'], f['scene'], sem_masks=f['sem'], latent_index=f['latent'], cam_ind=1)
    return ts


def restated(index, rng, focus=''):
    """The batch of frame `index` as the restatement forms it on the host: numpy arrays with the leading batch dimension of 1."""
    fr, shared = frames()
    f = fr[index]
    ref = f['msk'] if focus == '' else f['sem'][P.PART_NAMES.index(focus)]
    x0, y0, w, h, K32 = P.draw(f['msk'], ref, f['K'], PATCH, rng)
    k_inv, R, T, o = P.camera(K32, f['R'], f['T'])
    r = P.patch_batch(f['img'], f['msk'], x0, y0, w, h, k_inv, R, T, o, f['scene']['wbounds'])
    n = r['count']
    b = {'rgb': r['rgb'], 'occupancy': r['occupancy'].astype(bool), 'coord': r['coord'], 'ray_o': np.broadcast_to(o.astype(np.float32), (n, 3)),
         'ray_d': r['ray_d'], 'near': r['near'], 'far': r['far'], 'mask_at_box': r['mask_at_box'].astype(bool), 'H': np.int64(h), 'W': np.int64(w),
         'frame_dim': np.array(f['latent'] / 100).astype(np.float32), 'latent_index': np.int64(f['latent']), 'bw_latent_index': np.int64(f['latent']),
         'frame_index': np.int64(f['latent']), 'cam_ind': np.int64(1)}
    b.update(shared)
    b.update(f['scene'])
    return {k: np.ascontiguousarray(np.asarray(v)[None]) for k, v in b.items()}


def same(batch, want, tag):
    assert set(batch) == set(want), (tag, set(batch) ^ set(want))
    for k, v in want.items():
        t = batch[k]
        assert tuple(t.shape) == v.shape, (tag, k, tuple(t.shape), v.shape)
        got = t.detach().cpu().numpy()
        assert got.dtype == v.dtype, (tag, k, got.dtype, v.dtype)
        assert np.ascontiguousarray(got).tobytes() == v.tobytes(), (tag, k)
        assert t.is_cuda == (k not in driver.HOST_KEYS), (tag, k)          # H, W, frame_index, cam_ind stay host tensors


@pytest.mark.parametrize('seed', [0, 7])
def test_batches_equal_the_restatement_with_and_without_prefetch(seed):
    ts = make_set()
    ahead = list(ts.batches(ORDER, np.random.RandomState(seed), prefetch=2))
    plain = list(ts.batches(ORDER, np.random.RandomState(seed), prefetch=0))
    rng = np.random.RandomState(seed)
    assert len(ahead) == len(plain) == len(ORDER)
    counts = []
    for i, index in enumerate(ORDER):
        want = restated(index, rng)
        counts.append(want['ray_d'].shape[1])
        same(ahead[i], want, ('prefetch=2', i))
        same(plain[i], want, ('prefetch=0', i))
    assert seed != 7 or min(counts) < PATCH * PATCH                          # windows the box's silhouette cuts: compact tensors of count rows
    rng = np.random.RandomState(seed)
    same(ts.train_batch(ORDER[0], rng), restated(ORDER[0], np.random.RandomState(seed)), 'train_batch')


def test_focus_is_read_per_batch():
    ts = make_set()
    rng, ref = np.random.RandomState(3), np.random.RandomState(3)
    for focus in ('', 'head', 'leg', ''):                                    # 'leg': an empty semantic mask falls back to msk
        ts.cfg.sample_focus = focus
        same(ts.train_batch(1, rng), restated(1, ref, focus if focus == 'head' else ''), focus)


def test_a_yielded_batch_stays_valid():
    ts = make_set()
    gen = ts.batches(ORDER, np.random.RandomState(11), prefetch=2)
    first = next(gen)
    later = [next(gen) for _ in range(4)]                                    # four later batches drawn (two more are in flight)
    torch.cuda.synchronize()
    rng = np.random.RandomState(11)
    same(first, restated(ORDER[0], rng), 'first, after four more')
    for i, b in enumerate(later):
        same(b, restated(ORDER[1 + i], rng), ('later', i))
    gen.close()


def test_scene_tensors_are_referenced_not_copied():
    ts = make_set()
    a, b = ts.train_batch(2, np.random.RandomState(0)), ts.train_batch(2, np.random.RandomState(1))
    for k in SCENE_KEYS:
        assert a[k].data_ptr() == b[k].data_ptr() == ts.frames[2].scene[k].data_ptr(), k
    for k in SHARED_KEYS:
        assert a[k].data_ptr() == ts.shared[k].data_ptr() == ts.train_batch(0, np.random.RandomState(2))[k].data_ptr(), k
    assert a['ray_d'].data_ptr() != b['ray_d'].data_ptr()                  # output tensors are fresh per batch


def test_training_steps_fed_by_the_set_equal_host_fed_steps():
    """Three driver.train_step on the small test model: losses bit-equal whether the batches come from the set (prefetch 2) or are the
    restated host batches uploaded by hand."""
    cfg = make_cfg(table_log2=12, N_samples=16, patch_size=PATCH)
    sd0 = params.init_state_dict(cfg, seed=9)
    order = ORDER[:3]

    def run(feed):
        net = Network(cfg=copy.deepcopy(cfg))
        net.load_state_dict(sd0, strict=True)
        net = net.to(DEV).train()
        wrap = NetworkWrapper(net)
        opt = driver.make_optimizer(net, lr=5e-4, eps=1e-15)
        torch.manual_seed(5)                                                 # the jitter and the pair noise of the three steps
        losses = [driver.train_step(wrap, opt, batch, k + 1)[0] for k, batch in enumerate(feed)]
        return [float(l) for l in losses]

    ts = make_set(copy.deepcopy(cfg))
    mine = run(ts.batches(order, np.random.RandomState(7), prefetch=2))
    rng = np.random.RandomState(7)
    host = [restated(i, rng) for i in order]
    by_hand = run({k: (torch.from_numpy(v) if k in driver.HOST_KEYS else torch.from_numpy(v).to(DEV)) for k, v in b.items()} for b in host)
    assert [b['ray_d'].shape[1] for b in host] == [256, 256, 64]                # the third window is cut by the box: count < w h
    print('losses fed by the set :', ['%.9g' % v for v in mine])
    print('losses fed by the host:', ['%.9g' % v for v in by_hand])
    assert all(np.isfinite(mine)) and mine[0] > 0
    assert [np.float32(v).tobytes() for v in mine] == [np.float32(v).tobytes() for v in by_hand], (mine, by_hand)


def test_batch_fn_feeds_driver_train():
    cfg = make_cfg(table_log2=12, N_samples=16, patch_size=PATCH)
    net = Network(cfg=copy.deepcopy(cfg))
    net.load_state_dict(params.init_state_dict(cfg, seed=9), strict=True)
    net = net.to(DEV).train()
    ts = make_set(net.cfg)                                                   # the set reads the config the training stages write
    out = driver.train(NetworkWrapper(net), driver.make_optimizer(net, lr=5e-4, eps=1e-15), ts.batch_fn([0, 1, 2, 0], np.random.RandomState(1)),
                       epochs=2, ep_iter=2, stages=[{'_start': 0, 'sample_focus': ''}, {'_start': 1, 'sample_focus': 'head'}])
    assert out['iterations'] == 4 and np.isfinite(out['losses']).all() and net.cfg.sample_focus == 'head'


@pytest.mark.parametrize('index', [0, 2])
def test_eval_batch_equals_rays_within_bounds(index):
    ts = make_set()
    fr, shared = frames()
    f = fr[index]
    b = ts.test_batch(index)
    ray_o, ray_d, near, far, mask = rays.rays_within_bounds(H, W, f['K'], f['R'], f['T'], f['scene']['wbounds'], DEV)
    m = mask.cpu().numpy()
    assert 0 < m.sum() and torch.equal(b['mask_at_box'], mask.reshape(1, -1))
    for k, v in (('ray_o', ray_o), ('ray_d', ray_d), ('near', near), ('far', far)):
        assert torch.equal(b[k], v[None]), k
    assert np.array_equal(b['rgb'][0].cpu().numpy(), f['img'][m]) and np.array_equal(b['occupancy'][0].cpu().numpy(), f['msk'][m] > 0)
    assert int(b['H']) == H and int(b['W']) == W and not b['H'].is_cuda
    for k in SCENE_KEYS:
        assert b[k].data_ptr() == ts.frames[index].scene[k].data_ptr(), k
    # the batch renders: the eval loop of the driver on the resident sequence
    cfg = make_cfg(table_log2=12, N_samples=16)
    net = Network(cfg=copy.deepcopy(cfg))
    net.load_state_dict(params.init_state_dict(cfg, seed=9), strict=True)
    out = driver.run_evaluate(net.to(DEV), (ts.test_batch(i) for i in (index,)), device=DEV, in_flight=1)
    assert len(out['psnr']) == 1 and np.isfinite(out['psnr'][0])
