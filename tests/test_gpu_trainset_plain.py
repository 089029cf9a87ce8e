"""GPU: invr.trainset.TrainSet in mode 'plain' — N_rand ray batches formed on the device from three resident synthetic frames (96 x 80,
pose_seed 0..2, the third with a face class) against the NumPy restatement of the reference's plain branch applied on the host with
the same seed (tests/sample_reference.py: plain_batch): key by key the same shapes, dtypes and bits, with and without prefetch; the
mode=None rule follows the cfg flags per batch; a yielded batch stays valid; scene tensors are referenced, not copied; plain-MSE
training steps fed by the set equal the same steps fed by host-built batches uploaded by hand; batch_fn feeds driver.train."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import patch_reference as P              # noqa: E402  (checker only)
from tests import sample_reference as S             # noqa: E402  (checker only)
from invr import scene, params, driver               # noqa: E402
from invr.config import make_cfg                     # noqa: E402
from invr.network import Network                     # noqa: E402
from invr.trainer import NetworkWrapper              # noqa: E402
from invr.trainset import TrainSet                   # noqa: E402

DEV = 'cuda:0'
H, W, PATCH, N_RAND = 96, 80, 16, 200
RATIOS = (0.5, 0.25)                # frames 0 and 1 have no face: its quarter is dropped and drawn again in further rounds
SCENE_KEYS = ('A', 'big_A', 'pbw', 'pbounds', 'wbounds', 'R', 'Th', 'ppts', 'part_pts', 'part_pbw', 'lengths2', 'bounds')
SHARED_KEYS = ('tuv', 'tbounds')
ORDER = [0, 1, 2, 1, 0, 2, 2, 0]
CAM_DIST = (1.6, 2.4, 3.0)


@functools.lru_cache(maxsize=None)
def frames():
    """Three frames of one body: (img, msk, orig_msk, sem, K, R, T, scene items, latent index) each, and the shared items.  Read-only."""
    out, shared = [], None
    for f in range(3):
        b, ex = scene.make_scene(H, W, seed=0, frame=3 + 11 * f, cam_dist=CAM_DIST[f], pose_seed=f)
        msk, sem = P.synthetic_masks(H, W, cx=W / 2.0 + 3 * f, ay=0.40 * H)
        if f == 2:
            msk = S.with_face(msk, H, W)
        out.append(dict(img=P.synthetic_image(H, W, 20 + f, msk), msk=msk, orig_msk=S.synthetic_orig_msk(msk), sem=sem, K=ex['K'], R=ex['Rc'],
                        T=ex['Tc'], scene={k: b[k][0] for k in SCENE_KEYS}, latent=3 + 11 * f))
        shared = {k: b[k][0] for k in SHARED_KEYS}
    return out, shared


def plain_cfg(**kw):
    return make_cfg(**dict(dict(patch_size=PATCH, N_rand=N_RAND, body_sample_ratio=RATIOS[0], face_sample_ratio=RATIOS[1]), **kw))


def make_set(cfg=None):
    fr, shared = frames()
    ts = TrainSet(cfg or plain_cfg(), device=DEV, shared=shared)
    for f in fr:
        ts.add_frame(f['img'], f['msk'], f['K'], f['R'], f['T'], f['scene'], sem_masks=f['sem'], latent_index=f['latent'], cam_ind=1,
                     orig_msk=f['orig_msk'])
    return ts


def collate(f, b, shared):
    b.update(frame_dim=np.array(f['latent'] / 100).astype(np.float32), latent_index=np.int64(f['latent']), bw_latent_index=np.int64(f['latent']),
             frame_index=np.int64(f['latent']), cam_ind=np.int64(1))
    b.update(shared)
    b.update(f['scene'])
    return {k: np.ascontiguousarray(np.asarray(v)[None]) for k, v in b.items()}


def restated(index, rng, n_rand=N_RAND, rounds=None):
    """The plain batch of frame `index` as the restatement forms it on the host: numpy arrays with the leading batch dimension of 1."""
    fr, shared = frames()
    f = fr[index]
    r = S.plain_batch(f['img'], f['msk'], f['orig_msk'], f['K'], f['R'], f['T'], f['scene']['wbounds'], n_rand, RATIOS[0], RATIOS[1], rng)
    if rounds is not None:
        rounds.append(r['rounds'])
    b = {k: r[k] for k in ('rgb', 'occupancy', 'coord', 'ray_o', 'ray_d', 'near', 'far', 'mask_at_box')}
    b.update(H=np.int64(H), W=np.int64(W))
    return collate(f, b, shared)


def restated_patch(index, rng):
    fr, shared = frames()
    f = fr[index]
    x0, y0, w, h, K32 = P.draw(f['msk'], f['msk'], f['K'], PATCH, rng)
    k_inv, R, T, o = P.camera(K32, f['R'], f['T'])
    r = P.patch_batch(f['img'], f['msk'], x0, y0, w, h, k_inv, R, T, o, f['scene']['wbounds'])
    b = {'rgb': r['rgb'], 'occupancy': r['occupancy'].astype(bool), 'coord': r['coord'], 'ray_o': np.broadcast_to(o.astype(np.float32), (r['count'], 3)),
         'ray_d': r['ray_d'], 'near': r['near'], 'far': r['far'], 'mask_at_box': r['mask_at_box'].astype(bool), 'H': np.int64(h), 'W': np.int64(w)}
    return collate(f, b, shared)


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
def test_plain_batches_equal_the_restatement_with_and_without_prefetch(seed):
    ts = make_set()
    ahead = list(ts.batches(ORDER, np.random.RandomState(seed), prefetch=2, mode='plain'))
    direct = list(ts.batches(ORDER, np.random.RandomState(seed), prefetch=0, mode='plain'))
    rng, rounds = np.random.RandomState(seed), []
    assert len(ahead) == len(direct) == len(ORDER)
    for i, index in enumerate(ORDER):
        want = restated(index, rng, rounds=rounds)
        same(ahead[i], want, ('prefetch=2', i))
        same(direct[i], want, ('prefetch=0', i))
    b = ahead[0]
    assert b['coord'].dtype == torch.int64 and b['occupancy'].dtype == torch.uint8 and b['mask_at_box'].dtype == torch.bool      # as the reference collates
    assert tuple(b['coord'].shape) == (1, N_RAND, 2) and bool(b['mask_at_box'].all()) and int(b['H']) == H and int(b['W']) == W
    assert {1, 7} <= set(torch.unique(b['occupancy']).tolist())                                                 # the byte of orig_msk, not a flag
    assert all(len(r) >= 2 for i, r in zip(ORDER, rounds) if i != 2) and any(r[0][1] > 0 for r in rounds)       # several rounds; a face class drawn from
    same(ts.train_batch(ORDER[0], np.random.RandomState(seed), mode='plain'), restated(ORDER[0], np.random.RandomState(seed)), 'train_batch')


def test_mode_none_follows_the_cfg_flags_per_batch():
    ts = make_set()
    rng, ref = np.random.RandomState(3), np.random.RandomState(3)
    for flag in (None, 'patch_sampling', None, 'use_ssim'):
        for k in ('use_lpips', 'patch_sampling', 'use_ssim', 'use_fourier', 'use_tv_image'):
            ts.cfg[k] = k == flag
        same(ts.train_batch(1, rng), restated(1, ref) if flag is None else restated_patch(1, ref), flag)
    # inside one generator too: the flag is read when the batch is drawn (driver.change_training_stages writes cfg between epochs)
    ts.cfg.use_ssim = False
    rng, ref = np.random.RandomState(4), np.random.RandomState(4)
    gen = ts.batches([0, 2, 1], rng, prefetch=0)
    same(next(gen), restated(0, ref), 'generator, plain')
    ts.cfg.patch_sampling = True
    same(next(gen), restated_patch(2, ref), 'generator, patch')
    ts.cfg.patch_sampling = False
    ts.cfg.N_rand = 33                                                       # read at every draw
    same(next(gen), restated(1, ref, n_rand=33), 'generator, plain again')
    # a frame without orig_msk gives patches under None, as before, and refuses mode='plain'
    fr, shared = frames()
    f = fr[0]
    old = TrainSet(plain_cfg(), device=DEV, shared=shared)
    old.add_frame(f['img'], f['msk'], f['K'], f['R'], f['T'], f['scene'], sem_masks=f['sem'], latent_index=f['latent'], cam_ind=1)
    same(old.train_batch(0, np.random.RandomState(5)), restated_patch(0, np.random.RandomState(5)), 'no orig_msk')
    with pytest.raises(ValueError, match='without orig_msk'):
        old.train_batch(0, np.random.RandomState(5), mode='plain')


def test_a_yielded_batch_stays_valid():
    ts = make_set()
    gen = ts.batches(ORDER, np.random.RandomState(11), prefetch=2, mode='plain')
    first = next(gen)
    later = [next(gen) for _ in range(5)]                                    # five later batches drawn (two more are in flight): the staging ring has wrapped
    torch.cuda.synchronize()
    rng = np.random.RandomState(11)
    same(first, restated(ORDER[0], rng), 'first, after five more')
    for i, b in enumerate(later):
        same(b, restated(ORDER[1 + i], rng), ('later', i))
    gen.close()


def test_a_batch_larger_than_the_constant_rows():
    """N_rand beyond the 65536 constant ray_o rows of a frame and the staging buffers' first size: both grow."""
    ts = make_set()
    ts.cfg.N_rand = 70000
    b = ts.train_batch(2, np.random.RandomState(1), mode='plain')
    same(b, restated(2, np.random.RandomState(1), n_rand=70000), 'N_rand 70000')
    ts.cfg.N_rand = N_RAND
    same(ts.train_batch(2, np.random.RandomState(2), mode='plain'), restated(2, np.random.RandomState(2)), 'back to %d' % N_RAND)


def test_scene_tensors_are_referenced_not_copied():
    ts = make_set()
    a, b = ts.train_batch(2, np.random.RandomState(0), mode='plain'), ts.train_batch(2, np.random.RandomState(1), mode='plain')
    for k in SCENE_KEYS:
        assert a[k].data_ptr() == b[k].data_ptr() == ts.frames[2].scene[k].data_ptr(), k
    for k in SHARED_KEYS:
        assert a[k].data_ptr() == ts.shared[k].data_ptr() == ts.train_batch(0, np.random.RandomState(2), mode='plain')[k].data_ptr(), k
    assert a['ray_d'].data_ptr() != b['ray_d'].data_ptr()                  # output tensors are fresh per batch
    assert a['ray_o'].data_ptr() == b['ray_o'].data_ptr() and a['mask_at_box'].data_ptr() == b['mask_at_box'].data_ptr()          # constant rows, viewed


def test_training_steps_fed_by_the_set_equal_host_fed_steps():
    """Three driver.train_step of the plain-MSE objective (use_lpips False) on the small test model: losses bit-equal whether the
    batches come from the set (prefetch 2) or are the restated host batches uploaded by hand."""
    cfg = plain_cfg(table_log2=12, N_samples=16)
    assert not cfg.use_lpips
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
    mine = run(ts.batches(order, np.random.RandomState(7), prefetch=2))       # mode None: no patch flag is set, the plain branch
    rng = np.random.RandomState(7)
    host = [restated(i, rng) for i in order]
    by_hand = run({k: (torch.from_numpy(v) if k in driver.HOST_KEYS else torch.from_numpy(v).to(DEV)) for k, v in b.items()} for b in host)
    assert [b['ray_d'].shape[1] for b in host] == [N_RAND] * 3
    print('losses fed by the set :', ['%.9g' % v for v in mine])
    print('losses fed by the host:', ['%.9g' % v for v in by_hand])
    assert all(np.isfinite(mine)) and mine[0] > 0
    assert [np.float32(v).tobytes() for v in mine] == [np.float32(v).tobytes() for v in by_hand], (mine, by_hand)


def test_batch_fn_feeds_driver_train():
    cfg = plain_cfg(table_log2=12, N_samples=16)
    net = Network(cfg=copy.deepcopy(cfg))
    net.load_state_dict(params.init_state_dict(cfg, seed=9), strict=True)
    net = net.to(DEV).train()
    ts = make_set(net.cfg)                                                   # the set reads the config the training stages write
    out = driver.train(NetworkWrapper(net), driver.make_optimizer(net, lr=5e-4, eps=1e-15), ts.batch_fn([0, 1, 2, 0], np.random.RandomState(1), prefetch=0),
                       epochs=2, ep_iter=2, stages=[{'_start': 0, 'N_rand': 128}, {'_start': 1, 'N_rand': 64}])
    assert out['iterations'] == 4 and np.isfinite(out['losses']).all() and net.cfg.N_rand == 64
    assert out['ray_samples'] == (2 * 128 + 2 * 64) * 16                     # the second epoch's batches were drawn under its stage
