"""CPU: the host side of plain sampling (invr.raysample, TrainSet.add_frame / draw_rays) without a device and without the library —
the default bound mask against the brute-force hull of tests/sample_reference.py, the per-frame classes against np.argwhere, and the
draw loop against the restatement and against the imported reference's recorded draws (tests/golden/sample_small.npz)."""
import numpy as np
import pytest

from tests import sample_reference as S
from invr import raysample, scene
from invr.config import make_cfg
from invr.trainset import TrainSet

CASES = [c['name'] for c in S.golden_cases()]


def case(name):
    return next(c for c in S.golden_cases() if c['name'] == name)


def one_frame_set(c, bound='golden', **cfg):
    cfg = dict(dict(N_rand=c['N_rand'], body_sample_ratio=c['body_ratio'], face_sample_ratio=c['face_ratio']), **cfg)
    ts = TrainSet(make_cfg(**cfg), device='cpu')
    ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']}, orig_msk=c['orig_msk'],
                 bound_mask=c['bound'] if bound == 'golden' else None)
    return ts


# ---- the bound mask -------------------------------------------------------------------------------------------------------------------
POINT_SETS = {
    'square': [(3, 2), (20, 2), (20, 17), (3, 17), (10, 10), (4, 4), (19, 3), (11, 2)],
    'skew': [(-5, 7), (14, 1), (33, 12), (29, 30), (8, 35), (2, 20), (15, 15), (20, 9)],
    'single_pixel': [(7, 5)] * 8,
    'segment': [(2, 3), (8, 6), (14, 9), (5, 4)] * 2,                    # collinear: (5, 4) is off the line, the hull is a sliver
    'collinear': [(2, 3), (8, 6), (14, 9), (4, 4)] * 2,
    'vertical': [(9, -4), (9, 50), (9, 7), (9, 8)] * 2,
    'outside': [(-30, -30), (-5, -8), (-12, -2), (-7, -20)] * 2,
    'around': [(-100, -100), (200, -90), (210, 180), (-95, 170)] * 2,
}


@pytest.mark.parametrize('name', sorted(POINT_SETS))
def test_hull_mask_equals_the_brute_force(name):
    pts = POINT_SETS[name]
    for H, W in ((24, 40), (1, 1), (37, 23)):
        got, want = raysample.hull_mask(pts, H, W), S.hull_mask(pts, H, W)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, H, W, np.argwhere(got != want))
    m = S.hull_mask(pts, 24, 40)                                               # the case is what it is there for
    if name == 'single_pixel':
        assert m.sum() == 1 and m[5, 7] == 1
    elif name == 'collinear':
        assert {tuple(p) for p in np.argwhere(m)} == {(3, 2), (4, 4), (5, 6), (6, 8), (7, 10), (8, 12), (9, 14)}
    elif name == 'vertical':
        assert np.array_equal(np.argwhere(m), np.stack([np.arange(24), np.full(24, 9)], 1))
    elif name == 'outside':
        assert m.sum() == 0
    elif name == 'around':
        assert m.all()
    else:
        assert 0 < m.sum() < m.size and all(m[y, x] for x, y in pts if 0 <= x < 40 and 0 <= y < 24)         # closed: the vertices belong to it


@pytest.mark.parametrize('pose', [dict(cam_dist=2.2), dict(cam_dist=1.6), dict(cam_dist=3.0, pose_seed=2), dict(cam_dist=1.1, pose_seed=1)])
def test_default_bound_mask_on_posed_boxes(pose):
    H, W = 48, 40
    b, ex = scene.make_scene(H, W, seed=0, **pose)
    wb = b['wbounds'][0]
    got = raysample.bound_mask(wb, ex['K'], ex['Rc'], ex['Tc'], H, W)
    pts, depth = S.corners_2d(wb, ex['K'], ex['Rc'], ex['Tc'])
    assert (depth > 0).all() and np.array_equal(raysample.bound_corners(wb, ex['K'], ex['Rc'], ex['Tc']), pts)
    assert np.array_equal(got, S.hull_mask(pts, H, W)) and got.any()


def test_a_box_that_projects_to_one_pixel():
    """A box of zero extent in front of the camera: all eight corners round to one pixel, the mask is that pixel."""
    K, R, T = np.array([[50.0, 0, 20], [0, 50, 24], [0, 0, 1]]), np.eye(3), np.array([[0.0], [0.0], [4.0]])
    wb = np.array([[0.24, -0.1, 0.0], [0.24, -0.1, 0.0]], np.float32)
    m = raysample.bound_mask(wb, K, R, T, 48, 40)
    assert m.sum() == 1 and m[23, 23] == 1 and np.array_equal(m, S.hull_mask(S.corners_2d(wb, K, R, T)[0], 48, 40))     # x = 20 + 50 * 0.24 / 4, y = 24 - 50 * 0.1 / 4


def test_a_corner_behind_the_camera_raises():
    K, R, T = np.array([[50.0, 0, 20], [0, 50, 24], [0, 0, 1]]), np.eye(3), np.array([[0.0], [0.0], [0.5]])
    wb = np.array([[-1, -1, -1], [1, 1, 1]], np.float32)
    with pytest.raises(ValueError, match='in front of the camera'):
        raysample.bound_mask(wb, K, R, T, 48, 40)
    c = S.golden_cases()[0]
    with pytest.raises(ValueError, match='in front of the camera'):
        TrainSet(make_cfg(), device='cpu').add_frame(c['img'], c['msk'], K, R, T, {'wbounds': wb}, orig_msk=c['orig_msk'])


@pytest.mark.parametrize('tag', ['a', 'b', 'f'])
def test_default_bound_mask_equals_the_goldens(tag):
    """On the golden scenes the hull equals the six faces the reference filled (with the golden maker's closed even-odd fillPoly)."""
    c = next(c for c in S.golden_cases() if c['scene'] == tag)
    assert np.array_equal(raysample.bound_mask(c['wbounds'], c['K'], c['R'], c['T'], c['H'], c['W']), c['bound'])


# ---- classes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['a', 'b', 'f'])
def test_frame_classes_against_argwhere(tag):
    c = next(c for c in S.golden_cases() if c['scene'] == tag)
    f = one_frame_set(c).frames[0]
    coords = S.classes(c['msk'], c['bound'])
    planes, prefix = S.planes_and_prefix(coords, c['H'], c['W'])
    assert [int(v) for v in f.classes.sizes] == [len(co) for co in coords] and (len(coords[1]) > 0) == (tag == 'f')
    assert f.classes.planes.dtype == np.uint64 and np.array_equal(f.classes.planes, planes)
    assert f.classes.row_prefix.dtype == np.int32 and np.array_equal(f.classes.row_prefix, prefix)
    assert np.array_equal(f.planes.numpy().view(np.uint64), planes) and np.array_equal(f.row_prefix.numpy(), prefix)      # what is uploaded
    rays_o, rays_d = S.frame_rays(c['H'], c['W'], c['K'], c['R'], c['T'])
    inside = S.near_far(c['wbounds'], rays_o, rays_d.reshape(-1, 3))[2].reshape(c['H'], c['W'])
    for k in range(3):
        assert np.array_equal(f.classes.inside[k], inside[coords[k][:, 0], coords[k][:, 1]]), k
    assert tag == 'b' or not f.classes.inside[2].all()                        # 'a', 'f': hull pixels whose ray misses the box


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_draw_rays_returns_the_reference_draw(name):
    c = case(name)
    ts = one_frame_set(c)
    sel = ts.draw_rays(0, np.random.RandomState(c['seed']))
    coords = S.classes(c['msk'], c['bound'])
    assert sel.dtype == np.int32 and sel.shape == (len(c['near']), 2) and len(sel) == sum(r[3] for r in c['rounds']) >= c['N_rand']
    assert np.array_equal(np.stack([coords[k][r] for k, r in sel]), c['coord'])          # the reference's pixels in its order
    np.random.seed(c['seed'])                                                # rng=None draws from the global generator
    assert np.array_equal(ts.draw_rays(0), sel)
    mine = S.plain_batch(c['img'], c['msk'], c['orig_msk'], c['K'], c['R'], c['T'], c['wbounds'], c['N_rand'], c['body_ratio'], c['face_ratio'],
                         np.random.RandomState(c['seed']), bound=c['bound'])
    assert np.array_equal(mine['sel'], sel) and mine['rounds'] == c['rounds']
    assert np.array_equal(mine['coord'], c['coord']) and np.array_equal(mine['occupancy'], c['occupancy'])
    for k in ('ray_d', 'near', 'far'):
        bound = c['ulp'] + 1 if c['ulp'] else 0
        assert mine[k].dtype == np.float32 and S.ulp_distance(mine[k], c[k]) <= bound, (name, k)


def test_the_golden_cases_are_what_they_are_there_for():
    by = {c['name']: c for c in S.golden_cases()}
    rounds = {n: c['rounds'] for n, c in by.items()}
    assert any(len(r) == 1 for r in rounds.values())
    assert any(len(r) >= 2 and by[n]['face_ratio'] == 0 for n, r in rounds.items())                   # rays that miss the box alone force a round
    assert any(r[0][1] > 0 for r in rounds.values())                                                  # a face class that is drawn from
    assert any(r[0][1] == -1 and by[n]['face_ratio'] > 0 and len(r) >= 2 for n, r in rounds.items())  # an empty one: its share is dropped
    assert {c['N_rand'] for c in by.values()} == {1, 100, 1024}


def test_draw_rays_agrees_with_the_restatement_over_many_seeds():
    for tag, ratios in (('a', (0.5, 0.0)), ('a', (0.2, 0.5)), ('f', (0.5, 0.25)), ('f', (0.0, 1.0)), ('b', (1.0, 0.0))):
        c = next(c for c in S.golden_cases() if c['scene'] == tag)
        ts = one_frame_set(c, bound='default')
        coords = S.classes(c['msk'], c['bound'])
        rays_o, rays_d = S.frame_rays(c['H'], c['W'], c['K'], c['R'], c['T'])
        inside = S.near_far(c['wbounds'], rays_o, rays_d.reshape(-1, 3))[2].reshape(c['H'], c['W'])
        for seed in range(12):
            for n_rand in (1, 7, 300):
                ts.cfg.N_rand, ts.cfg.body_sample_ratio, ts.cfg.face_sample_ratio = n_rand, ratios[0], ratios[1]      # read at every draw
                want, _ = S.draw_rays(coords, inside, n_rand, ratios[0], ratios[1], np.random.RandomState(seed))
                assert np.array_equal(ts.draw_rays(0, np.random.RandomState(seed)), want), (tag, ratios, seed, n_rand)


def test_plain_sampling_raises_where_it_cannot_run():
    c = S.golden_cases()[0]
    ts = TrainSet(make_cfg(), device='cpu')
    ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']})
    with pytest.raises(ValueError, match='without orig_msk'):
        ts.draw_rays(0, np.random.RandomState(0))
    with pytest.raises(ValueError, match='without orig_msk'):
        ts.train_batch(0, np.random.RandomState(0), mode='plain')
    with pytest.raises(ValueError, match='mode must be'):
        ts.train_batch(0, np.random.RandomState(0), mode='rays')
    with pytest.raises(ValueError, match='without orig_msk'):
        ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']}, bound_mask=c['bound'])
    with pytest.raises(ValueError, match='0 / 1'):
        ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']}, orig_msk=c['orig_msk'], bound_mask=c['bound'] * 255)
    for key in ('prune_using_geo', 'train_with_coord', 'sample_using_mse'):
        ts = one_frame_set(c, **{key: True})
        with pytest.raises(ValueError, match='unsupported configuration ' + key):
            ts.draw_rays(0, np.random.RandomState(0))
    empty = np.zeros_like(c['msk'])                                            # no body pixel: the reference's randint(0, 0, n) raises
    ts = TrainSet(make_cfg(), device='cpu')
    ts.add_frame(c['img'], empty, c['K'], c['R'], c['T'], {'wbounds': c['wbounds']}, orig_msk=c['orig_msk'])
    with pytest.raises(ValueError, match='frame 0 has no body pixel'):
        ts.draw_rays(0, np.random.RandomState(0))


def test_mode_none_follows_the_reference_rule():
    c = S.golden_cases()[0]
    ts = one_frame_set(c)
    ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']})          # frame 1: no orig_msk, patches only
    assert ts._mode(None, 0) == 'plain' and ts._mode(None, 1) == 'patch'
    for flag in ('use_lpips', 'patch_sampling', 'use_ssim', 'use_fourier', 'use_tv_image'):
        ts.cfg[flag] = True
        assert ts._mode(None, 0) == 'patch' and ts._mode('plain', 0) == 'plain', flag
        ts.cfg[flag] = False
        assert ts._mode(None, 0) == 'plain' and ts._mode('patch', 0) == 'patch', flag


def test_config_defaults_and_adopt():
    from invr import config
    assert config.DEFAULTS['N_rand'] == 1024 and config.DEFAULTS['body_sample_ratio'] == 0.5 and config.DEFAULTS['face_sample_ratio'] == 0.0
    saved = dict(config.cfg)
    try:
        c = config.adopt(dict(config.DEFAULTS, N_rand=256, body_sample_ratio=0.25, face_sample_ratio=0.125, patch_sampling=True))
        assert c.N_rand == 256 and c.body_sample_ratio == 0.25 and c.face_sample_ratio == 0.125 and c.patch_sampling is True
    finally:
        config.set_cfg(config._node(saved))
