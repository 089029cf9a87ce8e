"""CPU: invr.trainset.TrainSet without a device and without the library — construction, the per-frame host precomputation and `draw`
against the imported reference's recorded windows (tests/golden/patch_small.npz)."""
import numpy as np
import pytest

from tests import patch_reference as P
from invr.config import make_cfg
from invr.trainset import TrainSet, bounding_rect, padding_bbox

CASES = [c['name'] for c in P.golden_cases()]


def one_frame_set(c, **cfg):
    ts = TrainSet(make_cfg(patch_size=c['patch_size'], sample_focus=c['focus'], **cfg), device='cpu')
    ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']}, sem_masks=c['sem'])
    return ts


@pytest.mark.parametrize('name', CASES)
def test_draw_returns_the_reference_window(name):
    c = next(c for c in P.golden_cases() if c['name'] == name)
    ts = one_frame_set(c)
    x0, y0, w, h, K32 = ts.draw(0, np.random.RandomState(c['seed']))
    assert (x0, y0, w, h) == c['window']
    assert K32.dtype == np.float32 and K32.tobytes() == c['K32'].tobytes()
    np.random.seed(c['seed'])                                                # rng=None draws from the global generator
    assert ts.draw(0)[:4] == c['window']


def test_draw_reads_the_focus_at_call_time():
    c = next(c for c in P.golden_cases() if c['focus'] == 'head' and c['cropped'])
    ts = one_frame_set(c)
    plain, focused = [], []
    for seed in range(10):
        ts.cfg.sample_focus = ''                                             # driver.change_training_stages writes cfg between epochs
        plain.append(ts.draw(0, np.random.RandomState(seed))[:4])
        assert plain[-1] == P.draw(c['msk'], c['msk'], c['K'], c['patch_size'], np.random.RandomState(seed))[:4]
        ts.cfg.sample_focus = 'head'
        focused.append(ts.draw(0, np.random.RandomState(seed))[:4])
        assert focused[-1] == P.draw(c['msk'], c['sem'][2], c['K'], c['patch_size'], np.random.RandomState(seed))[:4]
    assert plain != focused and focused[c['seed']] == c['window']


def test_draw_agrees_with_the_restatement_over_many_seeds():
    for tag in ('a', 'b', 'c'):
        c = next(c for c in P.golden_cases() if c['scene'] == tag)
        for focus in ('', 'head', 'leg'):
            ts = one_frame_set(dict(c, focus=focus))
            for seed in range(40):
                got = ts.draw(0, np.random.RandomState(seed))
                want = P.draw(c['msk'], P.ref_mask(dict(c, focus=focus)), c['K'], c['patch_size'], np.random.RandomState(seed))
                assert got[:4] == want[:4] and got[4].tobytes() == want[4].tobytes(), (tag, focus, seed)


def test_a_window_that_cannot_fit_raises():
    H, W = 40, 120
    msk = np.zeros((H, W), np.uint8)
    msk[2:38, 20:90] = 1
    img = np.zeros((H, W, 3), np.float32)
    c = P.golden_cases()[0]
    ts = TrainSet(make_cfg(patch_size=36), device='cpu')
    ts.add_frame(img, msk, c['K'], c['R'], c['T'], {'wbounds': c['wbounds']})
    # bounding rectangle 70 x 36 >= 36: cropped to rows 0..39 -> 39 rows; m = 36, side = (randint(28, 36) | 7) + 1 = 32 or 40; 40 > 39
    seen = set()
    for seed in range(40):
        try:
            seen.add(ts.draw(0, np.random.RandomState(seed))[2])
        except ValueError as e:
            assert 'frame 0' in str(e) and '40 x 40' in str(e)
            seen.add('raised')
    assert seen == {32, 'raised'}


def test_add_frame_copies_the_host_arrays():
    c = P.golden_cases()[0]
    img, msk = c['img'].copy(), c['msk'].copy()
    ts = TrainSet(make_cfg(patch_size=c['patch_size']), device='cpu')
    ts.add_frame(img, msk, c['K'], c['R'], c['T'], {'wbounds': c['wbounds']})
    img[:], msk[:] = 0, 0                                                    # a loader that reuses its buffers for the next frame
    assert ts.draw(0, np.random.RandomState(c['seed']))[:4] == c['window']
    assert np.array_equal(ts.frames[0].img.numpy(), c['img']) and np.array_equal(ts.frames[0].msk.numpy(), c['msk'])


def test_focus_without_semantic_masks_raises():
    c = P.golden_cases()[0]
    ts = TrainSet(make_cfg(patch_size=c['patch_size'], sample_focus='head'), device='cpu')
    ts.add_frame(c['img'], c['msk'], c['K'], c['R'], c['T'], {'wbounds': c['wbounds']})
    with pytest.raises(ValueError, match='sem_masks'):
        ts.draw(0, np.random.RandomState(0))


def test_rectangles_restated():
    m = np.zeros((50, 60), np.uint8)
    assert bounding_rect(m) == (0, 0, 0, 0)
    m[7:19, 11:40] = 100
    m[30, 5] = 1
    assert bounding_rect(m) == (5, 7, 35, 24) == P.bounding_rect(m)
    for (x, y, w, h) in ((5, 7, 35, 24), (20, 3, 8, 40), (3, 20, 50, 6), (0, 0, 60, 50)):
        b = np.zeros((50, 60), np.uint8)
        b[y:y + h, x:x + w] = 1
        assert padding_bbox(x, y, w, h, 50, 60) == tuple(int(v) for v in P.crop_rect(b, 50, 60, 1).reshape(-1))


def test_config_defaults_and_adopt():
    from invr import config
    assert config.DEFAULTS['patch_size'] == 64 and config.DEFAULTS['sample_focus'] == ''
    saved = dict(config.cfg)
    try:
        c = config.adopt(dict(config.DEFAULTS, patch_size=32, sample_focus='head'))
        assert c.patch_size == 32 and c.sample_focus == 'head'
    finally:
        config.set_cfg(config._node(saved))
