"""CPU: the NumPy restatement of the training-patch path (tests/patch_reference.py: the window draw and the contract of
include/invr_batch.h) against the imported reference's recorded outputs (tests/golden/patch_small.npz): every decision exact — the
window, the rays kept, their order — and every float bit for bit."""
import numpy as np
import pytest

from tests import patch_reference as P

CASES = [c['name'] for c in P.golden_cases()]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_the_fixture_holds_what_it_is_for():
    cs = P.golden_cases()
    sides = {c['window'][2] for c in cs}
    assert {56, 64} <= sides
    cut = [c for c in cs if 0 < c['mask_at_box'].sum() < c['mask_at_box'].size]
    assert len(cut) >= 3                                                     # windows the box silhouette cuts
    assert any(c['focus'] == 'head' and c['cropped'] for c in cs)            # a focused crop
    assert any(c['focus'] != '' and not c['cropped'] for c in cs)            # crop_image_msk returned None: the whole frame, float64 K
    assert any(c['focus'] == 'body' for c in cs)                             # an empty semantic mask: falls back to msk
    clamped = 0
    for c in cs:
        b = P.crop_rect(P.ref_mask(c), c['H'], c['W'], c['patch_size'])
        x_lo, y_lo, x_hi, y_hi = (0, 0, c['W'], c['H']) if b is None else (int(v) for v in b.reshape(-1))
        assert (b is not None) == c['cropped']
        x0, y0, w, h = c['window']
        clamped += x0 == x_lo or y0 == y_lo or x0 + w == x_hi or y0 + h == y_hi
    assert clamped >= 2


@pytest.mark.parametrize('name', CASES)
def test_draw_restated(name):
    c = next(c for c in P.golden_cases() if c['name'] == name)
    x0, y0, w, h, K32 = P.draw(c['msk'], P.ref_mask(c), c['K'], c['patch_size'], np.random.RandomState(c['seed']))
    assert (x0, y0, w, h) == c['window']
    assert K32.dtype == np.float32 and bits(K32) == bits(c['K32'])
    np.random.seed(c['seed'])                                                # rng=None: the global generator, as the reference
    assert P.draw(c['msk'], P.ref_mask(c), c['K'], c['patch_size'])[:4] == c['window']


@pytest.mark.parametrize('name', CASES)
def test_patch_batch_restated(name):
    c = next(c for c in P.golden_cases() if c['name'] == name)
    x0, y0, w, h = c['window']
    k_inv, R, T, o = P.camera(c['K32'], c['R'], c['T'])
    r = P.patch_batch(c['img'], c['msk'], x0, y0, w, h, k_inv, R, T, o, c['wbounds'])
    assert r['count'] == len(c['near']) == int(c['mask_at_box'].sum())
    assert np.array_equal(r['mask_at_box'], c['mask_at_box'])
    assert np.array_equal(r['coord'], c['coord']) and r['coord'].dtype == np.uint8
    assert np.array_equal(r['occupancy'], c['occupancy'])
    for k in ('ray_d', 'near', 'far'):
        assert r[k].dtype == np.float32 and bits(r[k]) == bits(c[k]), k
    assert bits(r['rgb']) == bits(c['img'][y0:y0 + h, x0:x0 + w][c['mask_at_box'].reshape(h, w).astype(bool)])
