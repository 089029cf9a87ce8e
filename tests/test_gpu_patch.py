"""GPU: invr_patch_batch (csrc/k_batch.hip) through the C ABI of include/invr_batch.h against the NumPy restatement of its contract
(tests/patch_reference.py) and against the imported reference's recorded outputs (tests/golden/patch_small.npz).

Everything is exact: floats bit for bit, bytes and the count equal.  Every output buffer is pre-filled with a sentinel: rows at or
past `count` keep it, and two calls over differently dirtied buffers give the same bits.

Windows: 1x1, 7x3, 8x8, 16x24, 56x56, 64x64, 65x33 (rows straddle waves) on a 96 x 80 frame; 128x96 (12 rounds of 1024 pixels) and
256x256 (the limit: 64 rounds) on a 300 x 280 one; each at the frame's origin, at its far corner and in the interior.  Boxes per window
(MODES): one that covers it (count = w h), one whose silhouette cuts it, a speck of fewer than 64 pixels in its middle (whole waves
without a set pixel), one that misses it (count = 0).
tests/test_hostsim_patch_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import patch_reference as P              # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
FRAMES = {'small': (96, 80), 'large': (300, 280)}                            # (H, W)
WINDOWS = [('small', 1, 1), ('small', 7, 3), ('small', 8, 8), ('small', 16, 24), ('small', 56, 56), ('small', 64, 64), ('small', 65, 33),
           ('large', 128, 96), ('large', 256, 256)]
SMALL = WINDOWS[:-1]                                                         # (the wave machine leaves 256x256 to HOSTSIM_FULL=1)
MODES = ('cover', 'cut', 'speck', 'miss')
KEYS = ('ray_d', 'near', 'far', 'rgb', 'occupancy', 'coord', 'mask_at_box')
FILLS = (0xA5, 0x3C)                                                         # sentinels: as floats -2.87e-16 and 0.0115, as bytes neither 0 nor 1


@functools.lru_cache(maxsize=None)
def frame(which):
    """-> (img (H,W,3) fp32, msk (H,W) uint8 with values 0 / 1 / 100, K, R, T) of a seeded frame; the pixels include -0.0, an inf and
    NaNs of two payloads: rgb is a bit copy."""
    H, W = FRAMES[which]
    g = np.random.RandomState(H)
    img = g.rand(H, W, 3).astype(np.float32)
    bits = img.view(np.uint32)
    bits[0, 0] = (0x80000000, 0x7F800000, 0x7FC00001)
    bits[H - 1, W - 1] = (0xFFC12345, 0x00000001, 0x7F7FFFFF)
    msk = g.choice(np.array([0, 1, 100], np.uint8), size=(H, W))
    f = 1.2 * max(H, W)
    K = np.array([[f, 0, W / 2.0 + 0.3], [0, 1.01 * f, H / 2.0 - 0.7], [0, 0, 1]])
    from invr.scene import rodrigues
    return img, msk, K, rodrigues(np.array([0.1, -0.2, 0.05])), np.array([[0.1], [-0.05], [0.2]])


@functools.lru_cache(maxsize=None)
def device_frame(which, dev):
    img, msk = frame(which)[:2]
    return torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev)


def window_camera(which, x0, y0):
    """The window's float32 intrinsic matrix as random_crop_image forms it, and the host arrays of the call."""
    _, _, K, R, T = frame(which)
    K32 = K.copy()
    K32[0, 2] -= x0
    K32[1, 2] -= y0
    return P.camera(K32.astype(np.float32), R, T)


def box(which, x0, y0, w, h, mode):
    """A world box (2,3) fp32 whose projection is about a square of radius r pixels around the window's local pixel (u, v)."""
    _, _, K, R, T = frame(which)
    u, v, r = {'cover': (w / 2.0, h / 2.0, 4.0 * max(w, h) + 50.0), 'cut': (0.0, 0.0, max(w, h) / 2.0 + 0.4),
               'speck': (w / 2.0, h / 2.0, 2.3), 'miss': (w / 2.0 + 10.0 * max(w, h) + 500.0, h / 2.0, 3.0)}[mode]
    depth = 3.0
    pc = np.linalg.inv(K) @ np.array([x0 + u, y0 + v, 1.0]) * depth
    centre = (pc - T.ravel()) @ R
    half = r * depth / K[0, 0]
    return np.stack([centre - half, centre + half]).astype(np.float32)


def placements(which, w, h):
    H, W = FRAMES[which]
    return [(0, 0), (W - w, H - h), ((W - w) // 2 + (1 if W - w > 1 else 0), (H - h) // 3)]


def run(img, msk, H, W, window, cam, bounds, fill):
    """One call over buffers pre-filled with the byte `fill` -> {key: ndarray of all w h rows}, count."""
    x0, y0, w, h = window
    k_inv, R, T, o = cam
    n = w * h
    shape = {'ray_d': (n, 3), 'near': (n,), 'far': (n,), 'rgb': (n, 3), 'occupancy': (n,), 'coord': (n, 2), 'mask_at_box': (n,)}
    o_t = {}
    for k in KEYS:
        dt = torch.float32 if k in ('ray_d', 'near', 'far', 'rgb') else torch.uint8
        t = torch.empty(shape[k], dtype=dt, device=DEV)
        t.view(torch.uint8).fill_(fill)
        o_t[k] = t
    count = torch.full((1,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    f32 = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    u8 = torch.uint8
    _abi.check(_abi.lib().invr_patch_batch(
        _abi.ptr(img), _abi.ptr(msk, u8), H, W, x0, y0, w, h, f32(k_inv), f64(R), f64(T), f64(o), f32(bounds), _abi.ptr(o_t['ray_d']),
        _abi.ptr(o_t['near']), _abi.ptr(o_t['far']), _abi.ptr(o_t['rgb']), _abi.ptr(o_t['occupancy'], u8), _abi.ptr(o_t['coord'], u8),
        _abi.ptr(o_t['mask_at_box'], u8), _abi.ptr(count, torch.int32), _abi.stream_ptr()))
    if DEV != 'cpu':
        torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in o_t.items()}, int(count.cpu()[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def check(got, count, want, n, fill, tag):
    assert count == want['count'], (tag, count, want['count'])
    assert np.array_equal(got['mask_at_box'], want['mask_at_box']), tag           # written for every pixel
    for k in KEYS[:-1]:
        assert got[k].dtype == want[k].dtype, (tag, k)
        assert np.array_equal(bits(got[k][:count]), bits(want[k])), (tag, k)     # bit-equal floats, exact bytes
        assert (bits(got[k][count:]) == fill).all(), (tag, k, 'a row at or past count was written')


@pytest.mark.parametrize('win', WINDOWS, ids=lambda w: '%s_%dx%d' % w)
def test_patch_against_the_contract(win):
    which, w, h = win
    H, W = FRAMES[which]
    img, msk = frame(which)[:2]
    img_d, msk_d = device_frame(which, DEV)
    n = w * h
    for x0, y0 in placements(which, w, h):
        cam = window_camera(which, x0, y0)
        for mode in MODES:
            bounds = box(which, x0, y0, w, h, mode)
            want = P.patch_batch(img, msk, x0, y0, w, h, *cam, bounds)
            tag = (win, x0, y0, mode)
            # the case is what it is there for
            if mode == 'cover':
                assert want['count'] == n, tag
            elif mode == 'miss':
                assert want['count'] == 0, tag
            elif mode == 'cut' and n >= 64:
                assert 0 < want['count'] < n, tag
            elif mode == 'speck' and n >= 16 * 24:
                assert 0 < want['count'] < 64, tag
                waves = np.add.reduceat(want['mask_at_box'].astype(np.int64), np.arange(0, n, 64))
                assert (waves == 0).any() and (waves > 0).any(), tag             # whole waves without a set pixel
            got, count = run(img_d, msk_d, H, W, (x0, y0, w, h), cam, bounds, FILLS[0])
            check(got, count, want, n, FILLS[0], tag)
            if mode in ('cut', 'speck'):                                         # the same bits over differently dirtied buffers
                again, count2 = run(img_d, msk_d, H, W, (x0, y0, w, h), cam, bounds, FILLS[1])
                assert count2 == count
                for k in KEYS:
                    rows = n if k == 'mask_at_box' else count
                    assert np.array_equal(bits(again[k][:rows]), bits(got[k][:rows])), (tag, k)
                    assert (bits(again[k][rows:]) == FILLS[1]).all(), (tag, k)


def test_rgb_is_a_bit_copy():
    """-0.0, an inf, a denormal and NaN payloads of the frame's corner pixels arrive unchanged."""
    img, msk = frame('small')[:2]
    H, W = FRAMES['small']
    img_d, msk_d = device_frame('small', DEV)
    for x0, y0 in ((0, 0), (W - 8, H - 8)):
        cam = window_camera('small', x0, y0)
        got, count = run(img_d, msk_d, H, W, (x0, y0, 8, 8), cam, box('small', x0, y0, 8, 8, 'cover'), FILLS[0])
        assert count == 64
        assert np.array_equal(bits(got['rgb']), bits(img[y0:y0 + 8, x0:x0 + 8].reshape(-1, 3)))
        assert np.array_equal(got['occupancy'], (msk[y0:y0 + 8, x0:x0 + 8].reshape(-1) > 0).astype(np.uint8))


@pytest.mark.parametrize('name', [c['name'] for c in P.golden_cases()])
def test_patch_against_the_reference_golden(name):
    """The windows the reference drew, its float32 K, its rays: ray_d / near / far bit-equal, coord / mask_at_box / occupancy exact."""
    c = next(c for c in P.golden_cases() if c['name'] == name)
    x0, y0, w, h = c['window']
    img_d, msk_d = torch.from_numpy(c['img']).to(DEV), torch.from_numpy(c['msk']).to(DEV)
    cam = P.camera(c['K32'], c['R'], c['T'])
    got, count = run(img_d, msk_d, c['H'], c['W'], c['window'], cam, c['wbounds'], FILLS[0])
    assert count == len(c['near']) == int(c['mask_at_box'].sum())
    assert np.array_equal(got['mask_at_box'], c['mask_at_box'])
    for k in ('ray_d', 'near', 'far'):
        assert np.array_equal(bits(got[k][:count]), bits(c[k])), (name, k)
    assert np.array_equal(got['coord'][:count], c['coord']) and np.array_equal(got['occupancy'][:count], c['occupancy'])
    assert np.array_equal(bits(got['rgb'][:count]), bits(c['img'][y0:y0 + h, x0:x0 + w][c['mask_at_box'].reshape(h, w).astype(bool)]))
    for k in KEYS[:-1]:
        assert (bits(got[k][count:]) == FILLS[0]).all(), (name, k)
