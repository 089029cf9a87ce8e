"""GPU: invr_ray_batch (csrc/k_sample.hip) through the C ABI of include/invr_sample.h against the NumPy restatement of its contract
(tests/sample_reference.py: ray_batch, the pixel of a row looked up in np.argwhere lists) and against the imported reference's recorded
outputs (tests/golden/sample_small.npz).

Everything is exact: floats bit for bit, bytes and coordinates equal.  Every output buffer holds PAD rows more than the call writes and
is pre-filled with a sentinel: the rows at or past n keep it, and two calls over differently dirtied buffers give the same bits.

Frames: every W of 1, 63, 64, 65, 130 (a partial last word), 300 with every H of 1, 2, 97.  Class patterns: full, a single member at
(0,0), a single member at (H-1,W-1), members only at the word boundaries x = 63, 64, 127, 128, rows without a member between rows
with members, a checkerboard.  Selections: every rank of a class exactly once where the class is small (the select is then a bijection
onto np.argwhere), always rank 0 and the last rank, duplicates, the three classes interleaved; n of 1, 63, 64, 65, 257, 1024.
tests/test_hostsim_ray_batch_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sample_reference as S             # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
WIDTHS, HEIGHTS = (1, 63, 64, 65, 130, 300), (1, 2, 97)
SHAPES = [(h, w) for h in HEIGHTS for w in WIDTHS]
TRIPLES = (('full', 'first', 'last'), ('words', 'gaps', 'checker'))
SIZES = (1, 63, 64, 65, 257, 1024)
KEYS = ('ray_d', 'near', 'far', 'rgb', 'occupancy', 'coord')
FILLS = (0xA5, 0x3C)
PAD = 5
ALL_RANKS = 700                                      # classes up to this size are selected rank by rank


def pattern(name, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    if name == 'full':
        return np.ones((H, W), bool)
    if name == 'first':
        return (yy == 0) & (xx == 0)
    if name == 'last':
        return (yy == H - 1) & (xx == W - 1)
    if name == 'words':
        return np.isin(xx, (63, 64, 127, 128))
    if name == 'gaps':
        return np.isin(yy % 10, (0, 3, 4, 9)) & (xx % 3 != 1)
    if name == 'checker':
        return (xx + yy) % 2 == 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def frame(H, W):
    """-> (img (H,W,3) fp32, occ (H,W) uint8 of arbitrary bytes, K, R, T, bounds) of a seeded frame; the corner pixels hold -0.0, an inf,
    a denormal and NaNs of two payloads: rgb is a bit copy.  Read-only."""
    g = np.random.RandomState(1000 * H + W)
    img = g.rand(H, W, 3).astype(np.float32)
    bits = img.view(np.uint32)
    bits[0, 0] = (0x80000000, 0x7F800000, 0x7FC00001)
    bits[H - 1, W - 1] = (0xFFC12345, 0x00000001, 0x7F7FFFFF) if H * W > 1 else bits[0, 0]
    occ = g.randint(0, 256, size=(H, W)).astype(np.uint8)
    f = 1.2 * max(H, W, 40)
    K = np.array([[f, 0, W / 2.0 + 0.3], [0, 1.01 * f, H / 2.0 - 0.7], [0, 0, 1]])
    from invr.scene import rodrigues
    R, T = rodrigues(np.array([0.1, -0.2, 0.05])), np.array([[0.1], [-0.05], [0.2]])
    centre = (np.linalg.inv(K) @ np.array([W / 2.0, H / 2.0, 1.0]) * 3.0 - T.ravel()) @ R          # a box the central rays meet, the outer ones miss
    half = 0.3 * max(H, W) * 3.0 / f + 0.05
    return img, occ, K, R, T, np.stack([centre - half, centre + half]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def classes_of(H, W, triple):
    """-> (coords: the three np.argwhere lists, planes, row_prefix) of a frame shape under a pattern triple.  Read-only."""
    coords = [np.argwhere(pattern(p, H, W)) for p in triple]
    return (coords,) + S.planes_and_prefix(coords, H, W)


def selection(coords, seed):
    """Rows (class, rank) over the three classes: every rank once for a small class, else rank 0, the last and random ones; some rows
    twice; all shuffled together."""
    g = np.random.RandomState(seed)
    rows = []
    for c, co in enumerate(coords):
        if len(co) == 0:
            continue
        ranks = np.arange(len(co)) if len(co) <= ALL_RANKS else np.concatenate([[0, len(co) - 1], g.randint(0, len(co), 300)])
        ranks = np.concatenate([ranks, ranks[g.randint(0, len(ranks), 1 + len(ranks) // 8)]])          # duplicates
        rows.append(np.stack([np.full(len(ranks), c), ranks], 1))
    rows = np.concatenate(rows)
    return np.ascontiguousarray(rows[g.permutation(len(rows))].astype(np.int32))


def run(H, W, planes, prefix, sel, fill):
    """One call over buffers of n + PAD rows pre-filled with the byte `fill` -> {key: ndarray of all n + PAD rows}."""
    img, occ, K, R, T, bounds = frame(H, W)
    n = len(sel)
    shape = {'ray_d': (n + PAD, 3), 'near': (n + PAD,), 'far': (n + PAD,), 'rgb': (n + PAD, 3), 'occupancy': (n + PAD,), 'coord': (n + PAD, 2)}
    dtype = {'occupancy': torch.uint8, 'coord': torch.int64}
    o = {}
    for k in KEYS:
        t = torch.empty(shape[k], dtype=dtype.get(k, torch.float32), device=DEV)
        t.view(torch.uint8).fill_(fill)
        o[k] = t
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    img_d, occ_d, planes_d, prefix_d, sel_d = up(img), up(occ), up(planes.view(np.int64)), up(prefix), up(sel)
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    cam_o = -np.dot(R.T, T).ravel()
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    _abi.check(_abi.lib().invr_ray_batch(
        _abi.ptr(img_d), _abi.ptr(occ_d, u8), _abi.ptr(planes_d, i64), _abi.ptr(prefix_d, i32), H, W, _abi.ptr(sel_d, i32), n,
        f64(np.linalg.inv(K)), f64(R), f64(T.ravel()), f64(cam_o), np.ascontiguousarray(bounds, np.float32).ctypes.data_as(C.POINTER(C.c_float)),
        _abi.ptr(o['ray_d']), _abi.ptr(o['near']), _abi.ptr(o['far']), _abi.ptr(o['rgb']), _abi.ptr(o['occupancy'], u8), _abi.ptr(o['coord'], i64),
        _abi.stream_ptr()))
    if DEV != 'cpu':
        torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in o.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def check(got, want, n, fill, tag):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, (tag, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(bits(got[k][:n]), bits(want[k])), (tag, k, np.flatnonzero((got[k][:n] != want[k]).reshape(n, -1).any(1))[:8])
        assert (bits(got[k][n:]) == fill).all(), (tag, k, 'a row at or past n was written')


def both_fills(H, W, coords, planes, prefix, sel, tag):
    img, occ, K, R, T, bounds = frame(H, W)
    want = S.ray_batch(img, occ, coords, sel, K, R, T, bounds)
    got = run(H, W, planes, prefix, sel, FILLS[0])
    check(got, want, len(sel), FILLS[0], tag)
    again = run(H, W, planes, prefix, sel, FILLS[1])                             # the same bits over differently dirtied buffers
    check(again, want, len(sel), FILLS[1], tag)
    return want


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_select_against_argwhere(shape):
    H, W = shape
    for triple in TRIPLES:
        coords, planes, prefix = classes_of(H, W, triple)
        sel = selection(coords, 7 * H + W)
        # the case is what it is there for
        for c, co in enumerate(coords):
            ranks = sel[sel[:, 0] == c, 1]
            assert len(co) == 0 or {0, len(co) - 1} <= set(ranks.tolist()), (shape, triple, c)
            assert len(co) > ALL_RANKS or set(ranks.tolist()) == set(range(len(co))), (shape, triple, c)          # onto: with S.ray_batch, a bijection
        assert len(np.unique(sel, axis=0)) < len(sel)                                                            # duplicates
        if triple[0] == 'words':
            assert len(coords[0]) == H * sum(x < W for x in (63, 64, 127, 128)) and (W != 130 or len(coords[0]) == 4 * H)
        want = both_fills(H, W, coords, planes, prefix, sel, (shape, triple))
        assert np.array_equal(want['coord'], np.stack([coords[c][r] for c, r in sel]))


@pytest.mark.parametrize('n', SIZES)
def test_batch_sizes(n):
    """n on both sides of a wave and of a workgroup, and several workgroups; the classes interleaved."""
    H, W = 97, 130
    coords, planes, prefix = classes_of(H, W, ('checker', 'gaps', 'full'))
    g = np.random.RandomState(n)
    cls = g.randint(0, 3, n)
    sel = np.stack([cls, [g.randint(0, len(coords[c])) for c in cls]], 1).astype(np.int32)
    sel[0] = (2, len(coords[2]) - 1)                                             # the frame's last pixel
    both_fills(H, W, coords, planes, prefix, sel, n)


def test_rgb_is_a_bit_copy_and_occupancy_the_byte():
    """-0.0, an inf, a denormal and NaN payloads of the frame's corner pixels arrive unchanged; occupancy is occ_msk's byte, not a flag."""
    H, W = 97, 300
    img, occ = frame(H, W)[:2]
    coords, planes, prefix = classes_of(H, W, TRIPLES[0])
    sel = np.array([[1, 0], [2, 0], [0, 0], [0, H * W - 1], [2, 0]], np.int32)
    got = run(H, W, planes, prefix, sel, FILLS[0])
    want = np.stack([img[0, 0], img[H - 1, W - 1], img[0, 0], img[H - 1, W - 1], img[H - 1, W - 1]])
    assert np.array_equal(bits(got['rgb'][:5]), bits(want))
    assert np.array_equal(got['occupancy'][:5], [occ[0, 0], occ[-1, -1], occ[0, 0], occ[-1, -1], occ[-1, -1]])
    assert np.array_equal(got['coord'][:5], [[0, 0], [H - 1, W - 1], [0, 0], [H - 1, W - 1], [H - 1, W - 1]])
    assert len(set(occ.ravel().tolist())) > 100


@pytest.mark.parametrize('name', [c['name'] for c in S.golden_cases()])
def test_ray_batch_against_the_reference_golden(name):
    """The rays the reference drew: coord and occupancy exact, rgb a bit copy, ray_d / near / far within the ulp bound the golden records
    (0: bit for bit)."""
    c = next(c for c in S.golden_cases() if c['name'] == name)
    coords = S.classes(c['msk'], c['bound'])
    rays_o, rays_d = S.frame_rays(c['H'], c['W'], c['K'], c['R'], c['T'])
    inside = S.near_far(c['wbounds'], rays_o, rays_d.reshape(-1, 3))[2].reshape(c['H'], c['W'])
    sel, rounds = S.draw_rays(coords, inside, c['N_rand'], c['body_ratio'], c['face_ratio'], np.random.RandomState(c['seed']))
    assert rounds == c['rounds']
    planes, prefix = S.planes_and_prefix(coords, c['H'], c['W'])
    n = len(sel)
    o = {k: torch.empty(s, dtype=d, device=DEV) for k, s, d in (('ray_d', (n, 3), torch.float32), ('near', (n,), torch.float32),
                                                               ('far', (n,), torch.float32), ('rgb', (n, 3), torch.float32),
                                                               ('occupancy', (n,), torch.uint8), ('coord', (n, 2), torch.int64))}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    keep = [up(c['img']), up(c['orig_msk']), up(planes.view(np.int64)), up(prefix), up(sel)]
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    _abi.check(_abi.lib().invr_ray_batch(
        _abi.ptr(keep[0]), _abi.ptr(keep[1], u8), _abi.ptr(keep[2], i64), _abi.ptr(keep[3], i32), c['H'], c['W'], _abi.ptr(keep[4], i32), n,
        f64(np.linalg.inv(c['K'])), f64(c['R']), f64(c['T'].ravel()), f64(rays_o), np.ascontiguousarray(c['wbounds'], np.float32).ctypes.data_as(C.POINTER(C.c_float)),
        _abi.ptr(o['ray_d']), _abi.ptr(o['near']), _abi.ptr(o['far']), _abi.ptr(o['rgb']), _abi.ptr(o['occupancy'], u8), _abi.ptr(o['coord'], i64),
        _abi.stream_ptr()))
    if DEV != 'cpu':
        torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in o.items()}
    assert np.array_equal(got['coord'], c['coord']) and np.array_equal(got['occupancy'], c['occupancy'])
    assert np.array_equal(bits(got['rgb']), bits(c['img'][c['coord'][:, 0], c['coord'][:, 1]]))
    bound = c['ulp'] + 1 if c['ulp'] else 0
    for k in ('ray_d', 'near', 'far'):
        assert S.ulp_distance(got[k], c[k]) <= bound, (name, k, S.ulp_distance(got[k], c[k]))
