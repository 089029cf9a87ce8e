"""GPU: the deformer's FORWARD, resd = 0.05 tanh(MLP(grid(uv(x), frame_dim))), in every form the library has it — element by element,
every element of every output, against the hand-written float64 reference of tests/deform_reference.py:

    |kernel - exact|  <=  8 noise  +  (c + 4) 2^-24 A  +  c 2^-126                  (tests/deform_cases.py: reference_fwd, accept)

noise = the largest of the fp32 oracle's deviation on the CPU, the move of `exact` under 4 ulp-sized perturbations of the point and its
move under the documented Softplus VALUE error; A = the absolute-value companion, c = 35; A == 0 requires exactly 0.0.  The rule, the
noise classes and the reference are those of the backward test (tests/test_gpu_deform_bwd.py), unchanged; nothing is fitted to a kernel
and no element is left out.  Each output prints K = max_e |kernel - exact| / (noise + 2^-23 A) for the kernel and for the fp32 oracle
(prefix DFF), each case one DFFCASE line (profiles/deform_fwd_headroom.md keeps them).

  A. scalar form, invr_deform_fwd -> k_deform_points (csrc/k_warp.hip; deform_fwd_act of csrc/deform_mlp.h): the clouds, the synthetic UV
     volume, the weight sets and the frames of tests/deform_cases.py; sizes around WARP_BLOCK = 128, the weight-set x cloud matrix, a
     grid whose slices do not fit, n = 0.
  B. invr_warp_deform -> k_warp_dense with a warp that is exact in fp32 (every joint matrix 2 I, one-hot blend weights: the blended
     matrix is 2 I, its determinant 8, 8 + 2^-23 rounds to 8, the inverse is 0.5 I): the canonical point IS the pose point, so resd is
     judged by the rule where the pair is flagged and is +0.0 where it is not, tpose = fl(pts + resd) and tdirs = pose_dirs bit for bit.
  C. pair form, k_deform_pairs through invr_geometry_fwd on the small scene of tests/test_gpu_warp_in_deformer.py (its world() /
     geometry() arrangement with the deformer's parameters, grid and frame_dim swapped): MFMA layers with the df_col weight order,
     log2-domain Softplus with the scales folded into the staged weights, per-frame slices in LDS.  l_r of ALL five lists, the
     far-constant pair included, at the canonical point fl(l_x - l_r) (l_x = fl(xb + r): the reconstructed point is within 2^-23 |x| of
     the kernel's own, and noise class (b) moves every point by (|x| + 1) 2^-23).  The three instantiations:
        <true, true>   slices + 24-bit UV index math : the production grid, every weight set x every frame
        <false, false> 3-D gathers                    : the `fallback` grid (its slices exceed DF_SLICE_MAX)
        <true, false>  slices + 64-bit UV index math : the UV volume zero-padded past 2^24 elements
     and two ray windows with a list count of 65 and of 255..257 (the last live lane of a partial batch).
  D. the per-frame slice table itself (InvrWsLayout.dslice): every entry against (1 - tz) row(cx, cy, c0z) + tz row(cx, cy, c1z).

Outputs are pre-filled (NaN, or the workspace's 0x7F bytes) and asserted bit-identical where nothing may be written.
tests/test_hostsim_deform_fwd_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_deform_bwd as B               # noqa: E402  (_dev_model, make_scene, product_spec, slices_fit)
import tests.test_gpu_warp_in_deformer as W         # noqa: E402  (geometry, per_ray_pairs, find_window, FRAME, S, FILL32)
from tests import deform_cases as DC                # noqa: E402  (checker only)
from tests import encoder_cases as EC               # noqa: E402  (checker only)
from tests import grid_reference as GR              # noqa: E402  (checker only)
from tests.mlp_reference import Ref                 # noqa: E402
from invr import _abi, params, scene as SC          # noqa: E402
from invr.config import make_cfg                    # noqa: E402
from invr.network import Network                    # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
PAD = 64                                            # rows behind n in every per-row output: they keep the pre-fill
_FR = ('t0', 'tmid', 't1')
SIZES = (1, 127, 128, 129, 257, 1000)               # WARP_BLOCK = 128: one thread, a block less one, a block, one more, two + 1, eight - 24
MATRIX = [(w, c, _FR[(i + j) % 3]) for i, w in enumerate(DC.WEIGHT_SETS) for j, c in enumerate(DC.CLOUDS)]
PAIR_CASES = [('prod', w, f) for w in DC.WEIGHT_SETS for f in _FR] + [('fallback', 'init', 'tmid'), ('fallback', 'wide', 't1')]


def set_device(dev):
    """One switch for this module and the two it borrows helpers from (the wave-machine twin) -> the device before."""
    global DEV
    old = DEV
    DEV = B.DEV = W.DEV = dev
    B._dev_model.cache_clear()
    W._CACHE.clear()
    _pair_net.cache_clear()
    return old


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def nan_filled(*shape):
    return torch.full(shape, NAN).to(DEV)


def assert_keeps_nan(t, what):
    assert (t.contiguous().view(torch.int32) == torch.full((1,), NAN).view(torch.int32)).all(), '%s: written at or past n' % what


def cut(ref, sel):
    return Ref(ref.exact[sel], ref.A[sel], ref.c)


class Judge:
    """Every output through the rule (all of them, so that every K line is printed), then the failures together and the case's line."""

    def __init__(self, cid):
        self.cid, self.failures, self.K, self.K32 = cid, [], 0.0, 0.0

    def one(self, name, val, ref, noise, o32):
        self.K32 = max(self.K32, EC.headroom(o32, ref, noise))
        self.K = max(self.K, EC.headroom(val, ref, noise) if not torch.isnan(val).any() else float('inf'))
        try:
            DC.accept(self.cid, name, val, ref, noise, o32, prefix='DFF')
        except AssertionError as e:
            self.failures.append(str(e))

    def done(self):
        print('DFFCASE %-52s K_kernel %.3g K_oracle32 %.3g' % (self.cid, self.K, self.K32))
        assert not self.failures, '\n'.join(self.failures)


@functools.lru_cache(maxsize=None)
def _reference(tag, wtag, cloud, frame, n):
    """-> (Ref, noise, o32) of resd on the first n rows of a cloud: computed once, shared by parts A and B, never modified."""
    if tag == 'prod':
        DC.check_params(wtag, DC.N_BASE)
    (_, ref, noise, o32, _), = DC.reference_fwd(DC.make_cloud(cloud, n, tag, frame), DC.make_params(wtag, tag), DC.make_scene(tag, frame),
                                                DC.make_spec(tag))
    return ref, noise, o32


# ---- A. invr_deform_fwd -> k_deform_points -------------------------------------------------------------------------------------------
def run_points(tag, wtag, frame, pts):
    """-> (status, resd (n,3) on the CPU); the PAD rows behind n asserted untouched (their input rows are NaN)."""
    n = pts.shape[0]
    model, _ = B._dev_model(tag, wtag, DEV)
    keep = []
    scene = B.make_scene(tag, frame, keep)
    x = torch.full((n + PAD, 3), NAN)
    x[:n] = pts
    x, out = x.to(DEV), nan_filled(n + PAD, 3)
    st = _abi.lib().invr_deform_fwd(C.byref(scene), C.byref(model), _abi.ptr(x), n, _abi.ptr(out), _abi.stream_ptr())
    sync()
    out = out.cpu()
    assert_keeps_nan(out[n:], 'resd')
    return st, out[:n]


def points_case(tag, wtag, cloud, frame, n):
    st, resd = run_points(tag, wtag, frame, DC.make_cloud(cloud, n, tag, frame))
    assert st == 0 and resd.shape == (n, 3)
    ref, noise, o32 = _reference(tag, wtag, cloud, frame, n)
    J = Judge('points-%s-%s-%s-%s-%d' % (tag, wtag, cloud, frame, n))
    J.one('resd', resd, ref, noise, o32)
    J.done()
    assert (resd.abs() <= torch.tensor(0.05)).all()


def test_cases_reach_the_intended_kernels():
    """The grids: the production deformer grid fits the slice table, `fallback` does not (and is the grid of the config the pair cases
    build); the padded UV volume of the 64-bit case is on the other side of 2^24 elements than the scene's own; WARP_BLOCK is 128."""
    assert B.slices_fit(B.product_spec('prod')) and sum(r * r for r in B.product_spec('prod')['res']) == 2959
    assert not B.slices_fit(B.product_spec('fallback'))
    for tag in ('prod', 'fallback'):
        p, o = params.deformer_grid_spec(_pair_cfg(tag)), B.product_spec(tag)
        for k in ('L', 'F', 'T', 'res', 'start_hash', 'separate_dense', 'dense_rows', 'sum', 'include_input', 'out_dim'):
            assert p[k] == o[k], (tag, k)
        assert torch.equal(torch.from_numpy(p['size']), torch.from_numpy(o['size'])) and p['bbox'].tolist() == DC.BBOX, tag
    small, big = _scene_np(False), _scene_np(True)
    assert small['tuv'].size <= 1 << 24 < big['tuv'].size
    text = open(os.path.join(_abi.HERE, 'csrc', 'k_warp.hip')).read()
    assert int(re.search(r'#define WARP_BLOCK (\d+)', text).group(1)) == 128


@pytest.mark.parametrize('n', SIZES)
def test_deform_fwd_sizes(n):
    points_case('prod', 'init', 'inside', _FR[SIZES.index(n) % 3], n)


@pytest.mark.parametrize('wtag,cloud,frame', MATRIX, ids=['%s-%s-%s' % c for c in MATRIX])
def test_deform_fwd_matrix(wtag, cloud, frame):
    points_case('prod', wtag, cloud, frame, 1000)


@pytest.mark.parametrize('wtag,cloud,frame', [('init', 'nodes', 't1'), ('wide', 'inside', 'tmid')])
def test_deform_fwd_generic_grid(wtag, cloud, frame):
    """The `fallback` grid (res 4 .. 68): the scalar form reads the 3-D tables whatever the grid, the same entry point must hold."""
    assert not B.slices_fit(B.product_spec('fallback'))
    points_case('fallback', wtag, cloud, frame, 1000)


def test_deform_fwd_count_zero():
    """n = 0: status 0 and nothing written (run_points: every row keeps the NaN pre-fill)."""
    st, resd = run_points('prod', 'init', 'tmid', torch.zeros(0, 3))
    assert st == 0 and resd.shape == (0, 3)


# ---- B. invr_warp_deform -> k_warp_dense with an exact warp ---------------------------------------------------------------------------
def run_warp(tag, wtag, frame, pts, dirs, bw, flag):
    """-> (tpose, tdirs, resd) (n,5,3) on the CPU; the PAD rows behind n asserted untouched."""
    n, NP = pts.shape[0], _abi.NUM_PARTS
    model, _ = B._dev_model(tag, wtag, DEV)
    keep = []
    scene = B.make_scene(tag, frame, keep)
    A = torch.diag(torch.tensor([2.0, 2.0, 2.0, 1.0])).expand(24, 4, 4).contiguous().to(DEV)
    scene.A = scene.big_A = A.data_ptr()
    ins = [t.to(DEV).contiguous() for t in (pts, dirs, bw)]
    fl = flag.to(DEV).contiguous()
    outs = [nan_filled(n + PAD, NP, 3) for _ in range(3)]
    _abi.check(_abi.lib().invr_warp_deform(C.byref(scene), C.byref(model), _abi.ptr(ins[0]), _abi.ptr(ins[1]), _abi.ptr(ins[2]),
                                           _abi.ptr(fl, torch.uint8), n, _abi.ptr(outs[0]), _abi.ptr(outs[1]), _abi.ptr(outs[2]),
                                           _abi.stream_ptr()))
    sync()
    res = []
    for name, t in zip(('tpose', 'tdirs', 'resd'), outs):
        t = t.cpu()
        assert_keeps_nan(t[n:], name)
        res.append(t[:n])
    return res


@pytest.mark.parametrize('wtag,cloud,frame', [('wide', 'inside', 'tmid'), ('saturated-head', 'nodes', 't1')])
def test_warp_deform_with_an_exact_warp(wtag, cloud, frame):
    n, NP = 1000, _abi.NUM_PARTS
    pts = DC.make_cloud(cloud, n, 'prod', frame)
    g = torch.Generator().manual_seed(23)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    assert (dirs != 0).all()
    joint = torch.randint(0, 24, (n, NP), generator=g)
    bw = torch.nn.functional.one_hot(joint, 24).float()
    flag = (torch.rand(n, NP, generator=g) < 0.6).to(torch.uint8)
    assert 0.5 < float(flag.float().mean()) < 0.7 and len(set(joint.reshape(-1).tolist())) == 24
    for p in range(NP):
        assert 0 < int(flag[:, p].sum()) < n                     # every part column with both values
    tpose, tdirs, resd = run_warp('prod', wtag, frame, pts, dirs, bw, flag)
    ref, noise, o32 = _reference('prod', wtag, cloud, frame, n)
    J = Judge('warp-prod-%s-%s-%s-%d' % (wtag, cloud, frame, n))
    for p in range(NP):
        on = flag[:, p] == 1
        J.one('resd[%d]' % p, resd[on, p], cut(ref, on), noise[on], o32[on])
        assert (resd[~on, p].contiguous().view(torch.int32) == 0).all(), 'part %d: resd of an unflagged pair is not +0.0' % p
    J.done()
    assert (resd.abs() <= torch.tensor(0.05)).all()
    want = pts[:, None, :] + resd                                 # the canonical point is the pose point bit for bit
    assert torch.equal(tpose.view(torch.int32), want.view(torch.int32)), int((tpose.view(torch.int32) != want.view(torch.int32)).sum())
    assert torch.equal(tdirs.view(torch.int32), dirs[:, None, :].expand(n, NP, 3).contiguous().view(torch.int32))


# ---- C. k_deform_pairs through invr_geometry_fwd ----------------------------------------------------------------------------------------
def _pair_cfg(tag):
    kw = {} if tag == 'prod' else dict(tpose_deformer={'embedder': {'kwargs': dict(DC.SPECS[tag], use_batch_bounds=False)}})
    return make_cfg(table_log2=12, N_samples=W.S, **kw)


@functools.lru_cache(maxsize=2)
def _scene_np(big):
    """The frame of tests/test_gpu_warp_in_deformer.py; big: its UV volume zero-padded past 2^24 elements, the bounds extended by whole
    voxels (the arithmetic of tests/test_gpu_big_volume.py)."""
    bnp, _ = SC.make_scene(**W.FRAME)
    if not big:
        return bnp
    vol, b = np.asarray(bnp['tuv'])[0], np.asarray(bnp['tbounds'], np.float64).reshape(2, 3)
    dx, dy, dz, c = vol.shape
    assert c == 2 and vol.size <= 1 << 24
    fx = int(np.ceil(np.sqrt((1 << 24) * 1.05 / vol.size))) + 1
    nx, ny = dx * fx, dy * fx
    pad = np.zeros((nx, ny, dz, c), np.float32)
    pad[:dx, :dy] = vol
    nb = b.copy()
    nb[1, 0] = b[0, 0] + (b[1, 0] - b[0, 0]) * (nx - 1) / (dx - 1)
    nb[1, 1] = b[0, 1] + (b[1, 1] - b[0, 1]) * (ny - 1) / (dy - 1)
    out = dict(bnp)
    out['tuv'], out['tbounds'] = pad[None], nb.astype(np.float32).reshape(np.asarray(bnp['tbounds']).shape)
    return out


def pair_params(tag, wtag):
    """The weight sets as DC.make_params scales them on its own base batch: on the points these lists hold they reach the ranges
    judge_lists asserts without a rescaling of their own (profiles/deform_fwd_headroom.md has the ranges)."""
    return DC.make_params(wtag, tag)


@functools.lru_cache(maxsize=2)
def _pair_net(tag, dev):
    """One network per grid (its derived eval tables are built once); pair_world loads a weight set into its deformer in place."""
    cfg = _pair_cfg(tag)
    sd = params.init_state_dict(cfg, seed=3)
    assert sd['tpose_deformer.embedder.bounds'].tolist() == DC.BBOX
    net = Network(cfg=cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval()


def load_deformer(net, P):
    """DC's parameters, tables included, into the network's deformer: the tensors the C-ABI model points at, written in place."""
    new = {'tpose_deformer.embedder.dense': P['dense'], 'tpose_deformer.embedder.hash': P['hash']}
    for i, k in enumerate((0, 2, 4)):
        new['tpose_deformer.mlp.%d.weight' % k], new['tpose_deformer.mlp.%d.bias' % k] = P['W'][i], P['b'][i]
    have = dict(net.named_parameters())
    for k, t in new.items():
        assert tuple(have[k].shape) == tuple(t.shape) and have[k].dtype == torch.float32, k
        with torch.no_grad():
            have[k].copy_(t.to(have[k].device))
    assert {k for k in have if k.startswith('tpose_deformer.mlp.') or k.endswith(('tpose_deformer.embedder.dense', 'tpose_deformer.embedder.hash'))} == set(new)


def pair_world(tag, wtag, frame, big=False):
    """-> (net, ctx, rays, reference scene dict): W.world() with the deformer's parameters, grid, frame_dim (and UV volume) swapped."""
    bnp = dict(_scene_np(big))
    bnp['frame_dim'] = np.full_like(np.asarray(bnp['frame_dim']), DC.FRAMES[frame])
    net = _pair_net(tag, DEV)
    load_deformer(net, pair_params(tag, wtag))
    gb = {k: v.to(DEV) for k, v in SC.to_torch(bnp).items()}
    ctx = net.prepare(gb)
    ref_scene = dict(tuv=torch.from_numpy(np.ascontiguousarray(bnp['tuv'][0])), tbounds=torch.from_numpy(np.asarray(bnp['tbounds'])).reshape(2, 3).clone(),
                     frame_dim=torch.tensor(DC.FRAMES[frame], dtype=torch.float32))
    assert gb['frame_dim'].dtype == torch.float32 and torch.equal(gb['frame_dim'].reshape(-1)[:1].cpu(), ref_scene['frame_dim'].reshape(1))
    return net, ctx, tuple(gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far')), ref_scene


def read_lists(st, v):
    """-> (counts, [l_x (c,3)], [l_r (c,3)]) on the CPU, every list up to its count (the far-constant pair included); everything past the
    counts of l_x / l_d / l_r asserted to hold the fill."""
    counts = [int(st[1 + p]) for p in range(_abi.NUM_PARTS)]
    lx, lr = [], []
    for p, c in enumerate(counts):
        assert 1 <= c <= v['lcap']
        for k in ('l_x', 'l_d', 'l_r'):
            tail = v[k][p].view(torch.int32)[:, c:]
            assert tail.shape[1] == v['lcap'] - c and bool((tail == W.FILL32).all()), (k, p, c)
        lx.append(v['l_x'][p][:, :c].t().contiguous().cpu())
        lr.append(v['l_r'][p][:, :c].t().contiguous().cpu())
    return counts, lx, lr


def judge_lists(cid, tag, wtag, ref_scene, counts, lx, lr, whole):
    """The conditions from the scene and the float64 reference alone, then every l_r entry of the five lists through the rule."""
    r_all = torch.cat(lr, 0)
    pts = (torch.cat(lx, 0).double() - r_all.double()).float()          # the canonical point, reconstructed (module docstring)
    chunks = DC.reference_fwd(pts, pair_params(tag, wtag), ref_scene, DC.make_spec(tag))
    z = {k: torch.cat([c[4][k] for c in chunks], 0) for k in ('z1', 'z2', 'z3')}
    rng = {k: (float(t.min()), float(t.max())) for k, t in z.items()}
    print('DFFPAIRS %-40s counts %s  z1 %.3g .. %.3g  z2 %.3g .. %.3g  z3 %.3g .. %.3g' % ((cid, counts) + rng['z1'] + rng['z2'] + rng['z3']))
    if whole:
        assert sum(counts) >= 4096 and max(counts) > 1024, counts
        if wtag in ('wide', 'saturated-head'):
            for k in ('z1', 'z2'):
                assert rng[k][0] <= -9.0 and rng[k][1] >= 9.0, (k, rng[k])
        if wtag == 'saturated-head':
            assert float(z['z3'].abs().max()) >= 6.0, rng['z3']
    ref = Ref(torch.cat([c[1].exact for c in chunks], 0), torch.cat([c[1].A for c in chunks], 0), chunks[0][1].c)
    noise, o32 = torch.cat([c[2] for c in chunks], 0), torch.cat([c[3] for c in chunks], 0)
    J = Judge(cid)
    lo = 0
    for p, c in enumerate(counts):
        sl = slice(lo, lo + c)
        J.one('l_r[%d]' % p, lr[p], cut(ref, sl), noise[sl], o32[sl])
        lo += c
    J.done()
    assert (r_all.abs() <= torch.tensor(0.05)).all()                   # |0.05f tanhf| <= 0.05f exactly


def pairs_case(tag, wtag, frame, big=False, window=None):
    net, ctx, rays, ref_scene = pair_world(tag, wtag, frame, big)
    if window is not None:
        rays = tuple(r[window[0]:window[1]] for r in rays)
    st, v = W.geometry(net, ctx, rays)
    counts, lx, lr = read_lists(st, v)
    cid = 'pairs-%s-%s-%s%s%s' % (tag, wtag, frame, '-bigvol' if big else '', '-rays%d..%d' % window if window else '')
    judge_lists(cid, tag, wtag, ref_scene, counts, lx, lr, whole=window is None)
    return counts


@pytest.mark.parametrize('tag,wtag,frame', PAIR_CASES, ids=['%s-%s-%s' % c for c in PAIR_CASES])
def test_pair_deformer(tag, wtag, frame):
    """prod: k_deform_pairs<true, true> (the slices fit, the scene's UV volume holds at most 2^24 elements); fallback:
    k_deform_pairs<false, false> (launch_warp_pairs: the slices do not fit)."""
    assert B.slices_fit(params.deformer_grid_spec(_pair_cfg(tag))) == (tag == 'prod')
    assert _scene_np(False)['tuv'].size <= 1 << 24
    pairs_case(tag, wtag, frame)


def test_pair_deformer_big_volume():
    """k_deform_pairs<true, false>: the slices fit and the UV volume holds more than 2^24 elements (volume_is_small, csrc/common.h)."""
    assert B.slices_fit(params.deformer_grid_spec(_pair_cfg('prod')))
    assert _scene_np(False)['tuv'].size <= 1 << 24 < _scene_np(True)['tuv'].size
    pairs_case('prod', 'wide', 'tmid', big=True)


def test_pair_deformer_boundary_counts():
    """Two of the ray windows of test_boundary_counts_values_and_fill — some part's list count is 65 (one lane into a wave's second
    batch), some part's in 255..257 (the workgroup's edge): the last live lane of a partial batch goes through the rule."""
    net, ctx, rays, _ = pair_world('prod', 'wide', 'tmid')
    st, v = W.geometry(net, ctx, rays)
    per_ray = W.per_ray_pairs(st, v, rays[0].shape[0])
    for lo, hi in ((65, 65), (255, 257)):
        win = W.find_window(per_ray, lo, hi)
        assert win is not None, (lo, hi)
        counts = pairs_case('prod', 'wide', 'tmid', window=win)
        assert any(lo <= c <= hi for c in counts), (lo, hi, counts)


# ---- D. the per-frame slice table -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _slice_levels(frame, dev):
    """One geometry pass of the production grid at `frame` -> per level (res, c0z, c1z, tz, f, err, A, S) with err = |table - exact| of the
    level's res^2 x 2 values, exact = (1 - tz) row(cx, cy, c0z) + tz row(cx, cy, c1z) in float64 from the level geometry of
    tests/grid_reference.py, A = (1 - tz) |v0| + tz |v1|, S = |v0| + |v1|, f = the level's float64 quotient t_n / cell = c0z + tz.
    Entries at and past off[8] = 2959 asserted to keep the workspace's fill."""
    net, ctx, rays, ref_scene = pair_world('prod', 'init', frame)
    st, v = W.geometry(net, ctx, tuple(r[::8].contiguous() for r in rays))
    got = v['dslice'].cpu()
    assert tuple(got.shape) == (_abi.DF_SLICE_MAX, 2)
    spec, P = DC.make_spec('prod'), DC.make_params('init', 'prod')
    tab = GR.flat_table(P['dense'], P['hash'], spec)
    xn0 = GR.normalise(torch.cat([torch.zeros(1, 2), ref_scene['frame_dim'].reshape(1, 1)], 1), spec['bbox'])
    off, levels = 0, []
    for l in range(spec['L']):
        res = int(spec['res'][l])
        c0, c1, t = GR.level_cells(xn0, spec, l)
        c0z, c1z, tz = int(c0[0, 2]), int(c1[0, 2]), float(t[0, 2])
        cx, cy = torch.meshgrid(torch.arange(res), torch.arange(res), indexing='ij')
        cell = torch.stack([cx.reshape(-1), cy.reshape(-1)], 1)
        lo = torch.cat([cell, torch.full((res * res, 1), c0z)], 1)
        hi = torch.cat([cell, torch.full((res * res, 1), c1z)], 1)
        rows = GR.level_rows(lo, hi, spec, l)                      # corner k = x y z bits: 0 = (cx, cy, c0z), 1 = (cx, cy, c1z)
        v0, v1 = tab[rows[0]], tab[rows[1]]
        exact = (1.0 - tz) * v0 + tz * v1
        err = (got[off:off + res * res].double() - exact).abs()
        levels.append((res, c0z, c1z, tz, c0z + tz, err, abs(1.0 - tz) * v0.abs() + abs(tz) * v1.abs(), v0.abs() + v1.abs()))
        off += res * res
    assert off == 2959
    assert (got[off:].contiguous().view(torch.int32) == W.FILL32).all(), 'the slice table is written past off[8]'
    return levels


@pytest.mark.parametrize('frame', _FR)
def test_slice_table(frame):
    """deform_slice_body (csrc/front_bodies.h) through Workspace::dslice: every entry within 4 2^-24 A + 2^-126 of the float64 value,
    A = (1 - tz) |v0| + tz |v1| — one rounded tz, 1 - tz, a product and an fma.  Every level is printed, then the failures together.

    The bound needs tz to be the exact offset rounded once, and deform_slice_body forms it so: the quotient t_n / cell in double.  With
    level_corners' fp32 quotient (f off by 2^-24 f absolute, inherited whole by tz = f - c0z) the same table missed this bound by up to
    20.5 x at tmid (level 5: f = 7.03, tz = 0.03) and 9.1e4 x at t1, where 1 / cell of the fp32 cell size lies just below res - 1 and
    fp32 rounds it onto the last cell: absolute errors of 1.35e-7 and 4.96e-7 on table values of about 0.1."""
    failures = []
    for l, (res, c0z, c1z, tz, f, err, A, S) in enumerate(_slice_levels(frame, DEV)):
        allow = 4.0 * 2.0 ** -24 * A + 2.0 ** -126
        k = float((err / allow).max())
        print('DFFSLICE %-4s level %d res %2d c0z %2d c1z %2d tz %.9g: max err %.3g, max err / allowed %.3g' % (frame, l, res, c0z, c1z, tz, float(err.max()), k))
        bad = err > allow
        if bad.any():
            failures.append('level %d: %d of %d slice values outside 4 2^-24 A + 2^-126 (worst %.3g x allowed)' % (l, int(bad.sum()), bad.numel(), k))
    assert not failures, '\n'.join(failures)
