"""GPU: the deformer's backward chain — k_deform_bwd, k_wgrad with the deformer's three jobs (csrc/k_train.hip) and k_deform_slice_bwd
(csrc/k_warp.hip), or the generic k_grid_encode_bwd_rt where the slices do not fit — called alone through the C-ABI
(invr_deform_bwd_list: the very launch code invr_train_bwd runs after it has built its list) against the hand-written float64
reference of tests/deform_reference.py — element by element, every element of every output:

    |kernel - exact|  <=  8 noise  +  (c + 4) 2^-24 A  +  c 2^-126                      (tests/deform_cases.py: reference, accept)

noise = the largest of the fp32 autograd's deviation on the CPU, the move of `exact` under 4 ulp-sized input perturbations and its
move under the documented Softplus VALUE error (1 ulp / 1.5e-7); A = the absolute-value companion, c = the number of summands;
A == 0 requires exactly 0.0.  Nothing is fitted to the kernels.  Each case prints K = max_e |kernel - exact| / (noise + 2^-23 A) for
the kernel and for the fp32 oracle, per output and (DFBCASE) per case (profiles/deform_bwd_headroom.md keeps them).

Why element by element: the training tests hold the tpose_deformer.* gradients to 5e-3 of each tensor's maximum.  A dropped a0 pad, a
wrong column of the 20-padded W0, a lost 4-row tail in k_wgrad or swapped (1 - tz, tz) weights change a few elements by a few per
cent of THOSE elements and nothing relative to the tensor's maximum.

Every per-entry output is pre-filled with NaN (asserted bit-identical at and past `count` afterwards); the gradient tensors are
zeroed or pre-loaded with non-zeros (they accumulate).  tests/test_hostsim_deform_bwd_cpu.py runs the same bodies on the CPU wave
machine."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import deform_cases as DC        # noqa: E402  (checker only)
from tests import deform_reference as DR    # noqa: E402  (checker only)
from tests import encoder_cases as EC       # noqa: E402  (checker only)
from invr import _abi, params               # noqa: E402
from invr.config import make_cfg            # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
WIDTHS = dict(uvt=3, gfeat=19, gz1=32, gz2=32, gz3=4, a0=20, a1=32, a2=32)          # csrc/train.h: the rows k_deform_bwd writes
PARAM_SHAPES = dict(dW0=(32, 19), db0=(32,), dW1=(32, 32), db1=(32,), dW2=(3, 32), db2=(3,))

# workgroup, slab and k-step edges of the three kernels: k_deform_bwd 256 entries per workgroup, k_wgrad 4-row MFMA k-steps in 256-row
# slabs (4 per workgroup), k_deform_slice_bwd 1024 entries per workgroup
SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)
LOOPS = {'wgrad': 48 * 4 * 256 + 300,           # k_wgrad's persistent grid (48 workgroups x 4 waves x 256 rows): a second slab for two waves
         'slice': 256 * 1024 + 1000,            # k_deform_slice_bwd's (256 workgroups x 1024 entries): a second pass for workgroup 0
         'deform': 2048 * 256 + 517}            # k_deform_bwd's (2048 workgroups x 256 entries)
_FR = ('t0', 'tmid', 't1')
MATRIX = [(w, c, _FR[(i + j) % 3], DC.PATTERNS[(i + j) % 2]) for i, w in enumerate(DC.WEIGHT_SETS) for j, c in enumerate(DC.CLOUDS)]


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def product_spec(tag):
    if tag == 'prod':
        return params.deformer_grid_spec(make_cfg())
    return params.grid_spec(bbox=DC.BBOX, **DC.SPECS[tag])


def slices_fit(spec):
    """csrc/front_bodies.h deform_slices_fit, restated: 8 levels whose (u, v) slices hold at most DF_SLICE_MAX float2 entries."""
    text = open(os.path.join(_abi.HERE, 'csrc', 'pipeline.h')).read()
    slice_max = int(re.search(r'#define DF_SLICE_MAX (\d+)', text).group(1))
    return spec['L'] == 8 and sum(r * r for r in spec['res']) <= slice_max


def test_specs_reach_the_intended_kernels():
    """The production deformer grid takes k_deform_slice_bwd; the `fallback` grid is refused by launch_deform_slice_bwd (its slices do
    not fit) and goes to the generic backward; both agree with the oracle's restatement of the constructor arithmetic."""
    for tag in ('prod', 'fallback'):
        p, o = product_spec(tag), DC.make_spec(tag)
        for k in ('L', 'F', 'T', 'res', 'start_hash', 'separate_dense', 'dense_rows', 'sum', 'sum_over_features', 'include_input', 'out_dim'):
            assert p[k] == o[k], (tag, k)
        assert torch.equal(torch.from_numpy(p['size']), o['size']) and p['bbox'].tolist() == DC.BBOX, tag
        assert (p['L'], p['F'], p['sum'], p['include_input'], p['out_dim']) == (8, 2, False, True, 19), tag
    assert slices_fit(product_spec('prod')) and sum(r * r for r in product_spec('prod')['res']) == 2959
    assert not slices_fit(product_spec('fallback'))
    assert LOOPS['wgrad'] > 49152 and LOOPS['slice'] > 262144 and LOOPS['deform'] > 524288


@functools.lru_cache(maxsize=4)
def _dev_model(tag, wtag, dev):
    P = DC.make_params(wtag, tag)
    keep = []
    m = _abi.InvrModel()
    bounds = torch.tensor(DC.BBOX, dtype=torch.float32).to(dev)
    m.deform_grid = _abi.make_grid(product_spec(tag), P['dense'].to(dev), P['hash'].to(dev), bounds, keep)
    m.deform_mlp = _abi.make_mlp([w.to(dev) for w in P['W']], [b.to(dev) for b in P['b']], keep)
    return m, keep


def make_scene(tag, frame, keep):
    sc = DC.make_scene(tag, frame)
    s = _abi.InvrScene()
    tuv, tb, fd = sc['tuv'].to(DEV).contiguous(), sc['tbounds'].to(DEV).contiguous(), sc['frame_dim'].reshape(1).to(DEV).contiguous()
    keep += [tuv, tb, fd]
    s.tuv, s.tbounds, s.frame_dim = tuv.data_ptr(), tb.data_ptr(), fd.data_ptr()
    for a in range(3):
        s.tuv_dims[a] = tuv.shape[a]
    return s


def run_list(tag, wtag, frame, pts, g_resd, n_max=None, pre=None):
    """One call of invr_deform_bwd_list on the first `count` = len(pts) entries of lists of n_max rows (rows at and past count: NaN
    inputs).  pre: name -> pre-loaded value of a gradient tensor (default zeros).  -> dict of CPU tensors, the per-entry matrices cut to
    `count` rows and to the reference's widths; every must-not-touch region and every pad column already asserted."""
    count = pts.shape[0]
    n_max = count if n_max is None else n_max
    assert count <= n_max
    P = DC.make_params(wtag, tag)
    model, _ = _dev_model(tag, wtag, DEV)
    keep = []
    scene = make_scene(tag, frame, keep)
    x, g = torch.full((n_max, 3), NAN), torch.full((n_max, 3), NAN)
    x[:count], g[:count] = pts, g_resd
    x, g = x.to(DEV), g.to(DEV)
    ent = {k: torch.full((n_max, w), NAN).to(DEV) for k, w in WIDTHS.items()}
    out = _abi.InvrDeformBwdOut()
    for k in WIDTHS:
        setattr(out, k, ent[k].data_ptr())
    shapes = dict(PARAM_SHAPES, g_dense=tuple(P['dense'].shape), g_hash=tuple(P['hash'].shape))
    grads = {k: (torch.zeros(s) if pre is None else pre[k].clone()).to(DEV) for k, s in shapes.items()}
    dW = (C.c_void_p * 3)(*[grads['dW%d' % l].data_ptr() for l in range(3)])
    db = (C.c_void_p * 3)(*[grads['db%d' % l].data_ptr() for l in range(3)])
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    _abi.check(_abi.lib().invr_deform_bwd_list(C.byref(scene), C.byref(model), _abi.ptr(x), _abi.ptr(g), n_max, _abi.ptr(cnt, torch.int32),
                                               C.byref(out), dW, db, _abi.ptr(grads['g_dense']), _abi.ptr(grads['g_hash']), _abi.stream_ptr()))
    sync()
    res = {k: v.cpu() for k, v in grads.items()}
    nan_bits = torch.full((1,), NAN).view(torch.int32)
    for k, v in ent.items():
        v = v.cpu()
        assert (v[count:].contiguous().view(torch.int32) == nan_bits).all(), '%s: written at or past count' % k
        res[k] = v[:count]
    # the pad columns and the constant coordinate
    assert (res['a0'][:, 19] == 0).all() and (res['gz3'][:, 3] == 0).all(), 'a pad column is not 0'
    fd = DC.make_scene(tag, frame)['frame_dim'].reshape(1)
    assert (res['uvt'][:, 2].contiguous().view(torch.int32) == fd.view(torch.int32)).all(), 'uvt[:, 2] is not frame_dim'
    res['a0'], res['gz3'] = res['a0'][:, :19].contiguous(), res['gz3'][:, :3].contiguous()
    return res


@functools.lru_cache(maxsize=2)
def _reference(tag, wtag, cloud, frame, pattern, n):
    return DC.reference(DC.make_cloud(cloud, n, tag, frame), DC.make_gresd(n, pattern), DC.make_params(wtag, tag), DC.make_scene(tag, frame),
                        DC.make_spec(tag))


class Judge:
    """Every output through the rule (all of them, so that every K line is printed), then the failures together and the case's line."""

    def __init__(self, cid):
        self.cid, self.failures, self.K, self.K32 = cid, [], 0.0, 0.0

    def one(self, name, val, ref, noise, o32, touched=None):
        self.K32 = max(self.K32, EC.headroom(o32, ref, noise))
        self.K = max(self.K, EC.headroom(val, ref, noise) if not torch.isnan(val).any() else float('inf'))
        try:
            DC.accept(self.cid, name, val, ref, noise, o32, touched)
        except AssertionError as e:
            self.failures.append(str(e))

    def entries(self, res, sl, ref, noise, o32):
        for k in DR.ENTRY_KEYS:
            self.one(k, res[k][sl], ref[k], noise[k], o32[k])

    def params(self, res, par, cloud, pre=None):
        ref, noise, o32, touched = par
        for k in DR.PARAM_KEYS:
            r, o = ref[k], o32[k]
            if pre is not None:
                r, o = DC.preloaded(r, pre[k]), o.double() + pre[k].double()
            self.one(k, res[k], r, noise[k], o, touched.get(k) if cloud == 'faces' and pre is None else None)

    def done(self):
        print('DFBCASE %-52s K_kernel %.3g K_oracle32 %.3g' % (self.cid, self.K, self.K32))
        assert not self.failures, '\n'.join(self.failures)


def run_case(tag, wtag, cloud, frame, pattern, n, n_max=None, preload=False):
    if n <= DC.N_BASE and tag == 'prod':
        DC.check_params(wtag, DC.N_BASE)
    pts, g = DC.make_cloud(cloud, n, tag, frame), DC.make_gresd(n, pattern)
    pre = None
    if preload:
        gen = torch.Generator().manual_seed(17)
        P = DC.make_params(wtag, tag)
        shapes = dict(PARAM_SHAPES, g_dense=tuple(P['dense'].shape), g_hash=tuple(P['hash'].shape))
        pre = {k: torch.randn(s, generator=gen) * 0.1 for k, s in shapes.items()}
    res = run_list(tag, wtag, frame, pts, g, n_max=n_max, pre=pre)
    for k in ('uvt', 'a0', 'a1', 'a2', 'gz1', 'gz2', 'gz3', 'gfeat'):
        assert res[k].shape[0] == n
    J = Judge('%s-%s-%s-%s-%s-%d%s' % (tag, wtag, cloud, frame, pattern, n, ('-of-%d' % n_max if n_max else '') + ('-preloaded' if preload else '')))
    if n <= DC.N_BASE:
        entries, par = _reference(tag, wtag, cloud, frame, pattern, n)
        for sl, ref, noise, o32 in entries:
            J.entries(res, sl, ref, noise, o32)
    else:                                                        # the persistent loops: judged chunk by chunk, nothing kept
        _, par = DC.reference(pts, g, DC.make_params(wtag, tag), DC.make_scene(tag, frame), DC.make_spec(tag),
                              on_chunk=lambda sl, ref, noise, o32: J.entries(res, sl, ref, noise, o32))
    J.params(res, par, cloud, pre)
    J.done()
    if pattern == 'sparse':                                      # the rows without an upstream gradient: every gradient row exactly +-0.0
        zero = ~g.any(1)
        assert zero.any() or n < 8
        for k in ('gz1', 'gz2', 'gz3', 'gfeat'):
            assert not res[k][zero].any(), k
    return res


@pytest.mark.parametrize('n', SIZES)
def test_deform_bwd_sizes(n):
    run_case('prod', 'init', 'inside', _FR[n % 3], 'dense', n)


@pytest.mark.parametrize('wtag,cloud,frame,pattern', MATRIX, ids=['%s-%s-%s-%s' % c for c in MATRIX])
def test_deform_bwd_matrix(wtag, cloud, frame, pattern):
    run_case('prod', wtag, cloud, frame, pattern, 1000)


@pytest.mark.parametrize('frame', _FR)
def test_deform_bwd_one_cloud_every_frame_sparse(frame):
    """All entries on the same LDS and table rows, at t = 0 / interior / 1 (t = 1: both z weights add into one row)."""
    run_case('prod', 'wide', 'one', frame, 'sparse', 1000)


@pytest.mark.parametrize('n', [1025, 5000])
def test_deform_bwd_generic_fallback(n):
    """A grid whose slices launch_deform_slice_bwd refuses (test_specs_reach_the_intended_kernels): the generic table backward."""
    assert not slices_fit(product_spec('fallback'))
    run_case('fallback', 'init', 'inside' if n == 5000 else 'nodes', 'tmid' if n == 5000 else 't1', 'dense', n)


def test_deform_bwd_device_count_below_capacity():
    """count = n_max - 37 read on the device; the input rows at and past count are NaN, the outputs there stay the pre-fill bit for bit
    (run_list), the gradients are finite and pass the rule for the first count entries."""
    res = run_case('prod', 'init', 'inside', 'tmid', 'dense', 1000 - 37, n_max=1000)
    for k in DR.PARAM_KEYS:
        assert torch.isfinite(res[k]).all(), k


def test_deform_bwd_count_zero():
    """count = 0 of n_max = 1000: nothing is written (run_list) and the gradients stay exactly 0."""
    res = run_list('prod', 'init', 'tmid', torch.zeros(0, 3), torch.zeros(0, 3), n_max=1000)
    for k in DR.PARAM_KEYS:
        assert not res[k].any(), k


def test_deform_bwd_accumulates_into_preloaded_gradients():
    """include/invr.h: "ACCUMULATES".  Gradient tensors pre-loaded with seeded non-zeros: pre-load + reference, the pre-load's magnitude
    in A and one more summand in c."""
    run_case('prod', 'init', 'inside', 't1', 'sparse', 1000, preload=True)


@pytest.mark.parametrize('kernel', list(LOOPS))
def test_deform_bwd_persistent_loop(kernel):
    run_case('prod', 'init', 'inside', 'tmid', 'dense', LOOPS[kernel])
