"""GPU: the backward kernels of the hash-grid encoder (csrc/k_encode.hip: k_part_encode_bwd, k_grid_encode_bwd_rt, k_expand_rows),
called through the C-ABI exactly as GridEncodeFn.backward does, against the float64 reference of tests/grid_reference.py —
element by element, every element of every output, none left out:

    |kernel - exact|  <=  8 noise  +  (c + 4) 2^-24 A  +  c 2^-126                      (tests/encoder_cases.py: accept, noise_of)

noise = the larger of the deviation of the oracle's own fp32 autograd and the largest move of `exact` under 4 ulp-sized
perturbations of the points (the convention of tests/conditioning.py); A = the absolute-sum companion, c = the number of
summands; an element no point reaches must be exactly 0.0; g_xyz is pre-filled with NaN so an unwritten element shows.  Nothing is
fitted to the kernels.  Each case prints K = max_e |kernel - exact| / (noise + 2^-23 A) for the kernel and for the fp32 oracle
(profiles/encoder_bwd_headroom.md keeps them).

Why element by element: the training tests hold a gradient tensor to 2e-4 of its maximum.  One lost flush of a run-length
accumulator at a tile end, one dropped cache slot, a mis-addressed hashed row or a wrong sign of one corner in g_xyz changes a few
elements by a few per cent of THOSE elements and nothing relative to the tensor's maximum.

tests/test_hostsim_encoder_bwd_cpu.py runs the same bodies on the CPU wave machine (DEV switched to 'cpu')."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import encoder_cases as EC       # noqa: E402  (checker only)
from tests import grid_reference as GR      # noqa: E402  (checker only)
from invr import _abi, params               # noqa: E402
from invr.config import make_cfg            # noqa: E402

DEV = 'cuda:0'

# ---- cases ------------------------------------------------------------------------------------------------------------------------
# part kernel (k_part_encode_bwd): 16-point tiles with ragged tails and fewer points than a tile; every cloud; the production
# table; the single-table form (no LDS routes)
PART = [('part-small', 'uniform', n) for n in (1, 15, 16, 17, 63, 64, 65)]
PART += [('part-small', c, 1000) for c in EC.CLOUDS]
PART += [('part-prod', c, 1000) for c in ('rays', 'one', 'faces')] + [('part-prod', 'uniform', 5000), ('part-prod', 'far', 4097)]
PART += [('part-onetable', 'uniform', 1000), ('part-onetable', 'far', 1000), ('part-onetable', 'rays', 4097), ('part-onetable', 'faces', 65)]
# generic kernel (k_grid_encode_bwd_rt + k_expand_rows): one workgroup, its edge, two workgroups, several
_GEN = ('deformer', 'deformer-small', 'deformer-nolds', 'rowscalar-generic', 'allhash', 'part-small-noinput', 'deformer-small-noinput')
GENERIC = [(t, c, n) for t in _GEN for c, n in (('uniform', 1), ('far', 1023), ('rays', 1024), ('faces', 1025), ('uniform', 5000))]
GENERIC += [('deformer-small', 'one', 1024), ('deformer-small', 'inside', 1024), ('rowscalar-generic', 'one', 1025)]
# large: the switch to 32-point tiles (n / 32 >= 4096), 64-point tiles and the persistent grid looping (512 workgroups x 4 waves x 64
# points = 131,072 < n); the generic kernel's grid-stride loop running twice (256 x 1024 threads)
LARGE = [('part-small', 'uniform', 65535), ('part-small', 'rays', 65535), ('part-prod', 'rays', 65535), ('part-prod', 'one', 65535)]
LARGE += [('part-prod', c, n) for n in (131071, 131072 + 5, 262144 + 37) for c in ('rays', 'uniform')]
LARGE += [('deformer-small', 'uniform', 262144 + 1000)]
ids = lambda cases: ['%s-%s-%d' % c for c in cases]


def product_spec(tag):
    return params.grid_spec(bbox=EC.BBOX, **EC.SPECS[tag])


@functools.lru_cache(maxsize=2)
def _dev_tables(tag, dev):
    dense, hsh = EC.make_tables(tag)
    return (None if dense is None else dense.to(dev)), hsh.to(dev), torch.tensor(EC.BBOX, dtype=torch.float32).to(dev)


def make_grid(tag, keep):
    dense, hsh, bounds = _dev_tables(tag, DEV)
    return _abi.make_grid(product_spec(tag), dense, hsh, bounds, keep), dense, hsh


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def run_bwd(tag, x, go, want_gxyz=True, into=None):
    """invr_grid_encode_bwd as GridEncodeFn.backward calls it: caller-zeroed tables (or `into`: accumulate), g_xyz full of NaN."""
    keep = []
    g, dense, hsh = make_grid(tag, keep)
    xd, god = x.to(DEV).contiguous(), go.to(DEV).contiguous()
    if into is None:
        g_hash = torch.zeros_like(hsh)
        g_dense = torch.zeros_like(dense) if dense is not None else None
    else:
        g_dense, g_hash = into
    g_xyz = torch.full_like(xd, float('nan')) if want_gxyz else None
    st = _abi.lib().invr_grid_encode_bwd(C.byref(g), _abi.ptr(xd), _abi.ptr(god), xd.shape[0], _abi.ptr(g_dense), _abi.ptr(g_hash),
                                         _abi.ptr(g_xyz), _abi.stream_ptr())
    _abi.check(st)
    sync()
    return {'g_xyz': g_xyz, 'g_dense': g_dense, 'g_hash': g_hash}


def inputs(tag, cloud, n, seed=0):
    spec = EC.make_spec(tag)
    return spec, EC.make_cloud(cloud, n, spec, seed), EC.make_gout(n, spec, seed)


def reference(tag, spec, x, go):
    dense, hsh = EC.make_tables(tag)
    ref = GR.encoder_bwd(x, go, dense, hsh, spec['bbox'], spec)
    noise, o32, touched = EC.noise_of(x, go, dense, hsh, spec, ref)
    return ref, noise, o32, touched


def judge(case_id, spec, cloud, out, ref, noise, o32, touched, keys=('g_xyz', 'g_dense', 'g_hash')):
    for k in keys:
        if ref[k] is None:
            assert out[k] is None
            continue
        val = out[k].cpu()
        EC.accept(case_id, k, val, ref[k], noise[k], o32[k], touched[k] if cloud == 'faces' else None)
        if k != 'g_xyz' and spec['sum'] and spec['sum_over_features']:          # k_expand_rows: all F columns of a row bit-identical
            bits = val.reshape(-1, spec['F']).view(torch.int32)
            assert (bits == bits[:, :1]).all(), (case_id, k)


def run_case(tag, cloud, n):
    spec, x, go = inputs(tag, cloud, n)
    out = run_bwd(tag, x, go)
    judge('%s-%s-%d' % (tag, cloud, n), spec, cloud, out, *reference(tag, spec, x, go))


def test_specs_reach_the_intended_kernels():
    """The spec families are what the case table says: table length, first hashed level, which levels take which route."""
    sp = EC.make_spec('part-small')
    assert (sp['T'], sp['start_hash'], sp['separate_dense']) == (4099, 7, True)
    sp = EC.make_spec('part-prod')
    assert (sp['T'], sp['start_hash']) == (262147, 11) and sp['res'][10] == 50 and sp['res'][5] ** 3 <= 1100 < sp['res'][6] ** 3
    assert EC.make_spec('allhash')['start_hash'] == 0 and not EC.make_spec('allhash')['separate_dense']
    assert not EC.make_spec('part-onetable')['separate_dense']
    d = params.deformer_grid_spec(make_cfg())
    o = EC.make_spec('deformer')
    for k in ('L', 'F', 'T', 'res', 'start_hash', 'separate_dense', 'sum', 'sum_over_features', 'include_input', 'out_dim'):
        assert d[k] == o[k], k
    lds = lambda tag: [(r ** 3 if l < s['start_hash'] else s['T']) * s['F'] <= 33792 for s in [EC.make_spec(tag)] for l, r in enumerate(s['res'])]
    assert all(lds('deformer-small')) and not all(lds('deformer-nolds')) and any(lds('deformer-nolds'))
    for tag in EC.SPECS:                                                        # the product's restatement agrees with the oracle's
        p, o = product_spec(tag), EC.make_spec(tag)
        assert (p['T'], p['res'], p['start_hash'], p['separate_dense'], p['dense_rows'], p['out_dim']) == \
               (o['T'], o['res'], o['start_hash'], o['separate_dense'], o['dense_rows'], o['out_dim']), tag
        assert torch.equal(torch.from_numpy(p['size']), o['size']), tag


@pytest.mark.parametrize('tag,cloud,n', PART, ids=ids(PART))
def test_encoder_bwd_part(tag, cloud, n):
    run_case(tag, cloud, n)


@pytest.mark.parametrize('tag,cloud,n', GENERIC, ids=ids(GENERIC))
def test_encoder_bwd_generic(tag, cloud, n):
    run_case(tag, cloud, n)


@pytest.mark.parametrize('tag,cloud,n', LARGE, ids=ids(LARGE))
def test_encoder_bwd_large(tag, cloud, n):
    run_case(tag, cloud, n)


@pytest.mark.parametrize('tag,n', [('part-small', 16), ('deformer-small', 64), ('rowscalar-generic', 64)])
def test_encoder_bwd_without_g_xyz_same_tables_bitwise(tag, n):
    """g_xyz = NULL leaves the table gradients bit-identical.  Sizes of ONE wave: with more, the order of the float atomics — and with
    it the last bit — is free to differ between two launches; the larger size is held to the acceptance rule instead."""
    spec, x, go = inputs(tag, 'uniform', n, seed=3)
    a, b = run_bwd(tag, x, go), run_bwd(tag, x, go, want_gxyz=False)
    assert b['g_xyz'] is None
    for k in ('g_dense', 'g_hash'):
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    spec, x, go = inputs(tag, 'uniform', 5000, seed=4)
    out = run_bwd(tag, x, go, want_gxyz=False)
    judge('%s-nogxyz-5000' % tag, spec, 'uniform', out, *reference(tag, spec, x, go), keys=('g_dense', 'g_hash'))


@pytest.mark.parametrize('tag', ['part-small', 'deformer-small'])
def test_encoder_bwd_no_points(tag):
    keep = []
    g, dense, hsh = make_grid(tag, keep)
    g_hash, g_dense = torch.zeros_like(hsh), torch.zeros_like(dense)
    x = torch.zeros(0, 3, device=DEV)
    st = _abi.lib().invr_grid_encode_bwd(C.byref(g), _abi.ptr(x), _abi.ptr(x), 0, _abi.ptr(g_dense), _abi.ptr(g_hash), None, _abi.stream_ptr())
    sync()
    assert st == 0
    assert not g_hash.any() and not g_dense.any()


@pytest.mark.parametrize('tag', ['part-small', 'deformer-small', 'allhash'])
def test_encoder_bwd_accumulates_into_unzeroed_tables(tag):
    """include/invr.h: "ACCUMULATES".  Two calls into the same tables = the reference of the concatenated cloud."""
    spec, x1, go1 = inputs(tag, 'uniform', 1000, seed=5)
    _, x2, go2 = inputs(tag, 'rays', 777, seed=6)
    a = run_bwd(tag, x1, go1)
    b = run_bwd(tag, x2, go2, into=(a['g_dense'], a['g_hash']))
    x, go = torch.cat([x1, x2]), torch.cat([go1, go2])
    out = {'g_xyz': torch.cat([a['g_xyz'], b['g_xyz']]), 'g_dense': b['g_dense'], 'g_hash': b['g_hash']}
    # (a row-scalar grid accumulates in column 0 and k_expand_rows copies it over the row after EACH call: the columns stay identical)
    judge('%s-accumulate' % tag, spec, 'uniform', out, *reference(tag, spec, x, go))


# ---- the list form of the fused training step (launch_part_encode_bwd_lists) -----------------------------------------------------
N_MAX = 150000
LISTS = [(t, c) for t in ('part-small', 'part-prod') for c in (0, 1, 17)]
LISTS_LARGE = [('part-small', 65535), ('part-prod', 65535), ('part-small', 140000), ('part-prod', 140000)]


def rows_of(d, h, F):
    """(dense (rows,F), hash (..,T,F)) -> (rows,) column 0 in invr_grid_row_sums order."""
    parts = [t.reshape(-1, F)[:, 0] for t in (d, h) if t is not None]
    return torch.cat(parts, 0)


def run_lists(tag, count):
    spec = EC.make_spec(tag)
    cloud = 'rays' if tag == 'part-prod' else 'uniform'
    x, go = EC.make_cloud(cloud, count, spec, seed=8), EC.make_gout(count, spec, seed=8)
    stride = N_MAX + 37                                                         # stride > n_max > count
    nan = float('nan')
    xs = torch.full((3, stride), nan)
    gs = torch.full((19, stride), nan)                                          # padding rows: nothing past `count` may reach a result
    xs[:, :count], gs[:, :count] = x.t(), go.t()
    keep = []
    g, dense, hsh = make_grid(tag, keep)
    nrows = int(_abi.lib().invr_grid_row_sums_len(C.byref(g)))
    assert nrows == GR.n_rows(spec)
    row_grad = torch.zeros(nrows, device=DEV)
    gx = torch.full((3, stride), nan, device=DEV)
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    xs, gs = xs.to(DEV), gs.to(DEV)
    st = _abi.lib().invr_part_encode_bwd_lists(C.byref(g), _abi.ptr(xs), _abi.ptr(gs), stride, N_MAX, _abi.ptr(cnt, torch.int32),
                                               _abi.ptr(row_grad), _abi.ptr(gx), _abi.stream_ptr())
    _abi.check(st)
    sync()
    gx, row_grad = gx.cpu(), row_grad.cpu()
    assert torch.isnan(gx[:, count:]).all(), 'g_x_soa written past count'
    cid = '%s-lists-%d' % (tag, count)
    if count == 0:
        assert not row_grad.any()
        return
    ref, noise, o32, touched = reference(tag, spec, x, go)
    EC.accept(cid, 'g_x_soa', gx[:, :count].t().contiguous(), ref['g_xyz'], noise['g_xyz'], o32['g_xyz'])
    F = spec['F']
    EC.accept(cid, 'row_grad', row_grad, GR.row_scalars(ref, spec), rows_of(noise['g_dense'], noise['g_hash'], F),
              rows_of(o32['g_dense'], o32['g_hash'], F))


@pytest.mark.parametrize('tag,count', LISTS, ids=['%s-%d' % c for c in LISTS])
def test_encoder_bwd_lists(tag, count):
    run_lists(tag, count)


@pytest.mark.parametrize('tag,count', LISTS_LARGE, ids=['%s-%d' % c for c in LISTS_LARGE])
def test_encoder_bwd_lists_large(tag, count):
    run_lists(tag, count)


def test_expand_row_grad_is_exact():
    """invr_expand_row_grad: every column of a row equals the row's scalar bit for bit, NaN-filled destinations are fully overwritten,
    rows whose scalar is 0 become 0, and the row order is the one in which invr_grid_encode_bwd fills column 0 of its tables."""
    tag = 'part-small'
    spec = EC.make_spec(tag)
    keep = []
    g, dense, hsh = make_grid(tag, keep)
    n = GR.n_rows(spec)
    gen = torch.Generator().manual_seed(5)
    rg = torch.randn(n, generator=gen) * (torch.rand(n, generator=gen) < 0.5)
    rg[:7] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, 1.0])
    gd, gh = torch.full_like(dense, float('nan')), torch.full_like(hsh, float('nan'))
    _abi.check(_abi.lib().invr_expand_row_grad(C.byref(g), _abi.ptr(rg.to(DEV)), _abi.ptr(gd), _abi.ptr(gh), _abi.stream_ptr()))
    sync()
    full = torch.cat([gd.cpu().reshape(-1, 16), gh.cpu().reshape(-1, 16)], 0)
    assert not torch.isnan(full).any()
    assert (full.view(torch.int32) == rg.view(torch.int32)[:, None]).all()
    assert (full[rg == 0] == 0).all()
    _, x, go = inputs(tag, 'uniform', 1000, seed=9)
    out = run_bwd(tag, x, go, want_gxyz=False)
    col0 = rows_of(out['g_dense'], out['g_hash'], 16).contiguous()
    gd, gh = torch.full_like(dense, float('nan')), torch.full_like(hsh, float('nan'))
    _abi.check(_abi.lib().invr_expand_row_grad(C.byref(g), _abi.ptr(col0), _abi.ptr(gd), _abi.ptr(gh), _abi.stream_ptr()))
    sync()
    assert torch.equal(gd.view(torch.int32), out['g_dense'].view(torch.int32)) and torch.equal(gh.view(torch.int32), out['g_hash'].view(torch.int32))
