"""GPU: the FORWARD kernels of the hash-grid encoder (csrc/k_encode.hip: k_grid_encode_rt, k_part_encode, k_part_encode_rows_all,
k_part_encode_rs, k_part_encode_rs_xcd, k_row_sums) through the C-ABI, against the float64 reference of tests/grid_reference.py —
element by element, every element of every output, none left out:

    |kernel - exact|  <=  8 noise  +  (c + 4) 2^-24 A  +  c 2^-126                 (tests/encoder_cases.py: accept, forward_noise)

One rule for every cloud: the CELL decision is the reference's own discrete fp32 decision (GR.fp32_cells: correctly rounded IEEE
operations, defined without any kernel), everything continuous is float64.  noise = the larger of the deviation of the oracle's fp32
forward and the largest move of `exact` under 4 ulp-sized perturbations of the points with the cells held; A = the absolute-sum
companion, c = the number of summands.  Outputs are pre-filled with NaN where a kernel must write and carry a marker where it must not.
Nothing is fitted to the kernels.  Each case prints K = max_e |kernel - exact| / (noise + 2^-23 A) for the kernel and for the fp32
oracle (profiles/encoder_fwd_headroom.md keeps them).

Why element by element: a flat bound on a level sum passes a mis-addressed hashed row at one corner (a few per cent of one ~0.1
value), a lost reload of a far second corner (one point in ten million in a frame — every `ties` point here) or a tile dealt to the
wrong offset of a part's list.  What the part kernels add over the rule: the three input columns are the fp32 quotient bit for bit
(the cells depend on it), and the two row-sum kernels agree bit for bit — every variant arm between them (reciprocal division hoisted
per tile or tested per quotient, the LDS-staged dense level, pair loads, the x-delta fold, the one-round modulo) is documented in the
source as "same bits".

tests/test_hostsim_encoder_fwd_cpu.py runs the same bodies on the CPU wave machine (DEV switched to 'cpu')."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import encoder_cases as EC       # noqa: E402  (checker only)
from tests import grid_reference as GR      # noqa: E402  (checker only)
from invr import _abi, params               # noqa: E402
from invr.config import make_cfg, PART_NAMES  # noqa: E402

DEV = 'cuda:0'
MARK = 12345.0                                # where a kernel must not write

# ---- cases ------------------------------------------------------------------------------------------------------------------------
PART_TAGS = ('part-small', 'part-prod', 'part-onetable', 'part-base16', 'part-t9', 'part-t19', 'part-t20')
PART_CLOUDS = EC.CLOUDS + ('ties',)
# k_part_encode walks a 64-point tile two points at a time (odd tiles duplicate the last point); the row-sum kernels take 256 per
# workgroup: every n around both, each with another cloud, then every cloud at 1000
PART = [(t, PART_CLOUDS[(i + j) % len(PART_CLOUDS)], n) for j, t in enumerate(PART_TAGS) for i, n in enumerate((1, 2, 63, 64, 65, 255, 256, 257))]
PART += [(t, c, 1000) for t in PART_TAGS for c in PART_CLOUDS]
# the x-delta fold wrapping through the table's end, either way (one pair in T / 60 of the other clouds): the three families that take it
PART += [(t, 'wrap', 256) for t in ('part-prod', 'part-t19', 'part-t20')]
PART.sort(key=lambda c: PART_TAGS.index(c[0]))                                  # (one family's tables at a time)
# generic kernel: 128 threads per workgroup
_GEN_CLOUDS = ('uniform', 'far', 'rays', 'faces', 'one')
GENERIC = [(t, _GEN_CLOUDS[(i + j) % 5], n) for j, t in enumerate(EC.SPECS) for i, n in enumerate((1, 127, 128, 129, 1000))]
GENERIC += [(t, 'ties', 1000) for t in EC.SPECS if t.startswith('part-') and 'noinput' not in t]
GENERIC.sort(key=lambda c: list(EC.SPECS).index(c[0]))
# large: the XCD kernel's tile-stride loop running twice (256 tiles of 256 per level group); the persistent grids of the row kernel
# (2048 workgroups x 4 waves x 64) and of the one-part row-sum kernel (2048 x 256) looping
LARGE = [('part-prod', 'rays', 65536 + 300, (0,)), ('part-small', 'uniform', 524288 + 37, (1, 2))]
ids = lambda cases: ['%s-%s-%d' % c[:3] for c in cases]


def family(tag):
    return EC.SPECS[tag] if tag in EC.SPECS else EC.SPECS_FWD[tag]


def with_bbox(spec, bbox):
    return spec if bbox is None else dict(spec, bbox=torch.tensor(bbox, dtype=torch.float32))


def product_spec(tag, bbox=None):
    return params.grid_spec(bbox=bbox if bbox is not None else EC.BBOX_OF.get(tag, EC.BBOX), **family(tag))


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=6)
def device_grid(tag, dev, bbox=None):
    """-> (InvrGrid with its row-sum table from invr_grid_row_sums where the grid has one, row sums or None, keep-alive list)."""
    dense, hsh = EC.make_tables(tag)
    spec = product_spec(tag, None if bbox is None else [list(bbox[:3]), list(bbox[3:])])
    keep = []
    g = _abi.make_grid(spec, None if dense is None else dense.to(dev), hsh.to(dev), torch.from_numpy(spec['bbox']).to(dev), keep)
    rs = None
    if spec['sum'] and spec['sum_over_features']:
        n = int(_abi.lib().invr_grid_row_sums_len(C.byref(g)))
        assert n == GR.n_rows(EC.make_spec(tag))
        rs = torch.full((n,), float('nan'), device=dev)
        _abi.check(_abi.lib().invr_grid_row_sums(C.byref(g), _abi.ptr(rs), _abi.stream_ptr()))
        sync()
        g.row_sums = rs.data_ptr()
    return g, rs, keep


def grid_of(tag, bbox=None):
    return device_grid(tag, DEV, None if bbox is None else tuple(bbox[0]) + tuple(bbox[1]))[0]


def aligned_bytes(nbytes):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


def run_generic(tag, x):
    out = torch.full((x.shape[0], EC.make_spec(tag)['out_dim']), float('nan'), device=DEV)
    xd = x.to(DEV).contiguous()
    _abi.check(_abi.lib().invr_grid_encode_fwd(C.byref(grid_of(tag)), _abi.ptr(xd), x.shape[0], _abi.ptr(out), _abi.stream_ptr()))
    sync()
    return out.cpu()


def run_part(tag, x, kernel, bbox=None):
    """invr_part_encode_fwd: xyz (n,3) -> (n,19) through kernel 0 (XCD row sums), 1 (64-byte rows) or 2 (one-part row sums)."""
    n = x.shape[0]
    out = torch.full((n, 19), float('nan'), device=DEV)
    xd = x.to(DEV).contiguous()
    L = _abi.lib()
    nbytes = L.invr_part_encode_workspace(n)
    ws = aligned_bytes(nbytes)
    _abi.check(L.invr_part_encode_fwd(C.byref(grid_of(tag, bbox)), _abi.ptr(xd), n, kernel, _abi.ptr(out), C.c_void_p(ws.data_ptr()), nbytes,
                                      _abi.stream_ptr()))
    sync()
    return out.cpu()


@functools.lru_cache(maxsize=8)
def reference(tag, cloud, n, seed=0, bbox=None):
    """Computed once per case and shared by its kernels -> x, Ref, noise, the fp32 oracle's output, torch's fp32 normalised xyz."""
    spec = with_bbox(EC.make_spec(tag), None if bbox is None else [list(bbox[:3]), list(bbox[3:])])
    x = EC.make_cloud(cloud, n, spec, seed)
    return (x,) + judge_inputs(tag, spec, x, seed)


def judge_inputs(tag, spec, x, seed=0):
    dense, hsh = EC.make_tables(tag)
    cells = GR.fp32_cells(x, spec['bbox'], spec)
    ref = GR.encoder_fwd(x, dense, hsh, spec['bbox'], spec, cells=cells)
    noise, o32 = EC.forward_noise(x, dense, hsh, spec, ref, cells, seed=seed)
    b = spec['bbox']
    return ref, noise, o32, (x - b[0]) / (b[1] - b[0])


def judge(cid, name, out, ref, noise, o32, xn32, input_cols=True):
    K = EC.accept(cid, name, out, ref, noise, o32, prefix='ENCF')
    if input_cols:                                                              # bit for bit: the cells depend on it
        assert torch.equal(out[:, :3].contiguous().view(torch.int32), xn32.contiguous().view(torch.int32)), (cid, name, 'input columns')
    return K


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- which family reaches which route -----------------------------------------------------------------------------------------------
def routes(spec):
    """A restatement of make_grid_dev's rule (csrc/invr_abi.hip) and of the staging rule of k_part_encode_rs_xcd: the hash reduction a
    grid's hashed levels take inside level_rowsum, rcell != 0 per level, the levels staged into LDS."""
    T, res = int(spec['T']), [int(r) for r in spec['res']]
    k = T.bit_length() - 1
    c = T - (1 << k)
    mod32 = mod24 = xdelta = mod1r = False
    if 10 <= k <= 30 and c > 0:
        y1 = c * ((1 << 41) >> k)
        y2 = c * (y1 >> k)
        y3 = c * (y2 >> k)
        mod32 = y1 < 2 ** 32 and y2 < 2 ** 32 and y3 < T and (y3 >> k) == 0 and T < 2 ** 30
        mod24 = mod32 and c < 2 ** 24 and ((1 << 41) >> k) < 2 ** 24 and (y1 >> k) < 2 ** 24 and (y2 >> k) < 2 ** 24
        xdelta = mod24 and T > 2 ** 14 and y2 < (1 << k) and 2 * max(res) <= T
        xbits = (max(res) * GR.HASH_P2).bit_length()
        mod1r = xdelta and xbits > k and c * ((1 << xbits) >> k) < 2 * T and 3 * T < 2 ** 31
    name = 'mod24_1r+xdelta' if mod1r else 'mod24_2r+xdelta' if xdelta else 'mod24' if mod24 else 'mod32' if mod32 else 'mod64'
    cell = np.asarray(spec['size'], dtype=np.float32)
    rcell = [bool(9.6e-7 < float(b) < 1.0e6 and (int(np.float32(b).view(np.uint32)) & 0x7fffff) != 0x7fffff) for b in cell]
    staged = [l for l in range(min(int(spec['start_hash']), 8)) if res[l] ** 3 <= 4096]
    return name, rcell, staged


def test_families_reach_the_intended_routes():
    """Every hash-reduction route of level_rowsum is named by the family that reaches it, and each of the five production grids of
    config.DEFAULTS is matched by a tested family in its hash route and in its staged levels.  (No nextprime(2^k) table length, k = 10
    .. 30, reaches the plain three-round hash_mod24 WITHOUT the x-delta fold: mod24 needs k >= 18, and every such length has c^2 <
    2^(3k - 41) and 2 res <= T — the loop below states it.)"""
    want = {'part-small': ('mod32', 4099, 7), 'part-onetable': ('mod32', 4099, 7), 'part-prod': ('mod24_1r+xdelta', 262147, 11),
            'part-base16': ('mod32', 65537, 3), 'part-t9': ('mod64', 521, 5), 'part-t19': ('mod24_2r+xdelta', 524309, 12),
            'part-t20': ('mod24_1r+xdelta', 1048583, 13)}
    got = {}
    for tag in PART_TAGS:
        p, o = product_spec(tag), EC.make_spec(tag)
        assert (p['T'], p['res'], p['start_hash'], p['separate_dense'], p['dense_rows'], p['out_dim']) == \
               (o['T'], o['res'], o['start_hash'], o['separate_dense'], o['dense_rows'], o['out_dim']), tag
        assert torch.equal(torch.from_numpy(p['size']), o['size']) and torch.equal(torch.from_numpy(p['bbox']), o['bbox']), tag
        name, rcell, staged = routes(p)
        assert (name, p['T'], p['start_hash']) == want[tag], (tag, name, p['T'], p['start_hash'])
        assert all(rcell), (tag, rcell)                                         # (1 / (res - 1) never has a mantissa of all ones here)
        got[tag] = (name, staged)
    assert got['part-small'][1] == got['part-prod'][1] == list(range(7)) and got['part-t9'][1] == list(range(5))
    assert got['part-base16'][1] == [0] and product_spec('part-base16')['res'][0] ** 3 == 4096          # exactly ENC_LDS_ROWS
    cfg = make_cfg()
    prod = {name: routes(params.part_grid_spec(cfg, name)) for name in PART_NAMES}
    assert {n: r[0] for n, r in prod.items()} == {'body': 'mod24_1r+xdelta', 'leg': 'mod24_1r+xdelta', 'head': 'mod24_1r+xdelta',
                                                 'larm': 'mod32', 'rarm': 'mod32'}
    assert params.part_grid_spec(cfg, 'body')['T'] == params.part_grid_spec(cfg, 'leg')['T'] == product_spec('part-t20')['T']
    assert params.part_grid_spec(cfg, 'head')['T'] == product_spec('part-prod')['T']
    for n, (name, rcell, staged) in prod.items():
        assert all(rcell), n
        assert any(name == g[0] for g in got.values()) and any(staged == g[1] for g in got.values()), (n, name, staged)
    for k in range(10, 31):                                                     # plain hash_mod24: reached by no nextprime length
        T = params.next_prime(2 ** k)
        name = routes(dict(T=T, res=[2, 2008], size=[1.0, 1.0], start_hash=0))[0]
        assert name != 'mod24', (k, T)


# ---- generic kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,cloud,n', GENERIC, ids=ids(GENERIC))
def test_encoder_fwd_generic(tag, cloud, n):
    x, ref, noise, o32, xn32 = reference(tag, cloud, n)
    judge('%s-%s-%d' % (tag, cloud, n), 'generic', run_generic(tag, x), ref, noise, o32, xn32, input_cols=EC.make_spec(tag)['include_input'])


# ---- part kernels ------------------------------------------------------------------------------------------------------------------
def run_part_case(tag, cloud, n, kernels=(0, 1, 2)):
    x, ref, noise, o32, xn32 = reference(tag, cloud, n)
    out = {}
    for k in kernels:
        out[k] = run_part(tag, x, k)
        judge('%s-%s-%d' % (tag, cloud, n), 'kernel%d' % k, out[k], ref, noise, o32, xn32)
    if 0 in out and 2 in out:
        assert same_bits(out[0], out[2]), 'kernels 0 and 2 differ in %d elements' % int((out[0].view(torch.int32) != out[2].view(torch.int32)).sum())


@pytest.mark.parametrize('tag,cloud,n', PART, ids=ids(PART))
def test_encoder_fwd_part(tag, cloud, n):
    run_part_case(tag, cloud, n)


@pytest.mark.parametrize('tag,cloud,n,kernels', LARGE, ids=ids(LARGE))
def test_encoder_fwd_large(tag, cloud, n, kernels):
    run_part_case(tag, cloud, n, kernels)


@pytest.mark.parametrize('tag', ['part-small', 'part-prod', 'part-base16'])
def test_encoder_fwd_exact_division_beside_the_reciprocal_form(tag):
    """Points with a normalised coordinate of exactly 0 (on a lower face of the box: div_exact's range test fails, the wave takes the
    hardware division) mixed into waves of ordinary points, whose waves alone take the reciprocal form (kernel 0: decided once per
    tile; kernel 2: per quotient): every point's 19 values are bit-identical to the same point in a run of its own kind."""
    spec = EC.make_spec(tag)
    b = spec['bbox']
    plain = EC.make_cloud('uniform', 512, spec, seed=11)
    zero = EC.make_cloud('uniform', 64, spec, seed=12)
    zero[torch.arange(64), torch.arange(64) % 3] = b[0][torch.arange(64) % 3]           # x_n == 0.0 on one axis
    zero[::5, 1] = b[0, 1]
    faces = EC.make_cloud('faces', 64, spec, seed=13)
    special = torch.cat([zero, faces])
    assert ((plain - b[0]) / (b[1] - b[0]) != 0).all()
    where = torch.arange(128) * 5 + 2                                           # a dozen special points in every wave of the mixed run
    mixed = torch.zeros(640, 3)
    is_special = torch.zeros(640, dtype=torch.bool)
    is_special[where] = True
    mixed[is_special], mixed[~is_special] = special, plain
    ref = judge_inputs(tag, spec, mixed, seed=11)
    for k in (0, 1, 2):
        m, p, s = run_part(tag, mixed, k), run_part(tag, plain, k), run_part(tag, special, k)
        judge('%s-mixed-640' % tag, 'kernel%d' % k, m, *ref)
        assert same_bits(m[~is_special], p), (k, 'ordinary points differ beside exact-division lanes')
        assert same_bits(m[is_special], s), (k, 'exact-division points differ beside ordinary lanes')


# ---- five parts in one launch --------------------------------------------------------------------------------------------------------
# five families / tables / bounds; part 1 (a 4096-row level 0) directly after a base-2 part: the staged LDS level is replaced by a larger one
FIVE = [('part-small', [[-0.5, -1.0, -0.3], [0.5, 0.9, 0.4]], 'ties'), ('part-base16', [[-1, -1.2, -0.34], [0.8, 0.7, 0.5]], 'uniform'),
        ('part-t9', [[-0.3, 0.3, -0.3], [0.3, 0.7, 0.3]], 'faces'), ('part-prod', [[0.2, 0, -0.2], [0.9, 0.35, 0.2]], 'ties'),
        ('part-onetable', [[-0.9, 0, -0.2], [-0.2, 0.35, 0.2]], 'far')]
FIVE_COUNTS = [((300, 0, 1, 700, 256), 700, 704), ((65, 64, 63, 0, 1), 65, 65), ((257, 257, 257, 257, 257), 600, 640)]


def run_five(counts, cap, stride, kernel):
    """invr_part_encode_fwd_all -> per part the (20, cap) SoA output.  The point lists are NaN past a count and the outputs carry NaN
    below it (must be written) and MARK at and past it (must not)."""
    L = _abi.lib()
    grids = (_abi.InvrGrid * 5)(*[grid_of(t, bb) for t, bb, _ in FIVE])
    xs, embs, pts = [], [], []
    for p, (tag, bb, cloud) in enumerate(FIVE):
        x = reference(tag, cloud, counts[p], 20 + p, tuple(bb[0]) + tuple(bb[1]))[0] if counts[p] else torch.zeros(0, 3)
        soa = torch.full((3, stride), float('nan'))
        soa[:, :counts[p]] = x.t()
        e = torch.full((20, cap), MARK)
        e[:, :counts[p]] = float('nan')
        pts.append(x); xs.append(soa.to(DEV)); embs.append(e.to(DEV))
    cnt = torch.tensor(counts, dtype=torch.int32).to(DEV)
    xp = (C.c_void_p * 5)(*[_abi.ptr(t).value for t in xs])
    ep = (C.c_void_p * 5)(*[_abi.ptr(t).value for t in embs])
    _abi.check(L.invr_part_encode_fwd_all(grids, xp, stride, _abi.ptr(cnt, torch.int32), cap, kernel, ep, _abi.stream_ptr()))
    sync()
    return pts, [e.cpu() for e in embs]


@pytest.mark.parametrize('kernel', [0, 1])
@pytest.mark.parametrize('counts,cap,stride', FIVE_COUNTS, ids=['-'.join(map(str, c[0])) for c in FIVE_COUNTS])
def test_encoder_fwd_five_parts_one_launch(counts, cap, stride, kernel):
    """The frame's five-part launches with more than one non-empty part: the per-part tile rotation wrapping, the level-group rotation,
    the staged dense level replaced between parts, workgroups without a tile of a part, an empty part.  Each part is judged by the
    rule, is bit-identical to the same points through the one-part entry, and nothing at or past a count is written."""
    pts, embs = run_five(counts, cap, stride, kernel)
    for p, (tag, bb, cloud) in enumerate(FIVE):
        n, e = counts[p], embs[p]
        assert (e[:, n:] == MARK).all(), 'part %d: written at or past its count' % p
        if n == 0:
            continue
        assert (e[19, :n] == 0).all(), 'part %d: pad row' % p
        out = e[:19, :n].t().contiguous()
        x, ref, noise, o32, xn32 = reference(tag, cloud, n, 20 + p, tuple(bb[0]) + tuple(bb[1]))
        judge('five-%s-part%d-%s-%d' % ('-'.join(map(str, counts)), p, tag, n), 'kernel%d' % kernel, out, ref, noise, o32, xn32)
        assert same_bits(out, run_part(tag, x, kernel, bb)), 'part %d differs from the one-part launch' % p


def test_encoder_fwd_all_refuses_bad_arguments():
    L = _abi.lib()
    grids = (_abi.InvrGrid * 5)(*[grid_of(t, bb) for t, bb, _ in FIVE])
    five = (C.c_void_p * 5)()
    assert L.invr_part_encode_fwd_all(grids, five, 8, None, 8, 0, five, None) != 0 and b'null pointer' in L.invr_last_error()
    one = torch.zeros(8, dtype=torch.int32).to(DEV)
    assert L.invr_part_encode_fwd_all(grids, five, 8, _abi.ptr(one, torch.int32), 8, 2, five, None) != 0 and b'kernel must be' in L.invr_last_error()
    assert L.invr_part_encode_fwd_all(grids, five, 8, _abi.ptr(one, torch.int32), 9, 0, five, None) != 0 and b'cap <= stride' in L.invr_last_error()
    assert L.invr_part_encode_fwd_all(grids, five, 8, _abi.ptr(one, torch.int32), 8, 0, five, None) != 0 and b'null list' in L.invr_last_error()
    assert L.invr_part_encode_fwd_all(grids, five, 8, _abi.ptr(one, torch.int32), 0, 0, five, None) == 0          # nothing to do


# ---- row sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['part-small', 'part-onetable', 'rowscalar-generic'])
def test_grid_row_sums_elementwise(tag):
    """invr_grid_row_sums, every element: |kernel - float64 row sum| <= (F + 4) 2^-24 sum |row| (an fp32 sum of F terms in any order);
    F = 16 (one quad per row), F = 4 (the atomic arm into a zeroed table), the single-table layout."""
    spec = EC.make_spec(tag)
    dense, hsh = EC.make_tables(tag)
    rs = device_grid(tag, DEV)[1].cpu()
    s, a = GR.row_sums64(dense, hsh, spec)
    assert rs.shape == s.shape and not torch.isnan(rs).any()
    err, bound = (rs.double() - s).abs(), (spec['F'] + 4.0) * 2.0 ** -24 * a
    print('ENCF %-44s row_sums max err / bound %.3g' % (tag, float((err / bound.clamp(min=1e-300)).max())))
    assert (err <= bound).all(), int((err > bound).sum())
