"""GPU: the two kernels in the middle of a part's backward chain — k_part_mlp_bwd (csrc/k_mlp_bwd.hip) and k_wgrad (csrc/k_train.hip) —
called alone through the C-ABI in both forms (invr_part_mlp_bwd; invr_part_mlp_bwd_lists + invr_part_wgrad, the forms invr_train_bwd
launches), against the hand-written float64 reference of tests/mlp_reference.py — element by element, every element of every output:

    |kernel - exact|  <=  8 noise  +  (c + 4) 2^-24 A  +  c 2^-126                      (tests/mlp_cases.py: reference, accept)

noise = the largest of the fp32 autograd's deviation on the CPU, the move of `exact` under 4 ulp-sized input perturbations and its
move under the kernels' two documented VALUE errors (hardware sin / cos 2e-6, Softplus 1 ulp / 1.5e-7); A = the absolute-value
companion, c = the number of summands; A == 0 requires exactly 0.0.  Nothing is fitted to the kernels.  Each case prints
K = max_e |kernel - exact| / (noise + 2^-23 A) for the kernel and for the fp32 oracle (profiles/mlp_bwd_headroom.md keeps them).

Why element by element: the existing direct test holds a tensor to 2e-5 of its maximum against fp32 autograd.  A slip in one of
the backward's computed weight-image indices, or a derivative factor formed with an ABSOLUTE error (1 - exp(-softplus(z)) for z << 0),
changes a few columns — the latent block, the high-frequency direction columns, the rows of hidden units that are off for every
pair — by a few per cent of THOSE columns and nothing relative to the tensor's maximum.

Outputs are pre-filled: NaN where a kernel must write, a recognisable bit pattern where it must not (asserted bit-identical
afterwards), non-zero values where it accumulates.  tests/test_hostsim_mlp_bwd_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mlp_cases as MC           # noqa: E402  (checker only)
from tests import mlp_reference as MR       # noqa: E402  (checker only)
from invr import _abi                       # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
MARK = -0x365A5A5B                          # int32 bit pattern 0xC9A5A5A5 = -1358004.6f: what no kernel may touch
PID_DEFAULT = 2

SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)              # a partial tile, one wave (16 pairs), one workgroup (64) and their edges
LOOP_N = 512 * 64 + 17                                          # the persistent grid (512 workgroups x 64 pairs): a second pass for workgroup 0
WGRAD_COUNTS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)    # a k-step (4 rows), a slab (256), a workgroup's four slabs and their edges
WGRAD_LOOP = 48 * 4 * 256 + 300                                 # the persistent grid (48 workgroups x 4 waves x 256 rows): a second slab for two waves


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def marked(*shape):
    return torch.full(shape, MARK, dtype=torch.int32).view(torch.float32)


def assert_marked(t, what):
    assert (t.contiguous().view(torch.int32) == MARK).all(), '%s: written where nothing may be written' % what


def make_model(P, pid, keep):
    """An InvrModel with part `pid` carrying the parameter set (the MLP entry points read nothing else)."""
    m = _abi.InvrModel()
    dev = lambda ts: [t.to(DEV) for t in ts]
    part = m.part[pid]
    part.occ = _abi.make_mlp(dev(P['occ_w']), dev(P['occ_b']), keep)
    part.rgb = _abi.make_mlp(dev(P['rgb_w']), dev(P['rgb_b']), keep)
    lat = P['latent_table'].to(DEV).contiguous()
    keep.append(lat)
    part.rgb_latent, part.latent_dim, part.num_latent_code = lat.data_ptr(), 8, lat.shape[0]
    m.n_dir_freq, m.geo_feature_dim = 4, 16
    return m


def prefill(n_rgb, count, stride, n_pad):
    """-> g_emb (20,stride), gz (5,n_pad,64), a (5,n_pad,72): NaN where the kernel must write, MARK everywhere else."""
    g_emb, gz, a = marked(20, stride), marked(5, n_pad, 64), marked(5, n_pad, 72)
    g_emb[:19, :count] = NAN
    for l in range(5):
        if l == 3 and n_rgb != 3:
            continue
        gz[l, :count, :MR.OUT_DIMS[l]] = NAN
        a[l, :count, :72 if l == 2 else MR.IN_DIMS[l]] = NAN
    return g_emb, gz, a


def run_mlp_bwd(P, pid, latent_index, emb, dirs, g_raw, entry='plain', stride=None, n_max=None, slots=False, latent_full=False, seed=0):
    """One call of invr_part_mlp_bwd (entry 'plain') or invr_part_mlp_bwd_lists, plus invr_part_mlp_fwd on the same inputs.
    -> dict of CPU tensors cut to the first `count` pairs, in the reference's layouts; g_latent with its pre-loaded value subtracted
    nowhere (the caller judges pre + gradient); every must-not-touch region already asserted."""
    count = emb.shape[0]
    n_rgb = len(P['rgb_w'])
    if entry == 'plain':
        stride = n_max = count
    stride = stride if stride is not None else count
    n_max = n_max if n_max is not None else count
    n_pad = n_max + 3
    keep = []
    model = make_model(P, pid, keep)
    g = torch.Generator().manual_seed(11 + seed)
    li = torch.tensor([latent_index], dtype=torch.int64, device=DEV)
    # inputs: NaN past `count` (nothing there may reach a result)
    emb_soa, dirs_soa = torch.full((20, stride), NAN), torch.full((3, stride), NAN)
    emb_soa[:19, :count], emb_soa[19, :count], dirs_soa[:, :count] = emb.t(), 0.0, dirs.t()
    l_slot = None
    if slots:                                                    # a random injective map into cap = 3 n slots; (cap,5) float4, NaN elsewhere
        cap = 3 * max(count, 1)
        perm = torch.randperm(cap, generator=g)[:count].to(torch.int32)
        graws = torch.full((cap, 5, 4), NAN)
        graws[perm.long(), pid] = g_raw
        free = sorted(set(range(cap)) - set(perm.tolist()))[0]
        l_slot = torch.full((stride,), free, dtype=torch.int32)   # (past count: a valid slot whose row is NaN)
        l_slot[:count] = perm
        l_slot = l_slot.to(DEV)
    else:
        graws = torch.full((stride, 4), NAN)
        graws[:count] = g_raw
    g_emb, gz, a = prefill(n_rgb, count, stride, n_pad)
    num_latent = P['latent_table'].shape[0]
    pre_lat = torch.randn(num_latent if latent_full else 1, 8, generator=g) * 0.3
    emb_soa, dirs_soa, graws, g_emb, gz, a, g_lat = [t.to(DEV).contiguous() for t in (emb_soa, dirs_soa, graws, g_emb, gz, a, pre_lat.clone())]
    out = _abi.InvrMlpBwdOut()
    out.g_emb, out.gz, out.a, out.n_pad, out.g_latent = g_emb.data_ptr(), gz.data_ptr(), a.data_ptr(), n_pad, g_lat.data_ptr()
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    L = _abi.lib()
    if entry == 'plain':
        st = L.invr_part_mlp_bwd(C.byref(model), pid, _abi.ptr(li, torch.int64), _abi.ptr(emb_soa), _abi.ptr(dirs_soa), count,
                                 _abi.ptr(graws), C.byref(out), _abi.stream_ptr())
    else:
        st = L.invr_part_mlp_bwd_lists(C.byref(model), pid, _abi.ptr(li, torch.int64), _abi.ptr(emb_soa), _abi.ptr(dirs_soa), stride, n_max,
                                       _abi.ptr(cnt, torch.int32), _abi.ptr(graws), _abi.ptr(l_slot, torch.int32), C.byref(out),
                                       int(latent_full), _abi.stream_ptr())
    _abi.check(st)
    raw = marked(count + 2, 4).to(DEV)
    if count:
        raw[:count] = NAN
        fe, fd = emb_soa[:, :count].contiguous(), dirs_soa[:, :count].contiguous()
        _abi.check(L.invr_part_mlp_fwd(C.byref(model), pid, _abi.ptr(li, torch.int64), _abi.ptr(fe), _abi.ptr(fd), count,
                                       _abi.ptr(cnt, torch.int32), _abi.ptr(raw), _abi.stream_ptr()))
    sync()
    g_emb, gz, a, g_lat, raw = g_emb.cpu(), gz.cpu(), a.cpu(), g_lat.cpu(), raw.cpu()
    # ---- what must not have been touched
    assert_marked(g_emb[19], 'g_emb row 19')
    assert_marked(g_emb[:, count:], 'g_emb columns >= count')
    assert_marked(gz[:, count:], 'gz rows >= count')
    assert_marked(a[:, count:], 'a rows >= count')
    assert_marked(raw[count:], 'raw rows >= count')
    if n_rgb != 3:
        assert_marked(gz[3], 'gz[3] of a 2-linear colour net')
        assert_marked(a[3], 'a[3] of a 2-linear colour net')
    assert_marked(gz[4][:, 3:], 'gz[4] columns 3..63')
    assert_marked(gz[1][:, 17:], 'gz[1] columns 17..63')
    assert_marked(a[0][:, 19:], 'a[0] columns 19..71')
    for l in (1, 3, 4):
        assert_marked(a[l][:, 64:], 'a[%d] columns 64..71' % l)
    row = latent_index if latent_full else 0
    others = [r for r in range(pre_lat.shape[0]) if r != row]
    assert torch.equal(g_lat[others].view(torch.int32), pre_lat[others].view(torch.int32)), 'latent gradient: another row was written'
    res = dict(raw=raw[:count], g_emb=g_emb[:19, :count].t().contiguous(), g_latent=g_lat[row], pre_latent=pre_lat[row])
    for l in range(5):
        if l == 3 and n_rgb != 3:
            continue
        res['gz%d' % l] = gz[l, :count, :MR.OUT_DIMS[l]].contiguous()
        if l == 2:
            a2 = a[2, :count]
            assert not a2[:, MR.PAD_SLOTS].any(), 'a[2]: a padding k-slot is not 0'
            res['a2'] = MR.unslot_a2(a2)
        else:
            res['a%d' % l] = a[l, :count, :MR.IN_DIMS[l]].contiguous()
    res['stacks'] = (gz.to(DEV), a.to(DEV), n_pad, cnt)
    return res


MLP_KEYS = ('raw', 'g_emb', 'g_latent', 'gz', 'a')


@functools.lru_cache(maxsize=2)
def _reference(tag, n_rgb, n, pattern, latent_index):
    emb, dirs = MC.make_inputs(n)
    P = MC.with_latent(MC.make_params(tag, n_rgb), latent_index)
    return MC.reference(emb, dirs, P, MC.make_graw(n, pattern))


def judge(cid, res, ref, noise, o32, keys=MLP_KEYS, pre=None):
    """Every output of `keys` through the rule (all of them, so that every K line is printed), then the failures together.
    pre: name -> pre-loaded value of an output that accumulates (one more summand in exact, A and c)."""
    pre = pre or {}
    failures = []
    for k in ref:
        if not k.startswith(keys):
            continue
        r, o = ref[k], o32[k]
        if k in pre:
            r, o = MC.preloaded(r, pre[k]), o.double() + pre[k].double()
        try:
            MC.accept(cid, k, res[k], r, noise[k], o)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


def run_case(tag, n_rgb, n, pattern, entry, latent_index=MC.NUM_LATENT - 1, pid=PID_DEFAULT, **kw):
    if tag != 'init' and latent_index == MC.NUM_LATENT - 1:
        MC.check_params(tag, n_rgb, n)
    emb, dirs = MC.make_inputs(n)
    res = run_mlp_bwd(MC.make_params(tag, n_rgb), pid, latent_index, emb, dirs, MC.make_graw(n, pattern), entry=entry, **kw)
    ref, noise, o32 = _reference(tag, n_rgb, n, pattern, latent_index)
    cid = '%s-%d-%s-%d-%s' % (tag, n_rgb, pattern, n, entry)
    judge(cid, res, ref, noise, o32, pre={'g_latent': res['pre_latent']})
    if pattern == 'sparse':                                      # the pairs the merge dropped: every gradient row exactly +-0.0
        zero = ~MC.make_graw(n, pattern).any(1)
        assert zero.any()
        for k in res:
            if k.startswith('gz') or k == 'g_emb':
                assert not res[k][zero].any(), (cid, k)
    return res


ENTRIES = ('plain', 'lists')                                     # (both in one test: they share the case's reference)


@pytest.mark.parametrize('n', SIZES)
def test_mlp_bwd_sizes(n):
    for entry in ENTRIES:
        run_case('init', 3 if n % 2 else 2, n, 'dense', entry, slots=entry == 'lists')


MATRIX = [(t, d, p) for t in MC.WEIGHT_SETS for d in (2, 3) for p in MC.PATTERNS]


@pytest.mark.parametrize('tag,n_rgb,pattern', MATRIX, ids=['%s-%d-%s' % c for c in MATRIX])
def test_mlp_bwd_matrix(tag, n_rgb, pattern):
    for entry in ENTRIES:
        run_case(tag, n_rgb, 1000, pattern, entry, slots=entry == 'lists')


def test_mlp_bwd_persistent_loop():
    for entry in ENTRIES:
        run_case('init', 3, LOOP_N, 'dense', entry)


@pytest.mark.parametrize('count', [0, 1, 999])
def test_mlp_bwd_lists_device_count(count):
    """count read on the device, far below what the launch was sized for (n_max = stride = 1024)."""
    if count == 0:
        emb, dirs = MC.make_inputs(1)
        res = run_mlp_bwd(MC.make_params('init', 3), PID_DEFAULT, 0, emb[:0], dirs[:0], torch.zeros(0, 4), entry='lists', stride=1024, n_max=1024)
        assert torch.equal(res['g_latent'].view(torch.int32), res['pre_latent'].view(torch.int32))
        return
    run_case('init', 3, count, 'dense', 'lists', stride=1024, n_max=1024)


def test_mlp_bwd_lists_count_equals_n_max_below_stride():
    run_case('init', 2, 300, 'dense', 'lists', stride=557, n_max=300)


@pytest.mark.parametrize('pid', [0, 4])
def test_mlp_bwd_lists_slot_indirection(pid):
    """g_raw fetched as g_raws[l_slot[pair] * 5 + part] from a (cap,5) array that is NaN everywhere else."""
    run_case('init', 3 if pid else 2, 777, 'sparse', 'lists', pid=pid, slots=True, stride=800, n_max=790)


@pytest.mark.parametrize('latent_index', [MC.NUM_LATENT - 1, 0])
def test_mlp_bwd_lists_latent_full(latent_index):
    """latent_full = 1: the kernel accumulates into row latent_index of the whole (num_latent,8) tensor and leaves the other rows alone."""
    run_case('init', 3, 500, 'dense', 'lists', latent_index=latent_index, latent_full=True, slots=True)


# ---- k_wgrad alone ---------------------------------------------------------------------------------------------------------------------
def run_wgrad(gz_l, a_l, n_rgb, count, n_pad, seed=0):
    """invr_part_wgrad on stacks built from per-layer (count,O_l) / (count,I_l) matrices: rows >= count NaN, every column past a
    layer's width and the padding k-slots of a[2] 1e30, dW / db pre-loaded.  -> (results name -> CPU tensor, pre-loaded values)."""
    gz, a = torch.full((5, n_pad, 64), NAN), torch.full((5, n_pad, 72), NAN)
    for l in range(5):
        if gz_l[l] is None:
            continue                                             # (a 2-linear colour net: layer 3 stays NaN, it may not be read)
        gz[l, :count], a[l, :count] = 1e30, 1e30
        gz[l, :count, :MR.OUT_DIMS[l]] = gz_l[l]
        a[l, :count, :72 if l == 2 else MR.IN_DIMS[l]] = MR.slot_a2(a_l[l]) if l == 2 else a_l[l]
        if l == 2:
            a[l, :count, MR.PAD_SLOTS] = 1e30
    return call_wgrad(gz.to(DEV), a.to(DEV), n_rgb, torch.tensor([count], dtype=torch.int32, device=DEV), n_pad, seed)


def call_wgrad(gz, a, n_rgb, cnt, n_pad, seed=0):
    g = torch.Generator().manual_seed(21 + seed)
    shapes = [(64, 19), (17, 64), (64, 70), (64, 64), (3, 64)]
    pre, dev = {}, {}
    pW, pb = (C.c_void_p * 5)(), (C.c_void_p * 5)()
    for l in range(5):
        if l == 3 and n_rgb != 3:
            continue
        pre['dW%d' % l], pre['db%d' % l] = torch.randn(shapes[l], generator=g) * 0.1, torch.randn(shapes[l][0], generator=g) * 0.1
        dev['dW%d' % l], dev['db%d' % l] = pre['dW%d' % l].clone().to(DEV), pre['db%d' % l].clone().to(DEV)
        pW[l], pb[l] = dev['dW%d' % l].data_ptr(), dev['db%d' % l].data_ptr()
    _abi.check(_abi.lib().invr_part_wgrad(_abi.ptr(gz), _abi.ptr(a), n_pad, n_rgb, pW, pb, _abi.ptr(cnt, torch.int32), _abi.stream_ptr()))
    sync()
    return {k: v.cpu() for k, v in dev.items()}, pre


def judge_wgrad(cid, res, pre, ref, noise, o32):
    assert set(res) == set(ref)
    judge(cid, res, ref, noise, o32, keys=('dW', 'db'), pre=pre)


def wgrad_case(count, n_rgb, n_pad=None):
    gz_l, a_l = MC.wgrad_stacks(count, n_rgb)
    res, pre = run_wgrad(gz_l, a_l, n_rgb, count, n_pad if n_pad is not None else count + 5)
    judge_wgrad('wgrad-%d-%d' % (count, n_rgb), res, pre, *MC.wgrad_reference(gz_l, a_l))


@pytest.mark.parametrize('n_rgb', [2, 3])
@pytest.mark.parametrize('count', WGRAD_COUNTS)
def test_wgrad(count, n_rgb):
    wgrad_case(count, n_rgb)


@pytest.mark.parametrize('n_rgb', [2, 3])
def test_wgrad_persistent_loop(n_rgb):
    wgrad_case(WGRAD_LOOP, n_rgb)


def test_wgrad_count_zero_and_far_below_n_pad():
    gz_l, a_l = MC.wgrad_stacks(0, 3)
    res, pre = run_wgrad(gz_l, a_l, 3, 0, 2000)                  # (every row NaN-or-1e30: nothing may be read)
    for k in pre:
        assert torch.equal(res[k].view(torch.int32), pre[k].view(torch.int32)), k
    wgrad_case(100, 3, n_pad=60000)                              # the grid is sized from n_pad: all but one workgroup leave at once


# ---- the chain: lists -> wgrad -> the ten parameter gradients --------------------------------------------------------------------------
CHAIN = [(t, d, n) for t in ('wide', 'dead') for d in (2, 3) for n in (1000, 5000)]


@pytest.mark.parametrize('tag,n_rgb,n', CHAIN, ids=['%s-%d-%d' % c for c in CHAIN])
def test_chain_parameter_gradients(tag, n_rgb, n):
    """invr_part_mlp_bwd_lists -> invr_part_wgrad on the stacks as the kernel left them (MARK / NaN past count and all): the ten
    parameter gradients, every element — the rows of the `dead` units included, which are made of derivative factors e^z, z in [-18, -6]."""
    MC.check_params(tag, n_rgb, n)
    emb, dirs = MC.make_inputs(n)
    res = run_mlp_bwd(MC.make_params(tag, n_rgb), PID_DEFAULT, MC.NUM_LATENT - 1, emb, dirs, MC.make_graw(n, 'dense'), entry='lists',
                      slots=True, stride=n + 40, n_max=n + 8)
    gz, a, n_pad, cnt = res['stacks']
    out, pre = call_wgrad(gz, a, n_rgb, cnt, n_pad)
    ref, noise, o32 = _reference(tag, n_rgb, n, 'dense', MC.NUM_LATENT - 1)
    cid = 'chain-%s-%d-%d' % (tag, n_rgb, n)
    judge(cid, out, ref, noise, o32, keys=('dW', 'db'), pre=pre)
    assert len(out) == (10 if n_rgb == 3 else 8)
