"""Test infrastructure shared by the part-MLP backward tests (tests/test_mlp_reference_cpu.py, tests/test_gpu_mlp_bwd.py and its
wave-machine twin): seeded weight sets, inputs, upstream-gradient patterns, the per-element noise scale and the acceptance rule.
Checker only: the one product function used is invr.autograd.part_mlps_torch — the torch-op statement of the two MLPs — whose fp32
autograd on the CPU is the oracle of noise class (a); no kernel is reached from here.

The rule is the one of tests/encoder_cases.py (EC.accept), every element judged, none left out:
    |kernel - exact| <= 8 noise + (c + 4) 2^-24 A + c 2^-126,        A == 0 requires exactly 0.0
noise per element = the largest of
  (a) the deviation from `exact` of torch's fp32 autograd of part_mlps_torch on the CPU,
  (b) the largest move of `exact` under 4 sign-random perturbations of the inputs: emb and dirs by (|x| + 1) 2^-23, g_raw by
      |g| 2^-23 (zero rows stay zero),
  (c) the largest move of `exact` under 4 sign-random draws of the two VALUE errors the kernels document: the sin / cos features
      offset by +-2e-6 (csrc/common.h, sincos_hw) and every forward Softplus output by +-max(1 fp32 ulp of itself, 1.5e-7)
      (csrc/mlp_common.h softplus4, csrc/common.h softplus_f).  Values only: the reference's derivative factors stay computed from z.
Nothing is fitted to a kernel."""
import functools
import types

import torch

from tests import encoder_cases as EC
from tests import mlp_reference as MR

N_BASE = 5000                      # the seeded input batch; a case of n <= N_BASE pairs takes its first n rows
WEIGHT_SETS = ('init', 'wide', 'dead')
PATTERNS = ('dense', 'sparse', 'occ-only', 'rgb-only')
N_DEAD = 8
HIDDEN = {2: ('occ1', 'rgb1'), 3: ('occ1', 'rgb1', 'rgb2')}
NUM_LATENT = 5


@functools.lru_cache(maxsize=4)
def make_inputs(n, seed=0):
    """-> emb (n,19), dirs (n,3) float32.  emb ~ 0.5 N(0,1); dirs of norm 0.5 .. 1.5; pair 0 has d = 0 exactly, pair 1 |d| = 12 (the
    largest argument of the hardware sin is then 8 x 12 = 96, inside the range sincos_hw documents).  n <= N_BASE: the first n rows of
    the base batch, so that what is asserted about a weight set on the base batch holds for every such case."""
    if n <= N_BASE and seed == 0:
        m = N_BASE
    else:
        m = n
    g = torch.Generator().manual_seed(4242 + seed + (0 if m == N_BASE else m))
    emb = torch.randn(m, 19, generator=g) * 0.5
    dirs = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=1) * (0.5 + torch.rand(m, 1, generator=g))
    dirs[0] = 0.0
    if m > 1:
        dirs[1] = torch.nn.functional.normalize(dirs[1], dim=0) * 12.0
    return emb[:n].contiguous(), dirs[:n].contiguous()


def make_graw(n, pattern, seed=0):
    g = torch.Generator().manual_seed(99 + seed + 7 * PATTERNS.index(pattern))
    gr = torch.randn(max(n, N_BASE), 4, generator=g)
    if pattern == 'sparse':                                        # as after the merge: most pairs did not win their sample
        gr[torch.rand(gr.shape[0], generator=g) < 0.7] = 0.0
    elif pattern == 'occ-only':
        gr[:, :3] = 0.0
    elif pattern == 'rgb-only':
        gr[:, 3] = 0.0
    return gr[:n].contiguous()


def _init_params(n_rgb, g):
    """nn.Linear's own initialisation scale (params._linear: U(-1/sqrt(fan_in), 1/sqrt(fan_in))); latent ~ N(0, 2/8)."""
    def lin(o, i):
        k = 1.0 / i ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * k, (torch.rand(o, generator=g) * 2 - 1) * k
    occ = [lin(64, 19), lin(17, 64)]
    rgb = [lin(64, 70)] + ([lin(64, 64)] if n_rgb == 3 else []) + [lin(3, 64)]
    latent = torch.randn(NUM_LATENT, 8, generator=g) * 0.5
    return dict(occ_w=[w for w, _ in occ], occ_b=[b for _, b in occ], rgb_w=[w for w, _ in rgb], rgb_b=[b for _, b in rgb],
                latent_table=latent)


def with_latent(P, latent_index):
    return dict(P, latent=P['latent_table'][latent_index])


def _zs(P, latent_index=NUM_LATENT - 1):
    emb, dirs = make_inputs(N_BASE)
    return MR.part_mlps(emb, dirs, with_latent(P, latent_index), torch.zeros(N_BASE, 4), companions=False)['z']


_LAYER = {'occ1': ('occ', 0), 'rgb1': ('rgb', 0), 'rgb2': ('rgb', 1)}


@functools.lru_cache(maxsize=None)
def make_params(tag, n_rgb):
    """Seeded float32 parameters of one part.  `wide`: every layer rescaled in turn, on the base batch and in float64, so that the
    hidden pre-activations of the ordinary pairs (all but the |d| = 12 one) reach +-15 and each of the four head logits spans [-20, 20].  `dead`: wide,
    then N_DEAD units of every 64-wide layer get their weight row shrunk and their bias moved so that the unit's pre-activation lies in
    [-17, -7] for EVERY pair of the base batch.  check_params asserts both on the reference."""
    g = torch.Generator().manual_seed(31 + n_rgb)
    P = _init_params(n_rgb, g)
    if tag == 'init':
        return P
    ordinary = torch.ones(N_BASE, dtype=torch.bool)
    ordinary[1] = False

    def rescale(kind, l, rows, z, target, centre=False):
        z = z[ordinary].reshape(int(ordinary.sum()), -1)
        W, b = P[kind + '_w'][l], P[kind + '_b'][l]
        if centre:                                                 # a head: every logit row spans [-target, target] on its own
            lo, hi = z.min(0).values, z.max(0).values
            f = 2.0 * target / (hi - lo)
            W[rows] = (W[rows].double() * f[:, None]).float()
            b[rows] = (b[rows].double() * f - f * (hi + lo) / 2.0).float()
        else:
            f = target / float(z.abs().max())
            W[rows], b[rows] = (W[rows].double() * f).float(), (b[rows].double() * f).float()
    z = _zs(P)
    rescale('occ', 0, slice(None), z['occ1'], 15.0)
    rescale('occ', 1, slice(0, 1), _zs(P)['lg'], 20.0, centre=True)
    rescale('rgb', 0, slice(None), _zs(P)['rgb1'], 15.0)
    if n_rgb == 3:
        rescale('rgb', 1, slice(None), _zs(P)['rgb2'], 15.0)
    rescale('rgb', n_rgb - 1, slice(None), _zs(P)['zo'], 20.0, centre=True)
    if tag == 'wide':
        return P
    assert tag == 'dead'
    for name in HIDDEN[n_rgb]:
        kind, l = _LAYER[name]
        rows = dead_units(name)
        z = _zs(P)[name][:, rows]
        lo, hi = z.min(0).values, z.max(0).values
        W, b = P[kind + '_w'][l], P[kind + '_b'][l]
        f = (10.0 / (hi - lo)).clamp(max=1.0)
        W[rows] = (W[rows].double() * f[:, None]).float()
        mid = ((hi + lo) / 2 - b[rows].double()) * f               # the centre of the shrunk row's own contribution
        b[rows] = (-12.0 - mid).float()
    return P


def dead_units(name):
    g = torch.Generator().manual_seed(500 + sum(map(ord, name)))
    return torch.randperm(64, generator=g)[:N_DEAD].sort().values


def check_params(tag, n_rgb, n):
    """The ranges a weight set promises, asserted on the float64 reference for the first n pairs of the base batch."""
    assert n <= N_BASE
    z = _zs(make_params(tag, n_rgb))
    if tag == 'init':
        return
    ordinary = torch.ones(n, dtype=torch.bool)
    ordinary[1:2] = False
    for name in HIDDEN[n_rgb]:
        zz = z[name][:n]
        live = torch.ones(64, dtype=torch.bool)
        if tag == 'dead':
            d = dead_units(name)
            live[d] = False
            assert float(zz[:, d].min()) >= -18.0 and float(zz[:, d].max()) <= -6.0, (tag, name, float(zz[:, d].min()), float(zz[:, d].max()))
        zo = zz[ordinary][:, live]
        assert -18.0 <= float(zo.min()) <= -9.0 and 9.0 <= float(zo.max()) <= 18.0, (tag, name, float(zo.min()), float(zo.max()))
    for name, hi in (('lg', 26.0), ('zo', 26.0)):
        zo = z[name][:n][ordinary]
        assert -hi <= float(zo.min()) <= -12.0 and 12.0 <= float(zo.max()) <= hi, (tag, name, float(zo.min()), float(zo.max()))


# ---- the fp32 oracle: torch autograd of part_mlps_torch on the CPU -------------------------------------------------------------------
def _pn(P, dtype):
    t = lambda x: x.to(dtype).clone().requires_grad_()
    mk = lambda ws, bs: types.SimpleNamespace(linears=[types.SimpleNamespace(weight=t(w), bias=t(b)) for w, b in zip(ws, bs)])
    return types.SimpleNamespace(occ=mk(P['occ_w'], P['occ_b']), rgb=mk(P['rgb_w'], P['rgb_b']), rgb_latent=t(P['latent'].reshape(1, 8)))


def oracle(emb, dirs, P, g_raw, dtype=torch.float32):
    """Autograd of invr.autograd.part_mlps_torch in `dtype` on the CPU -> the outputs of MR.part_mlps as plain tensors.  gz[l] and
    a[l] are read off the graph: the gradient arriving at each linear's node and the input it saved."""
    from invr import autograd as AG
    pn = _pn(P, dtype)
    e = emb.to(dtype).clone().requires_grad_()
    raw = AG.part_mlps_torch(pn, e, dirs.to(dtype), torch.zeros(1, dtype=torch.long), MR.N_FREQ)
    shapes = {(64, 19): 0, (17, 64): 1, (64, 70): 2, (64, 64): 3, (3, 64): 4}
    gz, a = [None] * 5, [None] * 5
    seen, todo = set(), [raw.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        todo += [f for f, _ in node.next_functions]
        if 'LinearFn' in node.name():
            x, w = node.saved_tensors
            l = shapes[tuple(w.shape)]
            a[l] = x.detach()
            node.register_prehook(lambda go, l=l: gz.__setitem__(l, go[0].detach().clone()))
    raw.backward(g_raw.to(dtype))
    lins = pn.occ.linears + pn.rgb.linears
    idx = [0, 1, 2, 3, 4] if len(pn.rgb.linears) == 3 else [0, 1, 2, 4]
    dW, db = [None] * 5, [None] * 5
    for l, lin in zip(idx, lins):
        dW[l], db[l] = lin.weight.grad, lin.bias.grad
    return dict(raw=raw.detach(), g_emb=e.grad, g_latent=pn.rgb_latent.grad.reshape(-1), gz=gz, a=a, dW=dW, db=db)


LIST_KEYS = ('gz', 'a', 'dW', 'db')


def flatten(out):
    """dict with per-layer lists -> flat dict name -> value ('gz2', 'dW0', ...; absent layers dropped)."""
    flat = {k: out[k] for k in ('raw', 'g_emb', 'g_latent')}
    for k in LIST_KEYS:
        for l in range(5):
            if out[k][l] is not None:
                flat['%s%d' % (k, l)] = out[k][l]
    return flat


def reference(emb, dirs, P, g_raw, trials=4, seed=0):
    """-> (ref: name -> MR.Ref, noise: name -> tensor, o32: name -> tensor), names as flatten() gives them."""
    ref = flatten(MR.part_mlps(emb, dirs, P, g_raw))
    o32 = flatten(oracle(emb, dirs, P, g_raw))
    noise = {k: (o32[k].double() - ref[k].exact).abs() for k in ref}
    g = torch.Generator().manual_seed(3000 + seed)
    sign = lambda *s: torch.randint(0, 2, s, generator=g).double() * 2.0 - 1.0
    e64, d64, g64 = emb.double(), dirs.double(), g_raw.double()
    n = emb.shape[0]
    three = len(P['rgb_w']) == 3

    def fold(p):
        p = flatten(p)
        for k in ref:
            noise[k] = torch.maximum(noise[k], (p[k].exact - ref[k].exact).abs())
    for _ in range(trials):                                                                                     # (b)
        fold(MR.part_mlps(e64 + sign(n, 19) * (e64.abs() + 1.0) * 2.0 ** -23, d64 + sign(n, 3) * (d64.abs() + 1.0) * 2.0 ** -23, P,
                          g64 + sign(n, 4) * g64.abs() * 2.0 ** -23, companions=False))
    for _ in range(trials):                                                                                     # (c)
        sp = dict(occ1=sign(n, 64), rgb1=sign(n, 64), lg=sign(n))
        if three:
            sp['rgb2'] = sign(n, 64)
        fold(MR.part_mlps(e64, d64, P, g64, companions=False, sincos_off=sign(n, 24) * 2e-6, softplus_sign=sp))
    return ref, noise, o32


def accept(tag, name, val, ref, noise, o32=None):
    """EC.accept, unchanged: the rule, the NaN / shape checks, the exact zeros, and the K_kernel / K_oracle32 line (prefix MLPB)."""
    return EC.accept(tag, name, val, ref, noise, o32, report=lambda s: print('MLPB' + s[4:]))


def preloaded(ref, pre):
    """The Ref of `pre + value` for an output that ACCUMULATES into a pre-loaded tensor: one more summand."""
    return MR.Ref(ref.exact + pre.double(), ref.A + pre.double().abs(), ref.c + 1.0)


# ---- k_wgrad alone: synthetic stacks ----------------------------------------------------------------------------------------------------
def wgrad_stacks(count, n_rgb, seed=0):
    """Random gz[l] (count,O_l) and a[l] (count,I_l) float32, a[2] in weight-column order; nothing of the MLP kernel.  A tenth of the gz
    rows are exactly zero (the merge) and the magnitudes span four decades, as the real stacks do."""
    g = torch.Generator().manual_seed(777 + count + n_rgb)
    gz, a = [None] * 5, [None] * 5
    for l in range(5):
        if l == 3 and n_rgb != 3:
            continue
        scale = 10.0 ** (torch.rand(count, 1, generator=g) * 4 - 3)
        gz[l] = torch.randn(count, MR.OUT_DIMS[l], generator=g) * scale * (torch.rand(count, 1, generator=g) > 0.1)
        a[l] = torch.randn(count, MR.IN_DIMS[l], generator=g)
    return gz, a


def wgrad_reference(gz, a):
    """-> (ref, noise, o32) for names dW<l>, db<l>: exact = gz^T a, A = |gz|^T |a|, c = count; noise = the fp32 matmul's deviation."""
    ref, noise, o32 = {}, {}, {}
    for l in range(5):
        if gz[l] is None:
            continue
        G, X = gz[l].double(), a[l].double()
        n = float(G.shape[0])
        ref['dW%d' % l] = MR.Ref(G.t() @ X, G.abs().t() @ X.abs(), n)
        ref['db%d' % l] = MR.Ref(G.sum(0), G.abs().sum(0), n)
        o32['dW%d' % l] = gz[l].t() @ a[l]
        o32['db%d' % l] = gz[l].sum(0)
    for k in ref:
        noise[k] = (o32[k].double() - ref[k].exact).abs()
    return ref, noise, o32
