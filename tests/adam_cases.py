"""CHECKER ONLY (imports nothing of the product): one Adam step in float64, its derived per-element error bound, the input kinds, the
canary-fenced arrays and the case tables of tests/test_gpu_adam_step.py.

Reference (torch/optim/adam.py:_single_tensor_adam, amsgrad off), in float64 from the SAME fp32 arrays p, g, m, v and the SAME fp32
scalars the device table hands the kernel (lr, weight_decay, bc1, bc2_sqrt; eps; w1 = float(1 - beta1), w2 = float(1 - beta2) with the
subtraction in double; float(beta2)):

    g' = wd p + g                 (only when wd != 0)
    m' = m + w1 (g' - m)
    v' = w2 g'^2 + float(b2) v
    p' = p - (lr / bc1) * m' / (sqrt(v') / bc2_sqrt + eps)

Bound: first-order propagation of one rounding (u = 2^-24 relative, 2^-149 absolute) per fp32 operation of the update, evaluated
in float64 from the reference's own intermediates (nothing fitted to any implementation):

    E_g = u |g'|                                               (0 when wd == 0)
    E_m = u (|m'| + 2 w1 |g' - m|) + w1 E_g
    E_v = u (|v'| + w2 g'^2 + b2 v) + 2 w2 |g'| E_g
    E_s = min(E_v / 2 sqrt(v'), sqrt(E_v)) + u sqrt(v')
    E_d = E_s / bc2_sqrt + u sqrt(v') / bc2_sqrt + u den       (den = sqrt(v') / bc2_sqrt + eps)
    E_q = E_m / den + |q| E_d / den + u |q|                    (q = m' / den)
    E_p = (lr / bc1) E_q + 2 u |upd| + u |p'|                  (upd = (lr / bc1) q)

each plus 4 x 2^-149.  Accepted: |x - exact| <= 2 E_x for p', m', v' (the factor 2: second-order terms, another order of the same
operations).  K = max_e |x - exact| / E_x is what the tests print; K <= 2 passes."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
ACCEPT = 2.0
CHUNK = 16384                   # elements per workgroup of the fused step (invr_adam_chunk_elems(); the tests assert it)
HOSTSIM_MAX = 200000            # cases above this many elements run on the CPU wave machine only under HOSTSIM_FULL=1


def f32(x):
    return float(np.float32(x))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bias_corrections(step, betas=(0.9, 0.999)):
    """(bc1, bc2_sqrt) as the host forms them: Python doubles, rounded to fp32 once."""
    return f32(1.0 - betas[0] ** step), f32(math.sqrt(1.0 - betas[1] ** step))


def scalars(lr, wd, step, betas=(0.9, 0.999), eps=1e-15, bc=None):
    """The fp32 scalars of one step (bc: the pair read back from a device table, else the host's own)."""
    bc1, bc2s = bc if bc is not None else bias_corrections(step, betas)
    return dict(lr=f32(lr), wd=f32(wd), bc1=bc1, bc2s=bc2s, eps=f32(eps), w1=f32(1.0 - betas[0]), w2=f32(1.0 - betas[1]), b2=f32(betas[1]),
                betas=betas, step=step)


def reference(p, g, m, v, sc):
    """-> {'p','m','v': exact float64 results, 'Ep','Em','Ev': the bounds} of one step (g already expanded to p's length)."""
    p, g, m, v = (x.detach().cpu().double().reshape(-1) for x in (p, g, m, v))
    w1, w2, b2, lr, wd, bc1, bc2s, eps = (sc[k] for k in ('w1', 'w2', 'b2', 'lr', 'wd', 'bc1', 'bc2s', 'eps'))
    T = 4 * TINY
    if wd != 0.0:
        gp = wd * p + g
        Eg = U * gp.abs() + T
    else:
        gp, Eg = g, torch.zeros_like(g)
    d = gp - m
    mp = m + w1 * d
    Em = U * (mp.abs() + 2 * w1 * d.abs()) + w1 * Eg + T
    vp = w2 * gp * gp + b2 * v
    Ev = U * (vp.abs() + w2 * gp * gp + b2 * v) + 2 * w2 * gp.abs() * Eg + T
    s = vp.sqrt()
    Es = torch.minimum(Ev / (2 * s), Ev.sqrt()) + U * s + T           # (s == 0: E_v / 0 = inf, the minimum takes sqrt(E_v))
    den = s / bc2s + eps
    Ed = Es / bc2s + U * s / bc2s + U * den + T
    q = mp / den
    Eq = Em / den + q.abs() * Ed / den + U * q.abs() + T
    ss = lr / bc1
    upd = ss * q
    pp = p - upd
    Ep = ss * Eq + 2 * U * upd.abs() + U * pp.abs() + T
    return {'p': pp, 'm': mp, 'v': vp, 'Ep': Ep, 'Em': Em, 'Ev': Ev}


def headroom(out, ref):
    """K per quantity: max_e |x - exact| / E_x (inf for a non-finite output)."""
    ks = {}
    for k in 'pmv':
        x = out[k].detach().cpu().double().reshape(-1)
        if not torch.isfinite(x).all():
            ks[k] = float('inf')
            continue
        ks[k] = float(((x - ref[k]).abs() / ref['E' + k]).max()) if x.numel() else 0.0
    return ks


def torch_adam32(p, g, m, v, sc):
    """torch's own fp32 Adam on CPU tensors, one step from the injected state: the second opinion the rule is validated with."""
    q = p.detach().cpu().clone().reshape(-1).requires_grad_()
    opt = torch.optim.Adam([q], lr=sc['lr'], betas=sc['betas'], eps=sc['eps'], weight_decay=sc['wd'], foreach=False)
    opt.state[q] = {'step': torch.tensor(float(sc['step'] - 1)), 'exp_avg': m.detach().cpu().clone().reshape(-1),
                    'exp_avg_sq': v.detach().cpu().clone().reshape(-1)}
    q.grad = g.detach().cpu().clone().reshape(-1)
    opt.step()
    return {'p': q.detach(), 'm': opt.state[q]['exp_avg'], 'v': opt.state[q]['exp_avg_sq']}


def accept(case_id, out, ref, inputs=None, sc=None, family='step'):
    """Print K of the kernel (and of torch's fp32 Adam when `inputs` is given), then hold the kernel to the rule."""
    ks = headroom(out, ref)
    line = 'ADAM-K %s %s kernel p=%.3f m=%.3f v=%.3f' % (family, case_id, ks['p'], ks['m'], ks['v'])
    if inputs is not None:
        kt = headroom(torch_adam32(*inputs, sc), ref)
        line += ' torch32 p=%.3f m=%.3f v=%.3f' % (kt['p'], kt['m'], kt['v'])
    print(line)
    for k in 'pmv':
        x = out[k].detach().cpu().reshape(-1)
        assert torch.isfinite(x).all(), (case_id, k, 'non-finite output')
        assert ks[k] <= ACCEPT, (case_id, k, ks[k], int(((x.double() - ref[k]).abs() / ref['E' + k]).argmax()))
    assert (out['v'].detach().cpu() >= 0).all(), (case_id, 'v < 0')
    return ks


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
KINDS = ('first', 'training', 'spike', 'zeros', 'tiny', 'wide', 'cancel')


def make_inputs(kind, n, sc, seed=0, n_grad=None):
    """fp32 CPU arrays p, g, m, v of `n` elements (g: n_grad elements when given — a row-scalar gradient)."""
    gen = torch.Generator().manual_seed(1000 * seed + 17 * KINDS.index(kind) + n % 9973)
    rn = lambda k=n: torch.randn(k, generator=gen, dtype=torch.float64)
    ru = lambda k=n: torch.rand(k, generator=gen, dtype=torch.float64)
    ng = n if n_grad is None else n_grad
    p = 0.1 * rn()
    g = 1e-3 * rn(ng)
    m = 1e-3 * rn()
    v = 1e-6 * (0.25 + ru()) ** 2
    if kind == 'first':
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    elif kind == 'training':
        pass
    elif kind == 'spike':
        assert ng == n
        g = torch.sign(rn()) * 10.0 ** (2 + 2 * ru()) * v.sqrt()
    elif kind == 'zeros':
        g = torch.zeros(ng, dtype=torch.float64)
        sel = torch.arange(n) % 4                                  # 0, 1: m = v = 0;  2: small m, small v;  3: small m, subnormal v
        m = torch.where(sel >= 2, 1e-5 * rn(), torch.zeros(n, dtype=torch.float64))
        v = torch.where(sel == 2, 1e-12 * (0.25 + ru()), torch.where(sel == 3, 1e-41 * (0.25 + ru()), torch.zeros(n, dtype=torch.float64)))
    elif kind == 'tiny':
        p = 1e-8 * rn()                                            # (small enough that an update of lr * 1e-6 moves it)
        g, m, v = 1e-21 * rn(ng), 1e-21 * rn(), 1e-42 * (0.1 + ru())
    elif kind == 'wide':
        mag = lambda k=n: torch.sign(rn(k)) * 2.0 ** (-60 + 80 * ru(k))
        p, g, m, v = mag(), mag(ng), mag(), mag().abs()
    elif kind == 'cancel':
        assert ng == n
        g = m.float().double() * (1 + 1e-6 * rn())
        r = reference(torch.zeros(n), g.float(), m.float(), v.float(), dict(sc, wd=0.0))
        p = -r['p'] * (1 + 1e-3 * rn())                            # p ~ the update: cancellation in p - upd
    else:
        raise KeyError(kind)
    return p.float(), g.float(), m.float(), v.float()


# ---- canary-fenced arrays -------------------------------------------------------------------------------------------------------------
CANARY = 64
CANARY_BITS = 0x4B3C5A69          # a finite float (1.2e7): read as data it wrecks the result, overwritten it shows


class Carved:
    """`n` floats inside a larger buffer with CANARY floats of a fixed bit pattern before and CANARY + CHUNK after (a workgroup that
    does not stop at numel runs to the end of its 16384-element chunk: that lands in canaries, not in somebody else's memory); the
    array starts 16-byte aligned (mis = 0) or one float later (mis = 1: the 4-byte-odd offset a contiguous view t[1:] has)."""

    def __init__(self, values, dev, mis=0):
        values = values.detach().reshape(-1).float()
        n = values.numel()
        self.buf = torch.empty(CANARY + 8 + n + CANARY + CHUNK, dtype=torch.float32, device=dev)
        self.buf.view(torch.int32).fill_(CANARY_BITS)
        self.o = CANARY + ((-(self.buf.data_ptr() + 4 * CANARY)) % 16) // 4 + mis
        self.n = n
        self.t = self.buf[self.o:self.o + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 4 * mis and self.t.is_contiguous()
        self.before = self.bits()

    ptr = property(lambda s: s.t.data_ptr())

    def bits(self):
        return self.t.view(torch.int32).cpu().clone()

    def cpu(self):
        return self.t.cpu().clone()

    def canaries_intact(self):
        b = self.buf.view(torch.int32).cpu()
        return bool((b[:self.o] == CANARY_BITS).all()) and bool((b[self.o + self.n:] == CANARY_BITS).all())

    def unchanged(self):
        """bit-for-bit what it was when carved (and the canaries around it)"""
        return self.canaries_intact() and torch.equal(self.bits(), self.before)


def same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 16383, 16384, 16385, 2 * 16384 + 3, 5 * 4099 * 16,
         64 * 19, 17 * 64, 64 * 70, 3 * 64, 32 * 32, 3 * 32]
STEPS = [1, 2, 7, 1000, 100000]
WDS = [0.0, 0.01]
LRS = [5e-4, 5e-4, 1e-2]
ALL_KINDS_AT = (4099, 16385)


def _single_cases():
    """(kind, n, step, weight_decay, lr): `training` at every size, every kind at 4099 and 16385; steps, weight decays and learning
    rates cycled with coprime periods (5, 2, 3) so that they mix; `first` is step 1 by definition."""
    out, k = [], 0
    for n in SIZES:
        kinds = KINDS if n in ALL_KINDS_AT else ('training',)
        for kind in kinds:
            out.append((kind, n, 1 if kind == 'first' else STEPS[k % 5], WDS[k % 2], LRS[k % 3]))
            k += 1
    for n in ALL_KINDS_AT:                                           # untouched rows with and without weight decay, early and late
        out += [('zeros', n, 1, 0.0, 5e-4), ('zeros', n, 1000, 0.01, 5e-4), ('first', n, 1, 0.0, 5e-4), ('tiny', n, 2, 0.0, 5e-4),
                ('spike', n, 100000, 0.0, 5e-4)]
    return out


SINGLE = _single_cases()
SINGLE_SMALL = [c for c in SINGLE if c[1] <= HOSTSIM_MAX]
SINGLE_LARGE = [c for c in SINGLE if c[1] > HOSTSIM_MAX]
single_id = lambda c: '%s-%d-s%d-wd%g-lr%g' % c

# row-scalar gradients: (rows, shift, kind, step, wd)
ROW_ROWS = [1, 3, 1024, 1025, 4099, 16384 + 1]
ROWS = [(rows, sh, ('training', 'first', 'wide', 'tiny', 'zeros', 'training')[(i + j) % 6], STEPS[(i + 2 * j) % 5], WDS[(i + j) % 2])
        for i, rows in enumerate(ROW_ROWS) for j, sh in enumerate((1, 2, 4))]
ROWS_SMALL = [c for c in ROWS if (c[0] << c[1]) <= HOSTSIM_MAX]
ROWS_LARGE = [c for c in ROWS if (c[0] << c[1]) > HOSTSIM_MAX]
row_id = lambda c: 'rows%d-shift%d-%s-s%d-wd%g' % c

ALIGN_N = [5, 1027, 4099, 16387]
ALIGN_WHICH = ['p', 'm', 'v', 'g', 'pmvg']

ADVANCE_N = [1, 63, 64, 65, 186, 1000]
ADVANCE_STEPS = [0, 1, 8, 99, 999, 9999, 99999, 2 ** 20]
ADVANCE_BETAS = [(0.9, 0.999), (0.8, 0.99)]
