"""Test infrastructure: float64 reference of the two MLPs of a part after the encoder (part_base_network.py:44-63: occ 19-64-17,
rgb 70-64(-64)-3, direction encoding with 4 frequencies, 8 latent values) and of their BACKWARD, written out by hand — no autograd —
so that every output comes with its conditioning.  Checker only: plain float64 torch, no import of the product.

part_mlps(emb, dirs, P, g_raw) returns per output a Ref:
    exact   the value
    A       the absolute-value companion.  Backward outputs: the same nested expression with every weight, derivative factor,
            activation and upstream gradient replaced by its magnitude (the companions chain: A(W^T gz) = |W|^T A(gz)).  Forward
            outputs: the layer's own sum, A(z) = |a_in| |W|^T + |b| on the exact input, carried through the activation as
            f'(z) A(z) + |f(z)|.  What the errors of EARLIER forward layers do to an output is not in A: that is the noise of
            tests/mlp_cases.py
    c       the number of summands: forward the layer's fan-in + 1 (+ 1 for an activation); backward the layer widths summed along
            the chain from g_raw; `n` for the parameter gradients; n + the chain for the latent gradient
Derivative factors are formed from the pre-activation z, never from the activation.  Softplus is torch.nn.Softplus(beta=1,
threshold=20) in value and derivative (z > 20: z and 1).

Outputs: raw (n,4) = [sigmoid rgb, occ]; g_emb (n,19); g_latent (8); gz[l] (n,O_l) and a[l] (n,I_l) for l = 0 occ layer 1, 1 occ layer
2, 2 rgb layer 1, 3 rgb layer 2 (None for a 2-linear colour net), 4 rgb head — a[2] in the weight's column order (slot_a2 / unslot_a2
convert to and from the kernel's k-slot order); dW[l], db[l].
"""
import collections

import torch

Ref = collections.namedtuple('Ref', 'exact A c')
N_FREQ, N_EMB, N_FEAT, N_LAT = 4, 19, 16, 8
OUT_DIMS, IN_DIMS = (64, 17, 64, 64, 3), (19, 64, 70, 64, 64)


def rgb1_col(s, g):
    """csrc/mlp_common.h rgb1_col: the input column of rgb layer 1 that k-slot (step s, lane group g) holds; -1 = zero padding.
    rgb input = [emb 0..18 | d 19..21, sin(2^k d), cos(2^k d) 22..45 | feat 46..61 | latent 62..69]."""
    if s < 5:
        e = 4 * s + g
        return e if e < 19 else -1
    if s < 11:
        u = s - 5
        return 19 + 3 + g * 6 + (u & 1) * 3 + (u >> 1)
    if s < 14:
        e = 4 * (s - 11) + g
        return 19 + e if e < 3 else (62 + (e - 3) if e < 11 else -1)
    return 46 + 4 * g + (s - 14)


SLOT_COL = [rgb1_col(j >> 2, j & 3) for j in range(72)]           # k-slot j = 4 s + g -> weight column
assert sorted(c for c in SLOT_COL if c >= 0) == list(range(70))
PAD_SLOTS = [j for j in range(72) if SLOT_COL[j] < 0]


def slot_a2(x70):
    """(n,70) in weight-column order -> (n,72) in k-slot order, padding slots 0."""
    out = x70.new_zeros(x70.shape[0], 72)
    for j, c in enumerate(SLOT_COL):
        if c >= 0:
            out[:, j] = x70[:, c]
    return out


def unslot_a2(a72):
    """(n,72) k-slot order -> (n,70) weight-column order (the padding slots are dropped)."""
    out = a72.new_zeros(a72.shape[0], 70)
    for j, c in enumerate(SLOT_COL):
        if c >= 0:
            out[:, c] = a72[:, j]
    return out


def softplus(z):
    return torch.where(z > 20.0, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0))))


def dsoftplus(z):
    return torch.where(z > 20.0, torch.ones_like(z), torch.sigmoid(z))


def dsigmoid(z):
    return torch.sigmoid(z) * torch.sigmoid(-z)                    # (not s (1 - s): 1 - s cancels for z >> 0)


def ulp32(x):
    """One float32 unit in the last place of |x| (normal range)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def as_params(P):
    """P: dict occ_w [W0 (64,19), W1 (17,64)], occ_b, rgb_w [W0 (64,70), (W1 (64,64)), Wout (3,64)], rgb_b, latent (8,) -> float64."""
    d = lambda t: t.detach().double()
    return dict(occ_w=[d(w) for w in P['occ_w']], occ_b=[d(b) for b in P['occ_b']], rgb_w=[d(w) for w in P['rgb_w']],
                rgb_b=[d(b) for b in P['rgb_b']], latent=d(P['latent']).reshape(-1))


def part_mlps(emb, dirs, P, g_raw, companions=True, sincos_off=None, softplus_sign=None):
    """emb (n,19), dirs (n,3), g_raw (n,4) -> dict of Ref (companions False: A = None everywhere, half the work).
    The two value-only perturbations of tests/mlp_cases.py (noise class c): sincos_off (n,24) is added to the sin / cos features,
    softplus_sign (dict name -> +-1 tensor, names 'occ1', 'rgb1', 'rgb2', 'lg') moves each forward Softplus output by that sign times
    max(1 fp32 ulp of itself, 1.5e-7).  The derivative factors stay computed from z."""
    P = as_params(P)
    emb, dirs, g_raw = emb.double(), dirs.double(), g_raw.double()
    n = emb.shape[0]
    three = len(P['rgb_w']) == 3
    comp = companions

    def act(name, z):
        h = softplus(z)
        if softplus_sign is not None:
            h = h + softplus_sign[name] * torch.maximum(ulp32(h), torch.full_like(h, 1.5e-7))
        return h

    def lin(x, W, b):                                               # -> z, A(z)
        return x @ W.t() + b, (x.abs() @ W.abs().t() + b.abs()) if comp else None

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    Wo1, Wo2 = P['occ_w']
    z1, Az1 = lin(emb, Wo1, P['occ_b'][0])
    h1 = act('occ1', z1)
    z2, Az2 = lin(h1, Wo2, P['occ_b'][1])
    lg, feat = z2[:, 0], z2[:, 1:]
    s_lg = act('lg', lg)
    occ = -torch.expm1(-s_lg)
    d_occ = torch.exp(-softplus(lg)) * dsoftplus(lg)               # d occ / d lg, from z
    pe = [dirs]
    for k in range(N_FREQ):
        pe += [torch.sin(dirs * 2.0 ** k), torch.cos(dirs * 2.0 ** k)]
    sc = torch.cat(pe[1:], -1)
    if sincos_off is not None:
        sc = sc + sincos_off
    x = torch.cat([emb, dirs, sc, feat, P['latent'][None].expand(n, -1)], -1)
    Wr1 = P['rgb_w'][0]
    zr1, Azr1 = lin(x, Wr1, P['rgb_b'][0])
    hr1 = act('rgb1', zr1)
    if three:
        Wr2 = P['rgb_w'][1]
        zr2, Azr2 = lin(hr1, Wr2, P['rgb_b'][1])
        hl, zl = act('rgb2', zr2), zr2
    else:
        hl, zl = hr1, zr1
    Wout = P['rgb_w'][-1]
    zo, Azo = lin(hl, Wout, P['rgb_b'][-1])
    rgb = torch.sigmoid(zo)
    raw = torch.cat([rgb, occ[:, None]], -1)

    def A_act(h, dz, Az):
        return (dz * Az + h.abs()) if comp else None

    A_raw = torch.cat([dsigmoid(zo) * Azo + rgb, (d_occ * Az2[:, 0] + occ)[:, None]], -1) if comp else None
    A_x = None
    if comp:
        A_x = x.abs().clone()
        A_x[:, 46:62] = Az2[:, 1:]
    a = [Ref(emb, emb.abs() if comp else None, 1.0), Ref(h1, A_act(h1, dsoftplus(z1), Az1), 21.0), Ref(x, A_x, 66.0),
         Ref(hr1, A_act(hr1, dsoftplus(zr1), Azr1), 72.0) if three else None,
         Ref(hl, A_act(hl, dsoftplus(zl), Azr2 if three else Azr1), 66.0 if three else 72.0)]

    # ---- backward (gradient, companion) pairs; c accumulates the widths along the chain --------------------------------------------
    ab = (lambda t: t.abs()) if comp else (lambda t: None)
    mm = lambda g, Ag, W: (g @ W, (Ag @ W.abs()) if comp else None)
    mul = lambda g, Ag, f: (g * f, (Ag * f.abs()) if comp else None)
    go, Ago = mul(g_raw[:, :3], ab(g_raw[:, :3]), dsigmoid(zo))
    c_go = 2.0
    g_lg, Aglg = mul(g_raw[:, 3], ab(g_raw[:, 3]), d_occ)
    gz, c = [None] * 5, [None] * 5
    gz[4], c[4] = (go, Ago), c_go
    g_h, A_h = mm(go, Ago, Wout)
    cc = c_go + 3
    if three:
        gz[3], c[3] = mul(g_h, A_h, dsoftplus(zr2)), cc + 1
        g_h, A_h = mm(*gz[3], Wr2)
        cc = c[3] + 64
    gz[2], c[2] = mul(g_h, A_h, dsoftplus(zr1)), cc + 1
    g_x, A_gx = mm(*gz[2], Wr1)
    c_x = c[2] + 64
    g_feat, A_gfeat = g_x[:, 46:62], (A_gx[:, 46:62] if comp else None)
    gz[1] = (torch.cat([g_lg[:, None], g_feat], -1), torch.cat([Aglg[:, None], A_gfeat], -1) if comp else None)
    c[1] = torch.cat([torch.full((1,), 2.0, dtype=torch.float64), torch.full((16,), c_x, dtype=torch.float64)])[None]
    g_h1, A_gh1 = mm(*gz[1], Wo2)
    gz[0], c[0] = mul(g_h1, A_gh1, dsoftplus(z1)), c_x + 17 + 1
    g_e, A_ge = mm(*gz[0], Wo1)
    g_emb = Ref(g_e + g_x[:, :19], (A_ge + A_gx[:, :19]) if comp else None, c[0] + 64 + c_x)
    g_lat = Ref(g_x[:, 62:70].sum(0), A_gx[:, 62:70].sum(0) if comp else None, n + c_x)
    dW, db, gzr = [None] * 5, [None] * 5, [None] * 5
    for l in range(5):
        if gz[l] is None:
            continue
        g, Ag = gz[l]
        gzr[l] = Ref(g, Ag, c[l])
        ain = a[l].exact
        dW[l] = Ref(g.t() @ ain, (Ag.t() @ ain.abs()) if comp else None, float(n))
        db[l] = Ref(g.sum(0), Ag.sum(0) if comp else None, float(n))
    return dict(raw=Ref(raw, A_raw, 66.0), g_emb=g_emb, g_latent=g_lat, gz=gzr, a=a, dW=dW, db=db,
                z=dict(occ1=z1, rgb1=zr1, rgb2=zr2 if three else None, lg=lg, zo=zo))
