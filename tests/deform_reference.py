"""Test infrastructure: float64 reference of the residual deformer resd = 0.05 tanh(MLP(grid(uv(x), frame_dim))) (uv_deformer.py:31-38:
UV-volume trilinear -> (u, v, t) -> 8-level F = 2 concat grid with its input -> 19-32-32-3 Softplus MLP) and of its BACKWARD with
respect to the parameters, written out by hand — no autograd — so that every output comes with its conditioning.  Checker only: plain
float64 torch on oracle.nvr_oracle.sample_volume and tests/grid_reference.py, no import of the product.  The canonical points carry no
gradient (the warp is gradient-free in the reference, inb_part_network_multiassign.py:87-90).

deformer(pts, g_resd, P, scene, spec) returns per output a Ref (exact, A, c) in the convention of tests/mlp_reference.py: A = the same
nested expression with every weight, derivative factor, activation, interpolation weight and upstream gradient replaced by its
magnitude, c = the number of summands along the chain from g_resd (`n` for the parameter gradients, the corner count of a row + the
chain for the table gradients — deformer() returns the corner count, chain_c adds the chain).  Derivative factors are formed from
the pre-activation: softplus' = sigmoid(z), tanh' = 1 / cosh(z)^2.  Their companions carry the factor's own conditioning,
A(f(z)) = |f'(z)| A(z) + |f(z)| — the rule tests/mlp_reference.py applies to the forward activations: on the `outside` cloud every
entry is clamped to a corner of the volume, no input perturbation moves anything, and the rounding of the 32-term sums z2, z3 in
front of a factor would otherwise have no scale to be measured against.

Outputs, per entry: resd (n,3), uvt (n,3) = [u, v, frame_dim], a0 (n,19) = the grid's output [normalised uvt, 16 features], a1, a2
(n,32) the inputs of layers 2 and 3, gz1, gz2 (n,32), gz3 (n,3) the gradients w.r.t. the layers' pre-activations, gfeat (n,19) the
gradient w.r.t. the grid's output.  Parameter gradients: dW0 (32,19), dW1 (32,32), dW2 (3,32), db0, db1, db2, g_dense, g_hash.
P: dict W [3], b [3], dense (rows,2) or None, hash (n_hash,T,2); scene: dict tuv (Dx,Dy,Dz,2), tbounds (2,3), frame_dim (scalar
tensor); spec: oracle.nvr_oracle.embedder_geometry(...) of the grid, its bbox the grid's bounds."""
import torch

from oracle import nvr_oracle as O
from tests import grid_reference as GR
from tests.mlp_reference import Ref, dsigmoid, dsoftplus, softplus, ulp32

ENTRY_KEYS = ('uvt', 'a0', 'a1', 'a2', 'gz1', 'gz2', 'gz3', 'gfeat')
PARAM_KEYS = ('dW0', 'db0', 'dW1', 'db1', 'dW2', 'db2', 'g_dense', 'g_hash')
C_GZ3, C_GZ2, C_GZ1, C_GFEAT = 4.0, 4.0 + 3 + 1, 4.0 + 3 + 1 + 32 + 1, 4.0 + 3 + 1 + 32 + 1 + 32


def chain_c(ref):
    """A table gradient's Ref with the chain from g_resd to gfeat added to the corner count of every row that is reached."""
    return Ref(ref.exact, ref.A, ref.c + C_GFEAT * (ref.c > 0))


def grid_geometry(uvt, spec):
    """uvt (n,3) float64 -> (xn (n,3), rows (L,8,n) int64 flat table rows, w (L,8,n) trilinear weights) of every level's eight corners
    (GR.level_cells / GR.level_rows, corner k = x y z bits, z fastest)."""
    xn = GR.normalise(uvt, spec['bbox'])
    rows, ws = [], []
    for l in range(spec['L']):
        c0, c1, t = GR.level_cells(xn, spec, l)
        rows.append(torch.stack(GR.level_rows(c0, c1, spec, l), 0))
        ax = [torch.stack([1.0 - t[:, a], t[:, a]], 0) for a in range(3)]
        ws.append(torch.stack([ax[0][(k >> 2) & 1] * ax[1][(k >> 1) & 1] * ax[2][k & 1] for k in range(8)], 0))
    return xn, torch.stack(rows, 0), torch.stack(ws, 0)


def grid_forward(geo, dense, hsh, spec, companions=True):
    """The concat grid with its input (part_base_embedder.py:106-174, sum False, include_input) -> (feat (n, 3 + L F), A or None)."""
    L, F = spec['L'], spec['F']
    assert not spec['sum'] and spec['include_input']
    xn, rows, w = geo
    n = xn.shape[0]
    tab = GR.flat_table(dense, hsh, spec)[rows.reshape(-1)].reshape(L, 8, n, F)
    val = (w[..., None] * tab).sum(1).permute(1, 0, 2).reshape(n, L * F)
    if not companions:
        return torch.cat([xn, val], -1), None
    A = (w.abs()[..., None] * tab.abs()).sum(1).permute(1, 0, 2).reshape(n, L * F)
    return torch.cat([xn, val], -1), torch.cat([xn.abs(), A], -1)


def grid_backward(geo, gfeat, Agf, dense, hsh, spec):
    """Table gradients of the concat grid for the upstream gfeat (n, 3 + L F) (the scatter of GR.encoder_bwd without its g_xyz):
    -> {'g_dense', 'g_hash'} of Ref; Agf None: exact only.  c = how many corner contributions landed on the row."""
    L, F = spec['L'], spec['F']
    xn, rows, w = geo
    n = xn.shape[0]
    R = GR.n_rows(spec)
    idx = rows.reshape(-1)

    def scatter(wt, gl):
        g = gl[:, 3:].reshape(n, L, F).permute(1, 0, 2)[:, None]               # (L,1,n,F)
        return torch.zeros(R, F, dtype=torch.float64).index_add_(0, idx, (wt[..., None] * g).reshape(-1, F))
    gt = scatter(w, gfeat)
    comp = Agf is not None
    if comp:
        gtA = scatter(w.abs(), Agf.abs())
        gtc = torch.zeros(R, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
    dr = spec['dense_rows'] if spec['separate_dense'] else 0

    def table(lo, hi, shape):
        if hi <= lo:
            return None
        if not comp:
            return Ref(gt[lo:hi].reshape(shape).clone(), None, None)
        return Ref(gt[lo:hi].reshape(shape).clone(), gtA[lo:hi].reshape(shape).clone(), gtc[lo:hi, None].expand(-1, F).reshape(shape).clone())
    return {'g_dense': table(0, dr, (dr, F)), 'g_hash': table(dr, R, tuple(hsh.shape))}


def deformer(pts, g_resd, P, scene, spec, companions=True, softplus_sign=None, geometry=None, backward=True):
    """pts, g_resd (n,3) -> dict of Ref (companions False: A = c = None everywhere).  geometry: the 'geometry' entry of an earlier
    result for the same pts (the UV sample and the grid's corner rows / weights are not formed again).  softplus_sign (dict 'h1', 'h2' -> +-1 tensors
    (n,32)): the value-only perturbation of tests/deform_cases.py, noise class (c) — each forward Softplus output moved by that sign
    times max(1 fp32 ulp of itself, 1.5e-7); the derivative factors stay computed from z.  backward False: the forward entries alone
    (resd, uvt, a0, a1, a2, z, geometry — the same statements; g_resd is not read)."""
    comp = companions
    d = lambda t: t.detach().double()
    W, b = [d(w) for w in P['W']], [d(x) for x in P['b']]
    dense, hsh = (None if P['dense'] is None else d(P['dense'])), d(P['hash'])
    pts, g = d(pts), d(g_resd)
    n = pts.shape[0]
    tuv, tb, fd = d(scene['tuv']), d(scene['tbounds']), d(scene['frame_dim']).reshape(1, 1)
    ab = (lambda t: t.abs()) if comp else (lambda t: None)

    def act(name, z):
        h = softplus(z)
        if softplus_sign is not None:
            h = h + softplus_sign[name] * torch.maximum(ulp32(h), torch.full_like(h, 1.5e-7))
        return h

    def lin(x, Wl, bl):
        return x @ Wl.t() + bl, (x.abs() @ Wl.abs().t() + bl.abs()) if comp else None

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    if geometry is not None:
        uvt, A_uvt, geo = geometry
    else:
        if n:
            uv = O.sample_volume(pts, tuv, tb)
            A_uv = O.sample_volume(pts, tuv.abs(), tb) if comp else None     # (border padding: every interpolation weight lies in [0, 1])
        else:
            uv = torch.zeros(0, 2, dtype=torch.float64)
            A_uv = uv.clone() if comp else None
        uvt = torch.cat([uv, fd.expand(n, 1)], -1)
        A_uvt = torch.cat([A_uv, fd.abs().expand(n, 1)], -1) if comp else None
        geo = grid_geometry(uvt, spec)
    feat, A_feat = grid_forward(geo, dense, hsh, spec, comp)
    z1, Az1 = lin(feat, W[0], b[0])
    h1 = act('h1', z1)
    z2, Az2 = lin(h1, W[1], b[1])
    h2 = act('h2', z2)
    z3, Az3 = lin(h2, W[2], b[2])
    th = torch.tanh(z3)
    sech2 = 1.0 / torch.cosh(z3) ** 2
    resd = 0.05 * th
    fwd = dict(resd=Ref(resd, (0.05 * (sech2 * Az3 + th.abs())) if comp else None, 35.0),
               uvt=Ref(uvt, A_uvt, 12.0),
               a0=Ref(feat, A_feat, 12.0),
               a1=Ref(h1, (dsoftplus(z1) * Az1 + h1.abs()) if comp else None, 21.0),
               a2=Ref(h2, (dsoftplus(z2) * Az2 + h2.abs()) if comp else None, 34.0),
               z=dict(z1=z1, z2=z2, z3=z3), geometry=(uvt, A_uvt, geo))
    if not backward:
        return fwd
    # ---- backward ----------------------------------------------------------------------------------------------------------------
    # a derivative factor is itself computed from a pre-activation that fp32 forms as a sum: its companion follows the forward rule
    # A(f(z)) = |f'(z)| A(z) + |f(z)| with f the factor (sigmoid' = sigmoid(z) sigmoid(-z), (1 / cosh^2)' = -2 tanh / cosh^2)
    mm = lambda x, Ax, Wl: (x @ Wl, (Ax @ Wl.abs()) if comp else None)
    mul = lambda x, Ax, f, Af: (x * f, (Ax * Af) if comp else None)
    fac = lambda z, Az: (dsoftplus(z), (dsigmoid(z) * Az + dsoftplus(z)) if comp else None)
    gz3, A3 = mul(g, ab(g), 0.05 * sech2, (0.05 * (2.0 * th.abs() * sech2 * Az3 + sech2)) if comp else None)
    gz2, A2 = mul(*mm(gz3, A3, W[2]), *fac(z2, Az2))
    gz1, A1 = mul(*mm(gz2, A2, W[1]), *fac(z1, Az1))
    gfeat, Agf = mm(gz1, A1, W[0])
    out = dict(fwd, gz3=Ref(gz3, A3, C_GZ3), gz2=Ref(gz2, A2, C_GZ2), gz1=Ref(gz1, A1, C_GZ1), gfeat=Ref(gfeat, Agf, C_GFEAT))
    nn = float(n) if comp else None
    for l, (gz, Ag, ain) in enumerate(((gz1, A1, feat), (gz2, A2, h1), (gz3, A3, h2))):
        out['dW%d' % l] = Ref(gz.t() @ ain, (Ag.t() @ ain.abs()) if comp else None, nn)
        out['db%d' % l] = Ref(gz.sum(0), Ag.sum(0) if comp else None, nn)
    # grid^T: the table gradients of the upstream gfeat; the companion is the same scatter of gfeat's own companion
    tg = grid_backward(geo, gfeat, Agf, dense, hsh, spec)
    for k in ('g_dense', 'g_hash'):
        out[k] = tg[k]                                                  # (c: the corner count alone, it adds up over chunks; see chain_c)
    return out
