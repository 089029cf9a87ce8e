"""Test infrastructure: float64 reference of the BACKWARD (encoder_bwd) and the FORWARD (encoder_fwd, at the end) of the
multi-resolution hash-grid encoder (part_base_embedder.py:106-174 as oracle/nvr_oracle.py:hash_embed restates it), together with
its conditioning.  Checker only: plain vectorised float64 torch, no import of the product.

For points x (n,3), an upstream gradient g_out (n,out_dim), the tables, the bounds and a spec (oracle.embedder_geometry) it returns
per output tensor (g_xyz, g_dense, g_hash) a Ref:
    exact   the gradient
    A       the absolute-sum companion: the same sums with every summand replaced by its absolute value.  Outside the box both
            corners of an axis clip to the same row and the weights (1 - t), t grow and cancel: A is the scale that
            cancellation happens at, so a rounding-error bound is a multiple of A, not of |exact|
    c       the number of summands per element (table rows: how many corner contributions landed on the row; g_xyz: 8 L F + L + 8)
Every reduction mode of the spec is covered: sum + sum_over_features, sum over levels, concatenation; separate_dense or one (L,T,F)
table; include_input on / off.
"""
import collections

import torch

HASH_P1, HASH_P2 = 19349663, 83492791                                  # part_base_embedder.py:132-136 (the x prime is 1)
Ref = collections.namedtuple('Ref', 'exact A c')


def corner_offsets():
    """(8,3) corner offsets 000, 001, ..., 111 (x y z, z fastest; part_base_embedder.py:81-88)."""
    return torch.tensor([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=torch.float32)


def normalise(x, bounds):
    b = bounds.double()
    return (x.double() - b[0]) / (b[1] - b[0])                         # :112


def n_rows(spec):
    """Rows of the flat row space: the dense rows, then T per hashed level (L T for a single table) — invr_grid_row_sums order."""
    return spec['dense_rows'] + (spec['L'] - spec['start_hash']) * spec['T'] if spec['separate_dense'] else spec['L'] * spec['T']


def flat_table(dense, hsh, spec):
    F = spec['F']
    if spec['separate_dense']:
        return torch.cat([dense.double().reshape(-1, F), hsh.double().reshape(-1, F)], 0)
    return hsh.double().reshape(-1, F)


def level_cells(xn, spec, l):
    """-> c0, c1 (n,3) int64 clipped corner cells, t (n,3) offset from c0 (:115-118)."""
    res = int(spec['res'][l])
    f = xn / spec['size'][l].double()
    c0 = f.trunc().clamp(0, res - 1)
    c1 = (f + 1.0).trunc().clamp(0, res - 1)
    return c0.long(), c1.long(), f - c0


def level_rows(c0, c1, spec, l):
    """-> list of 8 (n,) flat row indices of the level's corners."""
    res, T, sh = int(spec['res'][l]), spec['T'], spec['start_hash']
    rows = []
    for k in range(8):
        cx = c1[:, 0] if k & 4 else c0[:, 0]
        cy = c1[:, 1] if k & 2 else c0[:, 1]
        cz = c1[:, 2] if k & 1 else c0[:, 2]
        if l >= sh:
            r = (cx ^ (cy * HASH_P1) ^ (cz * HASH_P2)) % T               # :132-136
            base = spec['dense_rows'] + (l - sh) * T if spec['separate_dense'] else l * T
        else:
            r = cx * (res * res) + cy * res + cz                        # :124-129
            base = int(sum(int(q) ** 3 for q in spec['res'][:l])) if spec['separate_dense'] else l * T
        rows.append(r + base)
    return rows


def encoder_bwd(x, g_out, dense, hsh, bounds, spec, companions=True):
    """-> {'g_xyz': Ref, 'g_dense': Ref or None, 'g_hash': Ref}; with companions False only `exact` is filled (A = c = None)."""
    L, F = spec['L'], spec['F']
    n = x.shape[0]
    go = g_out.double()
    xn = normalise(x, bounds)
    ext = (bounds.double()[1] - bounds.double()[0])
    off = 3 if spec['include_input'] else 0
    rowscalar = spec['sum'] and spec['sum_over_features']
    Fe = 1 if rowscalar else F                                          # distinct gradient columns of a table row
    tab = flat_table(dense, hsh, spec)
    if rowscalar:                                                       # all F features share the level's upstream gradient
        tsum, tabs = tab.sum(1, keepdim=True), tab.abs().sum(1, keepdim=True)
    R = n_rows(spec)
    gt = torch.zeros(R, Fe, dtype=torch.float64)
    gtA = torch.zeros(R, Fe, dtype=torch.float64) if companions else None
    gtc = torch.zeros(R, dtype=torch.float64) if companions else None
    gx = torch.zeros(n, 3, dtype=torch.float64)
    gxA = torch.zeros(n, 3, dtype=torch.float64)
    ones = torch.ones(n, dtype=torch.float64)
    for l in range(L):
        c0, c1, t = level_cells(xn, spec, l)
        rows = level_rows(c0, c1, spec, l)
        if not spec['sum']:
            gl = go[:, off + l * F: off + (l + 1) * F]
        elif spec['sum_over_features']:
            gl = go[:, off + l: off + l + 1]
        else:
            gl = go[:, off: off + F]
        cell = spec['size'][l].double()
        for k in range(8):
            w = [t[:, a] if (k >> (2 - a)) & 1 else 1.0 - t[:, a] for a in range(3)]
            sg = [1.0 if (k >> (2 - a)) & 1 else -1.0 for a in range(3)]
            wk = w[0] * w[1] * w[2]
            gt.index_add_(0, rows[k], wk[:, None] * gl)
            if companions:
                gtA.index_add_(0, rows[k], wk.abs()[:, None] * gl.abs())
                gtc.index_add_(0, rows[k], ones)
            if rowscalar:
                dot, adot = gl[:, 0] * tsum[rows[k], 0], gl[:, 0].abs() * tabs[rows[k], 0]
            else:
                v = tab[rows[k]]
                dot, adot = (gl * v).sum(1), (gl.abs() * v.abs()).sum(1)
            for a in range(3):
                dw = w[(a + 1) % 3] * w[(a + 2) % 3]                   # d w_k / d t_a up to the sign
                gx[:, a] += sg[a] * dw * dot / cell
                if companions:
                    gxA[:, a] += dw.abs() * adot / cell
    if spec['include_input']:
        gx += go[:, :3]
        gxA += go[:, :3].abs()
    gx, gxA = gx / ext, gxA / ext.abs()

    def table(lo, hi, shape):
        if hi <= lo:
            return None
        e = gt[lo:hi].expand(-1, F).reshape(shape).clone()
        if not companions:
            return Ref(e, None, None)
        return Ref(e, gtA[lo:hi].expand(-1, F).reshape(shape).clone(), gtc[lo:hi, None].expand(-1, F).reshape(shape).clone())
    dr = spec['dense_rows'] if spec['separate_dense'] else 0
    return {'g_xyz': Ref(gx, gxA if companions else None, 8 * L * F + L + 8),
            'g_dense': table(0, dr, (dr, F)),
            'g_hash': table(dr, R, tuple(hsh.shape))}


def row_scalars(ref_out, spec):
    """The table gradients of a sum + sum_over_features grid reduced to one scalar per row, invr_grid_row_sums order -> Ref (rows,)."""
    parts = [r for r in (ref_out['g_dense'], ref_out['g_hash']) if r is not None]
    cat = lambda i: torch.cat([p[i].reshape(-1, spec['F'])[:, 0] for p in parts], 0)
    return Ref(cat(0), cat(1), cat(2))


def tie_mask(x, bounds, spec, exempt_faces=False):
    """Cell ties: the cell index is trunc(x_n / cell); a point whose quotient q is within rounding of an integer can land in the
    neighbouring cell in fp32.  -> (n,) bool, True where at some level and axis q lies in (-1.5, res + 0.5) and within
    2^-20 max(|q|, 1) (16 ulp) of an integer.  exempt_faces: coordinates exactly ON a face of the box (x_n == 0.0 or 1.0) are not
    counted (the `faces` cloud, whose ties are its purpose)."""
    xn = normalise(x, bounds)
    drop = torch.zeros(x.shape[0], dtype=torch.bool)
    for l in range(spec['L']):
        res = int(spec['res'][l])
        q = xn / spec['size'][l].double()
        tie = (q > -1.5) & (q < res + 0.5) & ((q - q.round()).abs() <= 2.0 ** -20 * q.abs().clamp(min=1.0))
        if exempt_faces:
            tie &= ~((xn == 0.0) | (xn == 1.0))
        drop |= tie.any(1)
    return drop


# ---- forward --------------------------------------------------------------------------------------------------------------------
def fp32_cells(x, bounds, spec):
    """The reference's own DISCRETE decision, in its own fp32 arithmetic as torch evaluates it on the CPU (:112-118): x_n = (x - b0) /
    (b1 - b0), f = x_n / size_l, trunc(f) and trunc(f + 1), clipped.  Every operation is a correctly rounded IEEE one, so the bits are
    defined without reference to any kernel.  -> [(c0, c1)] per level, (n,3) int64 each.  Where f lies half an ulp below a
    power-of-two integer, f + 1 rounds up and c1 = c0 + 2."""
    b = bounds.float()
    xn = (x.float() - b[0]) / (b[1] - b[0])
    cells = []
    for l in range(spec['L']):
        res = int(spec['res'][l])
        f = xn / spec['size'][l].float()
        cells.append((f.long().clamp(0, res - 1), (f + 1.0).long().clamp(0, res - 1)))
    return cells


_ROW_SUMS = []                                                         # [(dense, hsh, sums, abs sums)]: the last two tables seen


def row_sums64(dense, hsh, spec):
    """Per table row the float64 sum of its F features and of their absolute values, invr_grid_row_sums order -> (rows,), (rows,).
    (Summed from the fp32 tables directly: a 2^20 + 7 table is never copied to float64.)"""
    for d, h, s, a in _ROW_SUMS:
        if d is dense and h is hsh:
            return s, a
    parts = [dense, hsh] if spec['separate_dense'] else [hsh]
    s = torch.cat([p.reshape(-1, spec['F']).sum(1, dtype=torch.float64) for p in parts])
    a = torch.cat([p.reshape(-1, spec['F']).abs().sum(1, dtype=torch.float64) for p in parts])
    _ROW_SUMS.append((dense, hsh, s, a))
    del _ROW_SUMS[:-2]
    return s, a


def encoder_fwd(x, dense, hsh, bounds, spec, cells=None, companions=True):
    """Float64 forward -> Ref(exact, A, c) of out (n,out_dim).  `cells` (fp32_cells): the corner cells are the reference's discrete
    fp32 decision and everything continuous — t = f64 - c0, the weights, the sums — is float64; None: the cells of float64 (the two
    agree on a tie-free cloud).  A = the same sums with |w_k| |table entry|; c (out_dim,) = the number of summands of a column: 8 F for a
    level summed over features, 8 for a concatenated feature, 8 L for a feature summed over levels.  Input columns: exact = the float64
    normalised coordinate, A = |x - b0| / |ext|, c = 1.  The rows a point needs are gathered BEFORE widening to float64."""
    L, F, n = spec['L'], spec['F'], x.shape[0]
    xn = normalise(x, bounds)
    rowscalar = spec['sum'] and spec['sum_over_features']
    if rowscalar:
        rs, rsa = row_sums64(dense, hsh, spec)
    sep, sh, dr = spec['separate_dense'], spec['start_hash'], spec['dense_rows']
    lev, levA = [], []
    for l in range(L):
        if cells is None:
            c0, c1, t = level_cells(xn, spec, l)
        else:
            c0, c1 = cells[l]
            t = xn / spec['size'][l].double() - c0
        rows = level_rows(c0, c1, spec, l)
        src, base = (dense.reshape(-1, F), 0) if sep and l < sh else (hsh.reshape(-1, F), dr)
        o = torch.zeros(n, 1 if rowscalar else F, dtype=torch.float64)
        oA = torch.zeros_like(o)
        for k in range(8):
            w = [t[:, a] if (k >> (2 - a)) & 1 else 1.0 - t[:, a] for a in range(3)]
            wk = (w[0] * w[1] * w[2])[:, None]
            if rowscalar:
                v, va = rs[rows[k]][:, None], rsa[rows[k]][:, None]
            else:
                v = src[rows[k] - base].double()
                va = v.abs()
            o += wk * v
            if companions:
                oA += wk.abs() * va
        lev.append(o)
        levA.append(oA)
    if not spec['sum'] or rowscalar:
        e, A, c = torch.cat(lev, 1), torch.cat(levA, 1), torch.full((len(lev) * lev[0].shape[1],), 8.0 * (F if rowscalar else 1))
    else:
        e, A, c = sum(lev), sum(levA), torch.full((F,), 8.0 * L)
    if spec['include_input']:
        b = bounds.double()
        e = torch.cat([xn, e], 1)
        A = torch.cat([(x.double() - b[0]).abs() / (b[1] - b[0]).abs(), A], 1)
        c = torch.cat([torch.ones(3), c])
    assert e.shape == (n, spec['out_dim'])
    return Ref(e, A if companions else None, c.double() if companions else None)
