"""Test infrastructure: float64 reference of the part merge of TPoseHuman.forward (inb_part_network_multiassign.py:229-256) and of its
transpose, per survivor, in every cfg.aggr mode — written out by hand so that every output comes with its conditioning.  Checker
only: plain float64 torch, no import of the product.  The conventions are those of tests/mlp_reference.py (Ref = exact, A, c).

Inputs of merge(aggr, listed, far, vals, pdist), Na survivors x 5 parts:
    listed, far  (Na,5) bool: the (survivor, part) is flagged and carries its own field value / is flagged but so far from the part
                 that it takes the part's constant (the field at zero weights).  Never both.  Neither = unflagged: the reference's
                 zeros (raws / occs start as zeros and only flagged rows are filled, :201-202, :229-234)
    vals         (Na,5,4) the per-part [rgb, occ]; far entries hold the part's constant, unflagged entries anything (never read)
    pdist        (Na,5) part_dist ('dist', 'mindist'; ignored otherwise)
-> Merged(exact (Na,4), A (Na,4), c (Na,), wsel (Na,) int64)
    ''         the part of the FIRST maximum of {listed: occ, far: the constant's occ, unflagged: 0} — the walk starts from part 0
               whatever part 0 is, a later part takes over only with a strictly larger value (occs.argmax, :253-255)
    'mean'     sum over the flagged parts / 5 (raws.mean(dim=1), :236-239)
    'dist'     sum over the flagged parts of value x weight, weights = 1 / (pdist + 1e-5) divided by max(their L2 norm over ALL five
               parts, 1e-12) (F.normalize, :240-244); both constants are the float32 ones the fp32 code adds / clamps with
    'mindist'  the part of the first minimum of pdist, a NaN wins (argmin, :245-251): its value, its constant, or zeros if unflagged
  A = the same expression on magnitudes; c = the number of summands (1 for the two selections).
  wsel = the kernels' code of the result (csrc/pair_lists.h): p = the listed pair of part p, 8 + p = the far constant of part p,
  255 = zeros; the two sums: 0 where any part is flagged, 255 otherwise.

merge_bwd(aggr, listed, far, wsel, pdist, g) with g (Na,4) the gradient w.r.t. the merged value
-> (g_raws (Na,5,4): the gradient of every LISTED (survivor, part) value, zeros elsewhere,
    far_rows: five Ref(exact (4,), A (4,), c) — the sum over the part's far survivors (they share one constant), its magnitudes' sum and
    the number of contributors).
  The selections route by wsel (the forward's choice); the sums weight g by 1 / 5 or by the 'dist' weight (the weights depend on the
  geometry alone: no gradient).  Unflagged parts are zeros without a producer: no gradient."""
import collections

import torch

Ref = collections.namedtuple('Ref', 'exact A c')
Merged = collections.namedtuple('Merged', 'exact A c wsel')
NUM_PARTS = 5
WSEL_FAR, WSEL_NONE, WSEL_MERGED = 8, 255, 0
AGGRS = ('', 'mean', 'dist', 'mindist')
DIST_EPS = float(torch.tensor(1e-5, dtype=torch.float32))             # 1.0 / (part_dist + 1e-5) in float32
NORM_EPS = float(torch.tensor(1e-12, dtype=torch.float32))            # F.normalize's eps in float32


def dist_weights(pdist):
    """(Na,5) -> F.normalize(1.0 / (pdist + 1e-5), dim=-1) in float64."""
    w = 1.0 / (pdist.double() + DIST_EPS)
    return w / (w * w).sum(-1, keepdim=True).sqrt().clamp_min(NORM_EPS)


def first_min(pdist):
    """part_dist.argmin(dim=1): the first minimum, the first NaN if there is one."""
    pd = pdist.double()
    bd, bp = pd[:, 0].clone(), torch.zeros(pd.shape[0], dtype=torch.int64)
    for p in range(1, NUM_PARTS):
        d = pd[:, p]
        take = ~torch.isnan(bd) & ((d < bd) | torch.isnan(d))
        bd, bp = torch.where(take, d, bd), torch.where(take, torch.full_like(bp, p), bp)
    return bp


def first_max(cand):
    """occs.argmax(dim=1): start from part 0, a later part only takes over with a strictly larger value."""
    best, bp = cand[:, 0].clone(), torch.zeros(cand.shape[0], dtype=torch.int64)
    for p in range(1, NUM_PARTS):
        take = cand[:, p] > best
        best, bp = torch.where(take, cand[:, p], best), torch.where(take, torch.full_like(bp, p), bp)
    return bp


def _check(listed, far):
    assert listed.dtype == far.dtype == torch.bool and listed.shape == far.shape and listed.shape[1] == NUM_PARTS
    assert not bool((listed & far).any()), 'a (survivor, part) is both listed and far'


def dense(listed, far, vals):
    """The reference's raws (Na,5,4): zeros where the part is unflagged."""
    return torch.where((listed | far)[..., None], vals.double(), torch.zeros((), dtype=torch.float64))


def select_code(listed, far, part):
    """wsel of the survivor whose merge chose `part` (Na,)."""
    ar = torch.arange(part.shape[0])
    return torch.where(listed[ar, part], part, torch.where(far[ar, part], WSEL_FAR + part, torch.full_like(part, WSEL_NONE)))


def merge(aggr, listed, far, vals, pdist=None):
    _check(listed, far)
    assert aggr in AGGRS, aggr
    raws = dense(listed, far, vals)
    any_ = listed | far
    na = raws.shape[0]
    ar = torch.arange(na)
    if aggr in ('', 'mindist'):
        part = first_max(raws[:, :, 3]) if aggr == '' else first_min(pdist)
        exact = raws[ar, part]
        return Merged(exact, exact.abs(), torch.ones(na, dtype=torch.float64), select_code(listed, far, part))
    wsel = torch.where(any_.any(1), torch.tensor(WSEL_MERGED), torch.tensor(WSEL_NONE))
    c = any_.sum(1).double()
    if aggr == 'mean':
        return Merged(raws.sum(1) / NUM_PARTS, raws.abs().sum(1) / NUM_PARTS, c, wsel)
    w = dist_weights(pdist)[..., None]
    # (an unflagged part is a zero of the reference: it adds nothing whatever its weight; 0 x a NaN / inf weight is NaN there too)
    return Merged((raws * w).sum(1), (raws * w).abs().sum(1), c, wsel)


def merge_bwd(aggr, listed, far, wsel, pdist, g):
    _check(listed, far)
    assert aggr in AGGRS, aggr
    g = g.double()
    na = g.shape[0]
    parts = torch.arange(NUM_PARTS)[None]
    if aggr in ('', 'mindist'):
        wsel = wsel.long()
        assert bool(((wsel < NUM_PARTS) | ((wsel >= WSEL_FAR) & (wsel < WSEL_FAR + NUM_PARTS)) | (wsel == WSEL_NONE)).all())
        to_listed = wsel[:, None] == parts                              # (Na,5)
        to_far = wsel[:, None] == WSEL_FAR + parts
        contrib = g[:, None, :].expand(na, NUM_PARTS, 4)
    else:
        w = torch.full((na, NUM_PARTS), 1.0 / NUM_PARTS, dtype=torch.float64) if aggr == 'mean' else dist_weights(pdist)
        to_listed, to_far = listed, far
        contrib = g[:, None, :] * w[..., None]
    g_raws = torch.where(to_listed[..., None], contrib, torch.zeros((), dtype=torch.float64))
    far_rows = []
    for p in range(NUM_PARTS):
        rows = contrib[to_far[:, p], p]                                 # (n_p,4)
        far_rows.append(Ref(rows.sum(0), rows.abs().sum(0), float(rows.shape[0])))
    return g_raws, far_rows
