"""CPU: the float64 reference of the part merge (tests/merge_reference.py) against torch ops written straight from the reference's lines
(inb_part_network_multiassign.py:229-256: raws.mean(1), F.normalize, argmin, argmax, gather on a zero-initialised (Na,5,4) tensor) and
its transpose against float64 autograd of that form, on synthetic survivors that hold every case the rule distinguishes."""
import pytest
import torch
import torch.nn.functional as F

from tests import merge_reference as MG

NAN, INF = float('nan'), float('inf')
DENORM = 2.0 ** -140


def synthetic(seed=0, n_random=400):
    """-> listed, far (Na,5) bool, vals (Na,5,4) float32, pdist (Na,5) float32, g (Na,4) float32: hand-made rows first, random ones after."""
    g = torch.Generator().manual_seed(seed)
    const = torch.rand(5, 4, generator=g)                                  # the parts' far constants
    rows = []          # (flags per part: 0 unflagged / 1 listed / 2 far, occ per part or None, pdist per part or None)
    rows += [((1, 1, 0, 0, 0), (0.5, 0.5, 0, 0, 0), None)]                  # occupancy tie of two listed parts: the first wins
    rows += [((0, 1, 1, 0, 0), (0, 0.7, 0.7, 0, 0), None)]                  # tie behind an unflagged part 0
    rows += [((0, 1, 0, 1, 0), (0, 0.0, 0, 0.0, 0), None)]                  # tie at 0 with part 0 unflagged: part 0's zeros win
    rows += [((1, 1, 1, 1, 1), (0.0, 0.0, 0.0, 0.0, 0.0), None)]            # tie at 0, all listed: part 0's pair wins
    rows += [((0, 0, 0, 0, 0), None, None)] * 3                             # no flagged part
    rows += [((2, 0, 0, 0, 0), None, None), ((0, 0, 2, 0, 2), None, None), ((2, 2, 2, 2, 2), None, None)]      # far only
    rows += [((1, 1, 1, 1, 1), None, None)] * 3                             # all five listed
    rows += [((1, 2, 0, 1, 2), None, None)] * 3
    rows += [((1, 0, 1, 0, 1), None, (0.3, 0.1, 0.1, 0.2, 0.1))]            # pdist tie: the first minimum (an unflagged part)
    rows += [((1, 1, 1, 0, 2), None, (0.2, 0.2, 0.2, 0.2, 0.2))]            # all equal
    rows += [((1, 1, 0, 2, 1), None, (0.0, 0.0, 0.5, 0.1, 0.2))]            # zeros
    rows += [((0, 1, 1, 2, 1), None, (0.1, DENORM, 0.0, DENORM, 0.3))]      # denormals and a zero
    rows += [((1, 1, 2, 0, 1), None, (DENORM, DENORM, DENORM, DENORM, DENORM))]
    rows += [((1, 1, 1, 1, 0), None, (0.1, NAN, 0.05, 0.2, 0.3))]           # a NaN wins the minimum
    rows += [((1, 0, 1, 1, 2), None, (0.1, 0.3, NAN, NAN, 0.01))]           # the first NaN
    rows += [((1, 1, 2, 1, 0), None, (INF, 0.2, 0.1, INF, 0.4))]            # +inf: weight 0
    rows += [((1, 2, 1, 0, 1), None, (INF, INF, INF, INF, INF))]            # all weights 0: the norm is clamped
    rows += [(tuple(2 if q == p else 0 for q in range(5)), None, None) for p in range(5)]      # one far part alone, every part
    for _ in range(n_random):
        rows.append((tuple(int(x) for x in torch.randint(0, 3, (5,), generator=g)), None, None))
    na = len(rows)
    fl = torch.tensor([r[0] for r in rows])
    listed, far = fl == 1, fl == 2
    vals = torch.rand(na, 5, 4, generator=g)
    vals = torch.where(far[..., None], const[None].expand(na, 5, 4), vals)
    pdist = torch.rand(na, 5, generator=g) * 0.5
    for i, (_, occ, pd) in enumerate(rows):
        if occ is not None:
            vals[i, :, 3] = torch.tensor(occ)
        if pd is not None:
            pdist[i] = torch.tensor(pd)
    vals = torch.where((listed | far)[..., None], vals, torch.full_like(vals, NAN))      # unflagged entries are never read
    return listed, far, vals, pdist, torch.randn(na, 4, generator=g)


def direct(aggr, raws, pdist):
    """The reference's lines on its dense raws (Na,5,4) (occs = raws[..., 3:]) -> raw (Na,4), the chosen part or None."""
    n = raws.shape[0]
    occs = raws[..., 3:]
    if aggr == 'mean':
        return raws.mean(dim=1), None
    if aggr == 'dist':
        inv = F.normalize(1.0 / (pdist + MG.DIST_EPS), dim=-1, eps=MG.NORM_EPS)
        return torch.sum(raws * inv[..., None], dim=1), None
    sel = pdist[:, :, None].argmin(dim=1) if aggr == 'mindist' else occs.argmax(dim=1)
    return torch.gather(raws, 1, sel.reshape(n, 1, 1).expand(n, 1, 4))[:, 0, :], sel.reshape(n)


@pytest.fixture(scope='module')
def syn():
    return synthetic()


def test_synthetic_rows_hold_every_case(syn):
    listed, far, vals, pdist, _ = syn
    any_ = listed | far
    assert not bool((listed & far).any())
    assert int((~any_.any(1)).sum()) >= 3 and int((far.any(1) & ~listed.any(1)).sum()) >= 3 and int(listed.all(1).sum()) >= 3
    assert bool(torch.isnan(pdist).any()) and bool(torch.isinf(pdist).any()) and bool((pdist == 0).any())
    assert bool(((pdist > 0) & (pdist < 2.0 ** -126)).any())
    assert bool(torch.isnan(vals[~any_]).all())


@pytest.mark.parametrize('aggr', MG.AGGRS, ids=[a or 'max' for a in MG.AGGRS])
def test_merge_vs_reference_lines(syn, aggr):
    listed, far, vals, pdist, _ = syn
    m = MG.merge(aggr, listed, far, vals, pdist)
    raws = MG.dense(listed, far, vals)
    want, sel = direct(aggr, raws, pdist.double())
    assert m.exact.dtype == torch.float64 and m.exact.shape == (listed.shape[0], 4)
    if aggr in ('', 'mindist'):
        assert torch.equal(m.exact, want)
        ar = torch.arange(listed.shape[0])
        code = torch.where(listed[ar, sel], sel, torch.where(far[ar, sel], 8 + sel, torch.full_like(sel, 255)))
        assert torch.equal(m.wsel, code)
        assert torch.equal(m.A, want.abs()) and bool((m.c == 1).all())
        assert bool((m.exact[m.wsel == 255] == 0).all())
        assert len(set(m.wsel.tolist())) >= 10                           # listed, far and none codes all occur
    else:
        nan = torch.isnan(want)
        assert torch.equal(nan, torch.isnan(m.exact))
        assert bool(((m.exact - want).abs()[~nan] <= 1e-14 * m.A[~nan]).all())
        assert torch.equal(m.wsel, torch.where((listed | far).any(1), torch.tensor(0), torch.tensor(255)))
        assert torch.equal(m.c, (listed | far).sum(1).double())
        assert bool((m.A[~nan] >= m.exact.abs()[~nan] - 1e-300).all())
        assert bool((m.A[~(listed | far).any(1)] == 0).all())
    if aggr != 'dist':
        assert not bool(torch.isnan(m.exact).any())


def test_hand_made_rows(syn):
    listed, far, vals, pdist, _ = syn
    m = MG.merge('', listed, far, vals, pdist)
    assert m.wsel[:4].tolist() == [0, 1, 255, 0]
    assert m.wsel[4:7].tolist() == [255] * 3 and m.wsel[7:10].tolist() == [8, 10, 8 + int(vals[9, :, 3].argmax())]
    d = MG.merge('mindist', listed, far, vals, pdist)
    assert d.wsel[16:25].tolist() == [255, 0, 0, 2, 0, 1, 2, 8 + 2, 0]
    w = MG.dist_weights(pdist[24:25])
    assert torch.equal(w, torch.zeros(1, 5, dtype=torch.float64))        # all +inf: 0 / max(0, eps)
    assert bool((MG.merge('dist', listed, far, vals, pdist).exact[24] == 0).all())


@pytest.mark.parametrize('aggr', MG.AGGRS, ids=[a or 'max' for a in MG.AGGRS])
def test_merge_bwd_vs_autograd(syn, aggr):
    listed, far, vals, pdist, g = syn
    m = MG.merge(aggr, listed, far, vals, pdist)
    g_raws, far_rows = MG.merge_bwd(aggr, listed, far, m.wsel, pdist, g)
    raws = MG.dense(listed, far, vals).requires_grad_(True)
    out, _ = direct(aggr, raws, pdist.double())
    out.backward(g.double())
    gr = raws.grad                                                        # (Na,5,4): also for the zeros, which have no producer
    nan = torch.isnan(gr)
    assert torch.equal(torch.isnan(g_raws)[listed], nan[listed])
    ok = ~nan
    scale = g.double().abs()[:, None, :].expand_as(gr)                  # (every weight is at most 1)
    at = listed[..., None].expand_as(gr) & ok
    assert bool(((g_raws - gr).abs()[at] <= 1e-14 * scale[at]).all())
    assert bool((g_raws[~listed] == 0).all())
    n_far = 0
    for p in range(5):
        rows = gr[far[:, p], p]
        want = rows.sum(0)
        r = far_rows[p]
        if aggr in ('', 'mindist'):
            assert r.c == float((m.wsel == 8 + p).sum())
        else:
            assert r.c == float(far[:, p].sum())
        nn = torch.isnan(want)
        assert torch.equal(nn, torch.isnan(r.exact))
        assert bool(((r.exact - want).abs()[~nn] <= 1e-13 * r.A[~nn]).all())
        assert bool((r.A[~nn] >= r.exact.abs()[~nn]).all())
        n_far += r.c
    assert n_far > 10
