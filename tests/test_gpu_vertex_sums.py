"""GPU: the de-hashed vertex tables of the row-sum encoder kernels (include/invr_vertex.h: invr_grid_vertex_sums; csrc/k_encode.hip:
k_vertex_sums and the vertex-table route of level_rowsum).

A hashed level's value at vertex (cx, cy, cz) is row_sums[level base + hash(cx, cy, cz) mod T]; the builder writes it into a dense
(res^3,) table, and the encoder then reads the level as an ordinary dense level.  Two statements, both bit for bit:
  1. the builder: every entry of every table is the row-sum entry that a NumPy restatement of the hash (tests/grid_reference.py: the
     primes, the 64-bit product, the modulo) names; the two pad floats are zero; nothing is written behind them; a level above the cap
     has offset -1; cap 0 gives length 0;
  2. the encoder with the tables on equals the encoder with the tables off in all 19 columns — kernel 0 (k_part_encode_rs_xcd),
     kernel 2 (k_part_encode_rs) and one five-part launch — for three caps per family: none of the hashed levels, some, all.
The `ties` cloud carries the points with c1 - c0 == 2 on an axis of a hashed level: with a table that is the dense route's reload of
a far second z corner, and corners two apart in x / y.  Families: part-t9 (T 521, the fp64 modulo), part-small (T 4099, the 32-bit
modulo), part-prod (T 2^18 + 3, the one-round modulo under the x-delta fold; only its first hashed level gets a table).

tests/test_hostsim_vertex_sums_cpu.py runs the same bodies on the CPU wave machine (DEV switched to 'cpu', ALL lowered)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import encoder_cases as EC       # noqa: E402  (checker only)
from tests import grid_reference as GR      # noqa: E402  (checker only)
from invr import _abi, params               # noqa: E402

DEV = 'cuda:0'
MARK = 12345.0                                # where nothing may be written
FAMILIES = ('part-t9', 'part-small', 'part-prod')
ALL = 2 ** 24                                 # the ABI's limit: every hashed level of part-t9 / part-small fits (res 251: 15.8 M vertices)
CLOUDS = ('ties', 'faces', 'far', 'wrap', 'uniform')
SIZES = (1, 65, 257, 1000)


def caps_of(tag):
    """-> {'none', 'some', 'all'}: a cap below the first hashed level, one that takes some hashed levels, and every level that fits
    under ALL — part-prod: its first hashed level only (the others are 0.86 M .. 15.6 M vertices each)."""
    spec = EC.make_spec(tag)
    sh, cnt = spec['start_hash'], [int(r) ** 3 for r in spec['res']]
    if tag == 'part-prod':
        return {'none': cnt[sh] - 1, 'some': cnt[sh], 'all': cnt[sh + 1] - 1}          # ('all' here: still the first level alone, a cap between two levels)
    return {'none': cnt[sh] - 1, 'some': cnt[sh + 2], 'all': ALL}


def expected_layout(spec, cap):
    """The layout rule restated from the oracle's geometry alone -> (offset per level, floats)."""
    off, total = [], 0
    for l, r in enumerate(spec['res']):
        own = l >= spec['start_hash'] and int(r) ** 3 <= cap
        off.append(total if own else -1)
        total += int(r) ** 3 if own else 0
    return off, (total + 2 if total else 0)


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=4)
def base_grid(tag, dev):
    """-> (InvrGrid with row sums and the new fields zero, row sums, keep-alive)"""
    dense, hsh = EC.make_tables(tag)
    spec = params.grid_spec(bbox=EC.BBOX_OF.get(tag, EC.BBOX), **(EC.SPECS[tag] if tag in EC.SPECS else EC.SPECS_FWD[tag]))
    keep = []
    g = _abi.make_grid(spec, dense.to(dev), hsh.to(dev), torch.from_numpy(spec['bbox']).to(dev), keep)
    n = int(_abi.lib().invr_grid_row_sums_len(C.byref(g)))
    rs = torch.full((n,), float('nan'), device=dev)
    _abi.check(_abi.lib().invr_grid_row_sums(C.byref(g), _abi.ptr(rs), _abi.stream_ptr()))
    sync()
    g.row_sums = rs.data_ptr()
    assert g.vertex_rows == 0
    return g, rs, keep, spec


@functools.lru_cache(maxsize=12)
def vertex_grid(tag, cap, dev):
    """-> (InvrGrid whose row sums are followed by its vertex tables (vertex_rows = cap), the tables + 64 guard floats (a view of
    that buffer), offsets per level by the layout rule, floats)"""
    g0, rs, keep, spec = base_grid(tag, dev)
    L = _abi.lib()
    n = int(L.invr_grid_vertex_sums_len(C.byref(g0), cap))
    off, n_py = params.vertex_layout(spec, cap)
    assert (off, n) == expected_layout(EC.make_spec(tag), cap) and n_py == n, (tag, cap)
    buf = torch.full((rs.numel() + n + 64,), float('nan'), device=dev)
    buf[:rs.numel()] = rs
    buf[rs.numel() + n:] = MARK
    vs = buf[rs.numel():]
    _abi.check(L.invr_grid_vertex_sums(C.byref(g0), cap, C.c_void_p(vs.data_ptr()), _abi.stream_ptr()))
    sync()
    g = _abi.InvrGrid.from_buffer_copy(g0)
    g.row_sums, g.vertex_rows = buf.data_ptr(), cap          # (a cap that gives no table: the row sums alone are read)
    assert torch.equal(buf[:rs.numel()].view(torch.int32), rs.view(torch.int32)), 'the builder wrote into the row sums'
    return g, vs, off, n


def grid_for(tag, cap):
    return base_grid(tag, DEV)[0] if cap is None else vertex_grid(tag, cap, DEV)[0]


# ---- 1. the builder -------------------------------------------------------------------------------------------------------------------
BUILD = [(t, c) for t in FAMILIES for c in ('none', 'some', 'all')]


@pytest.mark.parametrize('tag,capname', BUILD, ids=['%s-%s' % c for c in BUILD])
def test_vertex_sums_builder(tag, capname):
    cap = caps_of(tag)[capname]
    spec = EC.make_spec(tag)
    g, vs, off, n = vertex_grid(tag, cap, DEV)
    rs = base_grid(tag, DEV)[1].cpu().numpy().view(np.int32)
    v = vs.cpu().numpy()
    assert (v[n:] == MARK).all(), 'written behind the tables'
    sh, T = spec['start_hash'], int(spec['T'])
    moved = [l for l in range(spec['L']) if off[l] >= 0]
    assert moved == [l for l in range(sh, spec['L']) if int(spec['res'][l]) ** 3 <= cap]
    if capname == 'none':
        assert n == 0 and moved == []
        return
    assert moved and (capname == 'all' or len(moved) < spec['L'] - sh)
    assert (v[n - 2:n] == 0).all(), 'pad floats'
    for l in moved:
        res = int(spec['res'][l])
        i = np.arange(res ** 3, dtype=np.int64)
        cx, cy, cz = i // (res * res), i // res % res, i % res
        row = (cx ^ (cy * GR.HASH_P1) ^ (cz * GR.HASH_P2)) % T                 # part_base_embedder.py:132-136
        base = spec['dense_rows'] + (l - sh) * T if spec['separate_dense'] else l * T
        got = v[off[l]:off[l] + res ** 3].view(np.int32)
        bad = int((got != rs[base + row]).sum())
        assert bad == 0, '%s level %d: %d of %d entries are not the row sum they name' % (tag, l, bad, res ** 3)


def test_vertex_sums_cap_zero_is_off():
    L = _abi.lib()
    for tag in FAMILIES:
        g0 = base_grid(tag, DEV)[0]
        assert L.invr_grid_vertex_sums_len(C.byref(g0), 0) == 0
        assert params.vertex_layout(base_grid(tag, DEV)[3], 0) == ([-1] * 16, 0)
        assert L.invr_grid_vertex_sums(C.byref(g0), 0, None, _abi.stream_ptr()) == 0          # nothing to build: `out` is not touched


# ---- 2. the encoder: tables on == tables off ----------------------------------------------------------------------------------------------
def aligned_bytes(nbytes):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


def run_part(g, x, kernel):
    n = x.shape[0]
    out = torch.full((n + 1, 19), float('nan'), device=DEV)
    out[n:] = MARK
    xd = x.to(DEV).contiguous()
    L = _abi.lib()
    nbytes = L.invr_part_encode_workspace(n)
    ws = aligned_bytes(nbytes)
    _abi.check(L.invr_part_encode_fwd(C.byref(g), _abi.ptr(xd), n, kernel, _abi.ptr(out), C.c_void_p(ws.data_ptr()), nbytes, _abi.stream_ptr()))
    sync()
    out = out.cpu()
    assert (out[n:] == MARK).all(), 'written past the count'
    assert not torch.isnan(out[:n]).any()
    return out[:n]


@functools.lru_cache(maxsize=None)
def cloud(tag, kind, n, seed=0):
    return EC.make_cloud(kind, n, EC.make_spec(tag), seed)


ENC = [(t, c, n) for t in FAMILIES for c in CLOUDS for n in SIZES]


def run_encoder_case(tag, kind, n):
    x = cloud(tag, kind, n)
    for kernel in (0, 2):
        off = run_part(grid_for(tag, None), x, kernel)
        for capname, cap in caps_of(tag).items():
            on = run_part(grid_for(tag, cap), x, kernel)
            assert torch.equal(on, off), '%s %s %d kernel %d cap %s: %d of %d elements differ, columns %s' % (
                tag, kind, n, kernel, capname, int((on != off).sum()), on.numel(), sorted(set((on != off).nonzero()[:, 1].tolist())))


@pytest.mark.parametrize('tag,kind,n', ENC, ids=['%s-%s-%d' % c for c in ENC])
def test_vertex_sums_encoder(tag, kind, n):
    run_encoder_case(tag, kind, n)


def test_ties_cloud_reaches_the_far_corner_of_a_moved_level():
    """The cases above mean what they say: at the `some` cap the `ties` cloud has points with c1 - c0 == 2 on the z axis (the dense
    route's reload) and on x / y of a level that reads its vertex table."""
    for tag in FAMILIES:
        spec = EC.make_spec(tag)
        moved = [l for l, o in enumerate(expected_layout(spec, caps_of(tag)['all'])[0]) if o >= 0]
        cells = GR.fp32_cells(cloud(tag, 'ties', 1000), spec['bbox'], spec)
        for a in range(3):
            two = sum(int((cells[l][1][:, a] - cells[l][0][:, a] == 2).sum()) for l in moved)
            assert two > 0, (tag, 'axis', a)


# ---- five parts in one launch ---------------------------------------------------------------------------------------------------------
FIVE = [('part-small', 'ties'), ('part-t9', 'uniform'), ('part-prod', 'faces'), ('part-t9', 'ties'), ('part-prod', 'wrap')]
FIVE_COUNTS, FIVE_CAP, FIVE_STRIDE = (300, 0, 1, 700, 256), 700, 704


def run_five(capname):
    L = _abi.lib()
    grids = (_abi.InvrGrid * 5)(*[grid_for(t, None if capname is None else caps_of(t)[capname]) for t, _ in FIVE])
    xs, embs = [], []
    for p, (tag, kind) in enumerate(FIVE):
        n = FIVE_COUNTS[p]
        soa = torch.full((3, FIVE_STRIDE), float('nan'))
        if n:
            soa[:, :n] = cloud(tag, kind, n, 20 + p).t()
        e = torch.full((20, FIVE_CAP), MARK)
        e[:, :n] = float('nan')
        xs.append(soa.to(DEV)); embs.append(e.to(DEV))
    cnt = torch.tensor(FIVE_COUNTS, dtype=torch.int32).to(DEV)
    xp = (C.c_void_p * 5)(*[_abi.ptr(t).value for t in xs])
    ep = (C.c_void_p * 5)(*[_abi.ptr(t).value for t in embs])
    _abi.check(L.invr_part_encode_fwd_all(grids, xp, FIVE_STRIDE, _abi.ptr(cnt, torch.int32), FIVE_CAP, 0, ep, _abi.stream_ptr()))
    sync()
    return [e.cpu() for e in embs]


def test_vertex_sums_five_parts_one_launch():
    """The frame's five-part launch, counts 300-0-1-700-256: parts with and without tables side by side, the staged LDS level replaced
    between parts.  Every part equals the launch without tables, and nothing at or past a count is written."""
    off = run_five(None)
    for capname in ('some', 'all'):
        on = run_five(capname)
        for p, n in enumerate(FIVE_COUNTS):
            assert (on[p][:, n:] == MARK).all(), 'part %d: written at or past its count' % p
            assert not torch.isnan(on[p][:, :n]).any(), 'part %d: not written' % p
            assert torch.equal(on[p], off[p]), 'part %d cap %s: %d elements differ' % (p, capname, int((on[p] != off[p]).sum()))
