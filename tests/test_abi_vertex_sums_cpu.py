"""CPU: include/invr_vertex.h (invr_grid_vertex_sums_len / invr_grid_vertex_sums) against the library and its binding table
(invr._abi.SIGNATURES_VERTEX), the argument checks and the length rule of the de-hashed vertex tables.  No compute calls: every call
stops at a check or has nothing to build.  include/invr.h keeps its prototypes, its ABI version and the size of InvrGrid: the one new
field, vertex_rows, lies where the struct had four bytes of padding."""
import ctypes as C
import os
import re

import pytest
import torch

from invr import _abi, params
from invr.config import make_cfg, PART_NAMES
from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

LIMIT = 2 ** 24
HEADER = os.path.join(ROOT, 'include', 'invr_vertex.h')


def test_library_exports_vertex_header_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', src, flags=re.M)
    protos = [(ret.strip(), name, [a.strip() for a in args.split(',')]) for ret, name, args in protos]
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_VERTEX) == ['invr_grid_vertex_sums_len', 'invr_grid_vertex_sums']
    others = set(_abi.SIGNATURES) | set(_abi.SIGNATURES_PERCEPTUAL) | set(_abi.SIGNATURES_MESH) | set(_abi.SIGNATURES_BATCH) | set(_abi.SIGNATURES_SAMPLE)
    assert not set(_abi.SIGNATURES_VERTEX) & others
    L = _abi.lib()
    assert _abi.EXPORTS == list(_abi.SIGNATURES) and L.invr_version() == _abi.ABI_VERSION == 2
    for ret, name, decls in protos:
        restype, argtypes = _abi.SIGNATURES_VERTEX[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert ctypes_kind(restype) == c_kind(ret) and len(argtypes) == len(decls), name
        for i, (decl, t) in enumerate(zip(decls, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)
    assert int(re.search(r'#define INVR_VERTEX_MAX_ROWS (\d+)', src).group(1)) == LIMIT == params.VERTEX_MAX_ROWS
    assert 'invr_grid_vertex_sums' not in re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'invr.h')).read(), flags=re.S)
    # vertex_rows fills padding: the struct and the field behind it stay where they were
    assert _abi.InvrGrid.vertex_rows.offset == _abi.InvrGrid.include_input.offset + 4 == _abi.InvrGrid.row_sums.offset - 4
    assert L.invr_sizeof(0) == C.sizeof(_abi.InvrGrid)


def grid_of(spec, keep):
    """An InvrGrid of `spec` over placeholder tables (never read here)."""
    t = torch.zeros(16)
    return _abi.make_grid(spec, t if spec['separate_dense'] else None, t, torch.from_numpy(spec['bbox']), keep)


def test_vertex_sums_argument_checks():
    L = _abi.lib()
    keep = []
    g = grid_of(params.grid_spec(log2_hashmap_size=12), keep)
    out = (C.c_float * 4)()
    assert L.invr_grid_vertex_sums_len(None, 1 << 20) == 0
    assert L.invr_grid_vertex_sums(None, 1 << 20, out, None) != 0 and b'null pointer' in L.invr_last_error()
    # the tables are built from the row sums
    assert not g.row_sums
    assert L.invr_grid_vertex_sums(C.byref(g), 1 << 20, out, None) != 0 and b'needs grid->row_sums' in L.invr_last_error()
    # 2^24 vertices per level is the limit (the dense route multiplies in 24 bits): one more is refused by both entry points
    g.row_sums = C.addressof(out)
    assert L.invr_grid_vertex_sums_len(C.byref(g), LIMIT) > 0
    assert L.invr_grid_vertex_sums_len(C.byref(g), LIMIT + 1) == -1 and b'2^24' in L.invr_last_error()
    assert L.invr_grid_vertex_sums(C.byref(g), LIMIT + 1, out, None) != 0 and b'2^24' in L.invr_last_error()
    assert L.invr_grid_vertex_sums(C.byref(g), -1, out, None) != 0
    assert L.invr_grid_vertex_sums(C.byref(g), 19 ** 3, None, None) != 0 and b'null pointer' in L.invr_last_error()      # its first hashed level to build, nowhere to put it
    assert L.invr_grid_vertex_sums(C.byref(g), 19 ** 3 - 1, None, None) == 0                                            # nothing to build
    assert params.VERTEX_MAX_ROWS == LIMIT
    with pytest.raises(ValueError):                                             # the Python layout refuses what the library refuses
        params.vertex_layout(params.grid_spec(log2_hashmap_size=12), LIMIT + 1)


def test_encoder_refuses_vertex_rows_above_the_limit():
    """A grid that tells the encoder its row sums are followed by vertex tables is held to the limit before anything is launched."""
    L = _abi.lib()
    keep = []
    g = grid_of(params.grid_spec(log2_hashmap_size=12), keep)
    buf = (C.c_float * 4)()
    g.row_sums = C.addressof(buf)
    ws = (C.c_char * 4096)()
    for bad in (LIMIT + 1, -1):
        g.vertex_rows = bad
        for kernel in (0, 2):
            st = L.invr_part_encode_fwd(C.byref(g), buf, 1, kernel, buf, ws, L.invr_part_encode_workspace(1), None)
            assert st != 0 and b'vertex_rows' in L.invr_last_error(), L.invr_last_error()


def test_vertex_sums_len_of_the_production_grids():
    """invr_grid_vertex_sums_len against grid_spec arithmetic, the five production grids at caps 2^20 and 2^22: the levels l >=
    start_hash with res_l^3 <= cap, back to back, + two pad floats — and the Python restatement of the layout says the same."""
    L = _abi.lib()
    cfg = make_cfg()
    keep = []
    moved = {}
    for name in PART_NAMES:
        spec = params.part_grid_spec(cfg, name)
        g = grid_of(spec, keep)
        for cap in (2 ** 20, 2 ** 22):
            levels = [l for l in range(spec['start_hash'], spec['L']) if spec['res'][l] ** 3 <= cap]
            want = sum(spec['res'][l] ** 3 for l in levels) + (2 if levels else 0)
            assert L.invr_grid_vertex_sums_len(C.byref(g), cap) == want, (name, cap)
            off, n = params.vertex_layout(spec, cap)
            assert n == want and [l for l in range(16) if off[l] >= 0] == levels, (name, cap)
            assert [off[l] for l in levels] == [sum(spec['res'][k] ** 3 for k in levels if k < l) for l in levels]
            moved[name, cap] = levels
        assert L.invr_grid_vertex_sums_len(C.byref(g), 0) == 0
    # the hashed levels of the production grids that fit (resolutions int(base 1.38^l): 36, 50, 69, 95, 132, 182, 251 / body 110, 152)
    assert moved['larm', 2 ** 20] == moved['rarm', 2 ** 20] == [9, 10, 11, 12] and moved['head', 2 ** 20] == [11, 12]
    assert moved['leg', 2 ** 20] == [] and moved['body', 2 ** 20] == []
    assert moved['larm', 2 ** 22] == [9, 10, 11, 12, 13] and moved['head', 2 ** 22] == [11, 12, 13] and moved['leg', 2 ** 22] == [13]
    assert moved['body', 2 ** 22] == [6, 7]
