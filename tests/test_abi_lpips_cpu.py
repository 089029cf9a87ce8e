"""CPU: include/invr_lpips.h against the library and its binding table (invr._abi.SIGNATURES_LPIPS), in the manner of
tests/test_abi_perceptual_cpu.py: every declared symbol is exported, the table states each prototype with the header's types (by kind
and width) in the header's order, the layout struct mirrors the header's field list, the layouts are disjoint, aligned and sized, and
the argument checks return a status with the function's name in the message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind
from tests.test_abi_perceptual_cpu import lib

HEADER = os.path.join(ROOT, 'include', 'invr_lpips.h')
CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
BLOCK = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
TAPS = (1, 3, 6, 9, 12)


def header_text():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return re.sub(r'//[^\n]*', '', src)


def header_prototypes():
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', header_text(), flags=re.M)
    return [(ret.strip(), name, [' '.join(a.split()) for a in args.split(',') if a.strip() != 'void']) for ret, name, args in protos]


def test_library_exports_lpips_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 5 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_LPIPS)
    assert not set(_abi.SIGNATURES_LPIPS) & (set(_abi.SIGNATURES) | set(_abi.SIGNATURES_PERCEPTUAL))          # the other tables are untouched
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_LPIPS[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)


def test_layout_struct_mirrors_the_header():
    from invr import _abi
    body = re.search(r'typedef struct InvrLpipsLayout \{(.*?)\} InvrLpipsLayout;', header_text(), re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            assert decl.startswith('int64_t '), decl
            m = re.fullmatch(r'(\w+)(?:\[(\d+)\])?', decl[len('int64_t '):].strip())
            fields.append((m.group(1), int(m.group(2)) if m.group(2) else 0))
    mirror = [(k, t._length_ if hasattr(t, '_length_') else 0) for k, t in _abi.InvrLpipsLayout._fields_]
    assert fields == mirror
    assert all((t._type_ if hasattr(t, '_length_') else t) is C.c_int64 for _, t in _abi.InvrLpipsLayout._fields_)
    assert (tuple(_abi.LPIPS_CIN), tuple(_abi.LPIPS_COUT), tuple(_abi.LPIPS_BLOCK), tuple(_abi.LPIPS_TAPS)) == (CIN, COUT, BLOCK, TAPS)


def arrays(lay, H, W):
    """(name, byte offset, byte size) of every stored array of a layout"""
    out = [('scaled', lay.scaled, 24 * H * W)]
    for l in range(13):
        out.append(('act%d' % l, lay.act[l], 8 * COUT[l] * (H >> BLOCK[l]) * (W >> BLOCK[l])))
    for b in range(4):
        out.append(('pool%d' % b, lay.pool[b], 8 * CIN[TAPS[b] + 1] * (H >> (b + 1)) * (W >> (b + 1))))
    out.append(('partial', lay.partial, 8 * lay.n_partial))
    return out


def test_keep_layout_is_disjoint_aligned_and_sized():
    from invr import _abi
    L = lib()
    for H, W in ((16, 16), (17, 19), (16, 67), (37, 53), (48, 64), (100, 31)):
        lay = _abi.InvrLpipsLayout()
        assert L.invr_lpips_workspace_layout(H, W, 1, C.byref(lay)) == 0
        spans = sorted((off, off + size, name) for name, off, size in arrays(lay, H, W))
        end = 0
        for lo, hi, name in spans:
            assert lo % 256 == 0 and lo >= end, (H, W, name)
            end = hi
        assert end <= lay.bytes == L.invr_lpips_workspace_bytes(H, W, 1)
        n = 0
        for t in range(5):
            pixels = (H >> t) * (W >> t)
            assert lay.part_off[t] == n and lay.n_part[t] == (pixels + 15) // 16
            n += lay.n_part[t]
        assert n == lay.n_partial


def test_rotating_layout_stays_inside_its_bytes_and_never_writes_its_input():
    from invr import _abi
    L = lib()
    for H, W in ((16, 16), (37, 53), (512, 512)):
        lay = _abi.InvrLpipsLayout()
        assert L.invr_lpips_workspace_layout(H, W, 0, C.byref(lay)) == 0
        at = dict((name, (off, size)) for name, off, size in arrays(lay, H, W))
        for name, (off, size) in at.items():
            assert off % 256 == 0 and off + size <= lay.bytes == L.invr_lpips_workspace_bytes(H, W, 0), name
        order = []                                       # the stages in stream order: each reads its predecessor and writes elsewhere
        for l in range(13):
            if l > 0 and BLOCK[l] != BLOCK[l - 1]:
                order.append('pool%d' % (BLOCK[l] - 1))
            order.append('act%d' % l)
        prev = 'scaled'
        for name in order:
            (a, na), (b, nb) = at[prev], at[name]
            assert a + na <= b or b + nb <= a, (prev, name)
            assert at['partial'][0] >= b + nb or at['partial'][0] + at['partial'][1] <= b
            prev = name
    assert 0.25e9 < L.invr_lpips_workspace_bytes(512, 512, 0) < 0.35e9


def test_workspace_bytes_is_monotone_and_bounded():
    L = lib()
    for keep in (0, 1):
        for fixed in (16, 40, 333):
            prev_h = prev_w = 0
            for v in list(range(16, 80)) + [127, 128, 129, 500, 512, 640]:
                bh, bw = L.invr_lpips_workspace_bytes(v, fixed, keep), L.invr_lpips_workspace_bytes(fixed, v, keep)
                assert bh >= prev_h > -1 and bw >= prev_w > -1 and bh > 0 and bw > 0, (keep, fixed, v)
                prev_h, prev_w = bh, bw
    for H, W in ((15, 16), (16, 15), (16, 2049), (2049, 16), (0, 0), (-1, 64)):
        assert L.invr_lpips_workspace_bytes(H, W, 0) == 0 and L.invr_lpips_workspace_bytes(H, W, 1) == 0
    limit = int(re.search(r'#define INVR_LPIPS_KEEP_MAX_BYTES (\d+)', open(HEADER).read()).group(1))
    assert L.invr_lpips_workspace_bytes(2048, 2048, 0) > 0
    assert L.invr_lpips_workspace_bytes(2048, 2048, 1) == 0               # 2424 bytes per pixel: beyond the header's limit
    assert 0 < L.invr_lpips_workspace_bytes(900, 900, 1) <= limit
    assert L.invr_lpips_packed_floats() == sum(9 * (4 if l == 0 else CIN[l]) * COUT[l] for l in range(13)) + sum(COUT) + sum(COUT[l] for l in TAPS) + 6


def test_argument_checks_return_a_status_and_launch_nothing():
    from invr import _abi
    L = lib()
    lay = _abi.InvrLpipsLayout()
    assert L.invr_lpips_workspace_layout(15, 16, 0, C.byref(lay)) != 0 and b'invr_lpips_workspace_layout: H, W must be in' in L.invr_last_error()
    assert L.invr_lpips_workspace_layout(16, 2049, 1, C.byref(lay)) != 0 and b'invr_lpips_workspace_layout: H, W must be in' in L.invr_last_error()
    assert L.invr_lpips_workspace_layout(16, 16, 0, None) != 0 and b'invr_lpips_workspace_layout: null layout' in L.invr_last_error()
    assert L.invr_lpips_workspace_layout(2048, 2048, 1, C.byref(lay)) != 0 and b'invr_lpips_workspace_layout: a keep = 1 layout' in L.invr_last_error()
    assert L.invr_lpips_pack_weights(None, None, None, None, None, None, None) != 0 and b'invr_lpips_pack_weights: null pointer' in L.invr_last_error()
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    w13, l5 = (C.c_void_p * 13)(), (C.c_void_p * 5)()
    assert L.invr_lpips_pack_weights(w13, w13, l5, a, a, a, None) != 0 and b'invr_lpips_pack_weights: null weight / bias pointer of layer 0' in L.invr_last_error()
    full = (C.c_void_p * 13)(*([a] * 13))
    assert L.invr_lpips_pack_weights(full, full, l5, a, a, a, None) != 0 and b'invr_lpips_pack_weights: null lin pointer of tap 0' in L.invr_last_error()
    nb = L.invr_lpips_workspace_bytes(16, 16, 0)
    assert L.invr_lpips_fwd(a, a, a, 15, 16, 0, a, nb, a, None) != 0 and b'invr_lpips_fwd: H, W must be in' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 2049, 0, a, nb, a, None) != 0 and b'invr_lpips_fwd: H, W must be in' in L.invr_last_error()
    assert L.invr_lpips_fwd(None, a, a, 16, 16, 0, a, nb, a, None) != 0 and b'invr_lpips_fwd: null packed weights' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, None, a, 16, 16, 0, a, nb, a, None) != 0 and b'invr_lpips_fwd: null packed weights' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 16, 0, None, nb, a, None) != 0 and b'invr_lpips_fwd: null packed weights' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 16, 0, a, nb, None, None) != 0 and b'invr_lpips_fwd: null packed weights' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 16, 0, a + 64, nb, a, None) != 0 and b'invr_lpips_fwd: the workspace must be 256-byte aligned' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 16, 0, a, nb - 1, a, None) != 0 and b'invr_lpips_fwd: workspace too small' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 16, 16, 1, a, nb, a, None) != 0 and b'invr_lpips_fwd: workspace too small' in L.invr_last_error()
    assert L.invr_lpips_fwd(a, a, a, 2048, 2048, 1, a, nb, a, None) != 0 and b'invr_lpips_fwd: a keep = 1 layout' in L.invr_last_error()
