"""CPU: include/invr_imgloss.h against the library and its binding table (invr._abi.SIGNATURES_IMGLOSS) — what
tests/test_abi_perceptual_cpu.py does for include/invr_perceptual.h: every declared symbol is exported, the table states each
prototype with the header's types (by kind and width) in the header's order, the layout struct mirrors the header's field list, and
the argument checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind
from tests.test_abi_perceptual_cpu import lib

HEADER = os.path.join(ROOT, 'include', 'invr_imgloss.h')


def header_text():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return re.sub(r'//[^\n]*', '', src)


def header_prototypes():
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', header_text(), flags=re.M)
    return [(ret.strip(), name, [a.strip() for a in args.split(',') if a.strip() != 'void']) for ret, name, args in protos]


def test_library_exports_imgloss_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 10 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_IMGLOSS)
    assert not set(_abi.SIGNATURES_IMGLOSS) & (set(_abi.SIGNATURES) | set(_abi.SIGNATURES_PERCEPTUAL))          # the other tables are untouched
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_IMGLOSS[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)


def test_layout_struct_mirrors_the_header():
    from invr import _abi
    body = re.search(r'typedef struct InvrImglossLayout \{(.*?)\} InvrImglossLayout;', header_text(), re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            assert decl.startswith('int64_t '), decl
            fields += [f.strip() for f in decl[len('int64_t '):].split(',')]
    assert fields == [k for k, _ in _abi.InvrImglossLayout._fields_]
    assert all(t is C.c_int64 for _, t in _abi.InvrImglossLayout._fields_)


def test_workspace_layout_is_disjoint_aligned_and_sized():
    from invr import _abi
    L = lib()
    for H, W, w in ((2, 2, 11), (7, 9, 11), (17, 15, 31), (64, 64, 11), (640, 33, 1), (2048, 2048, 11)):
        lay = _abi.InvrImglossLayout()
        assert L.invr_imgloss_workspace_layout(H, W, w, C.byref(lay)) == 0
        P = H * W
        size = {'rank': 4 * P, 'img': 24 * P, 'mom': 60 * P, 'smap': 12 * P, 'pqr': 36 * P, 'occ': P, 'tvmax': 8 * lay.n_tv,
                'partial': 8 * lay.n_partial, 'out8': 32, 'gimg': 12 * P}
        end = 0
        for k in _abi.InvrImglossLayout.ARRAYS:
            off = getattr(lay, k)
            assert off % 256 == 0 and off >= end, (H, W, k)
            end = off + size[k]
        assert end <= lay.bytes == L.invr_imgloss_workspace_bytes(H, W, w)
        assert lay.n_ssim == 3 * ((H + 15) // 16) * ((W + 15) // 16) and lay.n_tv == min((P + 255) // 256, 1024)
        assert lay.n_partial == max(lay.n_ssim, 4 * lay.n_tv) + 2
    for H, W, w in ((1, 8, 11), (8, 2049, 11), (8, 8, 10), (8, 8, 33), (8, 8, 0)):
        assert L.invr_imgloss_workspace_bytes(H, W, w) == 0


def test_argument_checks_return_a_status_and_launch_nothing():
    from invr import _abi
    L = lib()
    lay = _abi.InvrImglossLayout()
    assert L.invr_imgloss_workspace_layout(1, 8, 11, C.byref(lay)) != 0 and b'H, W must be in' in L.invr_last_error()
    assert L.invr_imgloss_workspace_layout(8, 8, 11, None) != 0 and b'null layout' in L.invr_last_error()
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    nb = L.invr_imgloss_workspace_bytes(8, 8, 11)
    assert L.invr_ssim_fwd(a, a, a, a, 11, 4, 1, 8, a, nb, a, None) != 0 and b'invr_ssim_fwd: H, W must be in' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, a, a, a, 12, 4, 8, 8, a, nb, a, None) != 0 and b'the window must be odd' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, a, a, a, 11, 65, 8, 8, a, nb, a, None) != 0 and b'n_rays must be in [0, H*W]' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, a, None, a, 11, 4, 8, 8, a, nb, a, None) != 0 and b'null mask / workspace' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, a, a, a, 11, 4, 8, 8, a + 64, nb, a, None) != 0 and b'256-byte aligned' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, a, a, a, 11, 4, 8, 8, a, nb - 1, a, None) != 0 and b'workspace too small' in L.invr_last_error()
    assert L.invr_ssim_fwd(a, None, a, a, 11, 4, 8, 8, a, nb, a, None) != 0 and b'null rgb / taps / out8' in L.invr_last_error()
    assert L.invr_ssim_bwd(a, a, 11, 4, 8, 8, a, nb, None, a, None) != 0 and b'null taps / g_loss / g_rgb' in L.invr_last_error()
    assert L.invr_tv_fwd(a, a, None, a, 4, 8, 8, a, nb, a, None) != 0 and b'null rgb / occupancy / out8' in L.invr_last_error()
    assert L.invr_tv_bwd(a, -1, 8, 8, a, nb, a, a, None) != 0 and b'invr_tv_bwd: n_rays' in L.invr_last_error()
    assert L.invr_train_loss_ssim_fwd(a, a, a, a, 11, None, None, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, None, None) != 0
    assert b'invr_train_loss_ssim_fwd: null pointer' in L.invr_last_error()
    assert L.invr_train_loss_ssim_bwd(a, a, 11, a, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, a, None, None, None) != 0
    assert b'invr_train_loss_ssim_bwd: null pointer' in L.invr_last_error()
    assert L.invr_train_loss_tv_fwd(a, a, a, a, None, None, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, None, None) != 0
    assert b'invr_train_loss_tv_fwd: null pointer' in L.invr_last_error()
    assert L.invr_train_loss_tv_bwd(a, a, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, a, None, None, None) != 0
    assert b'invr_train_loss_tv_bwd: null pointer' in L.invr_last_error()
