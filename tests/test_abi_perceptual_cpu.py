"""CPU: include/invr_perceptual.h against the library and its binding table (invr._abi.SIGNATURES_PERCEPTUAL) — what
tests/test_abi_symbols.py::test_library_exports_header_symbols does for include/invr.h: every declared symbol is exported, the
table states each prototype with the header's types (by kind and width) in the header's order, the layout struct mirrors the
header's field list, and the argument checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_perceptual.h')


def header_text():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return re.sub(r'//[^\n]*', '', src)


def header_prototypes():
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', header_text(), flags=re.M)
    return [(ret.strip(), name, [a.strip() for a in args.split(',') if a.strip() != 'void']) for ret, name, args in protos]


def lib():
    from invr import _abi
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _abi.lib()


def test_library_exports_perceptual_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 8 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_PERCEPTUAL)
    assert not set(_abi.SIGNATURES_PERCEPTUAL) & set(_abi.SIGNATURES)          # invr.h's table is untouched
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_PERCEPTUAL[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)


def test_layout_struct_mirrors_the_header():
    from invr import _abi
    body = re.search(r'typedef struct InvrPerceptualLayout \{(.*?)\} InvrPerceptualLayout;', header_text(), re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            assert decl.startswith('int64_t '), decl
            fields += [f.strip() for f in decl[len('int64_t '):].split(',')]
    assert fields == [k for k, _ in _abi.InvrPerceptualLayout._fields_]
    assert all(t is C.c_int64 for _, t in _abi.InvrPerceptualLayout._fields_)


def test_workspace_layout_is_disjoint_aligned_and_sized():
    from invr import _abi
    L = lib()
    for H, W in ((2, 2), (3, 3), (9, 7), (17, 15), (56, 56), (64, 64)):
        lay = _abi.InvrPerceptualLayout()
        assert L.invr_perceptual_workspace_layout(H, W, C.byref(lay)) == 0
        P, p = H * W, (H // 2) * (W // 2)
        size = {'rank': 4 * P, 'img': 24 * P, 'a11': 512 * P, 'a12': 512 * P, 'pool': 512 * p, 'a21': 1024 * p, 'a22': 1024 * p,
                'partial': 8 * lay.n_partial, 'out8': 32, 'g22': 512 * p, 'gm22': 512 * p, 'g21': 512 * p, 'gm21': 512 * p, 'gpool': 256 * p,
                'g12': 256 * P, 'gm12': 256 * P, 'g11': 256 * P, 'gm11': 256 * P, 'gimg': 12 * P}
        end = 0
        for k in _abi.InvrPerceptualLayout.ARRAYS:
            off = getattr(lay, k)
            assert off % 256 == 0 and off >= end, (H, W, k)
            end = off + size[k]
        assert end <= lay.bytes == L.invr_perceptual_workspace_bytes(H, W)
        assert lay.n_partial == lay.n_part1 + lay.n_part2 + 2 and lay.n_part1 * 16 >= P * 4 and lay.n_part2 * 16 >= p * 8
    assert L.invr_perceptual_workspace_bytes(1, 8) == 0 and L.invr_perceptual_workspace_bytes(8, 4096) == 0
    assert L.invr_perceptual_packed_floats() == 527488


def test_argument_checks_return_a_status_and_launch_nothing():
    from invr import _abi
    L = lib()
    lay = _abi.InvrPerceptualLayout()
    assert L.invr_perceptual_workspace_layout(1, 8, C.byref(lay)) != 0 and b'H, W must be in' in L.invr_last_error()
    assert L.invr_perceptual_workspace_layout(8, 8, None) != 0 and b'null layout' in L.invr_last_error()
    assert L.invr_perceptual_pack_weights(None, None, None, None) != 0 and b'null pointer' in L.invr_last_error()
    four = (C.c_void_p * 4)()
    assert L.invr_perceptual_pack_weights(four, four, 256, None) != 0 and b'layer 0' in L.invr_last_error()
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    nb = L.invr_perceptual_workspace_bytes(8, 8)
    assert L.invr_perceptual_fwd(a, a, a, a, 4, 1, 8, a, nb, a, None) != 0 and b'invr_perceptual_fwd: H, W must be in' in L.invr_last_error()
    assert L.invr_perceptual_fwd(a, a, a, a, 65, 8, 8, a, nb, a, None) != 0 and b'n_rays must be in [0, H*W]' in L.invr_last_error()
    assert L.invr_perceptual_fwd(None, a, a, a, 4, 8, 8, a, nb, a, None) != 0 and b'null packed weights' in L.invr_last_error()
    assert L.invr_perceptual_fwd(a, a, a, a, 4, 8, 8, a + 64, nb, a, None) != 0 and b'256-byte aligned' in L.invr_last_error()
    assert L.invr_perceptual_fwd(a, a, a, a, 4, 8, 8, a, nb - 1, a, None) != 0 and b'workspace too small' in L.invr_last_error()
    assert L.invr_perceptual_fwd(a, None, a, a, 4, 8, 8, a, nb, a, None) != 0 and b'null rgb / out8' in L.invr_last_error()
    assert L.invr_perceptual_bwd(a, a, 4, 8, 8, a, nb, None, a, None) != 0 and b'null g_loss / g_rgb' in L.invr_last_error()
    assert L.invr_perceptual_bwd(a, a, -1, 8, 8, a, nb, a, a, None) != 0 and b'invr_perceptual_bwd: n_rays' in L.invr_last_error()
    assert L.invr_train_loss_lpips_fwd(a, a, a, a, None, None, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, None, None) != 0
    assert b'invr_train_loss_lpips_fwd: null pointer' in L.invr_last_error()
    assert L.invr_train_loss_lpips_bwd(a, a, a, 4, 8, 8, 0.0, 0.0, 0.0, 0, a, nb, a, a, None, None, None) != 0
    assert b'invr_train_loss_lpips_bwd: null pointer' in L.invr_last_error()
