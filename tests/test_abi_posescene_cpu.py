"""CPU: include/invr_posescene.h against the library and its binding table (invr._abi.SIGNATURES_POSESCENE) — what
tests/test_abi_mesh_cpu.py does for include/invr_mesh.h: every declared symbol is exported, the table states each prototype with the
header's types (by kind and width) in the header's order, the workspace size is monotone and 0 outside the limits, and the argument
checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_posescene.h')


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


def i3(*v):
    return (C.c_int32 * 3)(*v)


def d3(*v):
    return (C.c_double * 3)(*v)


def test_library_exports_posescene_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 2 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_POSESCENE)
    others = (_abi.SIGNATURES, _abi.SIGNATURES_PERCEPTUAL, _abi.SIGNATURES_MESH, _abi.SIGNATURES_BATCH, _abi.SIGNATURES_SAMPLE, _abi.SIGNATURES_VERTEX)
    assert not any(set(_abi.SIGNATURES_POSESCENE) & set(t) for t in others)          # the other tables are untouched
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_POSESCENE[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)
    src = open(HEADER).read()
    assert '#define INVR_POSESCENE_MAX_VERTS ((int32_t)1 << 20)' in src and '#define INVR_POSESCENE_MAX_POINTS ((int64_t)1 << 27)' in src


def test_workspace_size_is_monotone_and_zero_outside_the_limits():
    L = lib()
    size = L.invr_distance_volume_workspace_bytes
    prev = 0
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 1000, 6890, 6891, 2 ** 16, 2 ** 20 - 1, 2 ** 20):
        b = size(n)
        assert b >= 16 * n and b % 256 == 0 and b >= prev, n          # one 16-byte record per vertex
        prev = b
    for n in (0, -1, -2 ** 31, 2 ** 20 + 1, 2 ** 31 - 1):
        assert size(n) == 0, n


def test_argument_checks_return_a_status_and_launch_nothing():
    L = lib()
    err = L.invr_last_error
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    n = 100
    nb = L.invr_distance_volume_workspace_bytes(n)
    o, s, dims = d3(0.0, 0.0, 0.0), d3(0.025, 0.025, 0.025), i3(3, 5, 4)
    inf, nan = float('inf'), float('nan')

    def call(verts=a, n_verts=n, origin=o, step=s, dims=dims, dist=a, nearest=a, ws=a, ws_bytes=nb):
        return L.invr_distance_volume(verts, n_verts, origin, step, dims, dist, nearest, ws, ws_bytes, None)

    for kw in (dict(verts=None), dict(dist=None), dict(ws=None)):
        assert call(**kw) != 0 and b'invr_distance_volume: null verts / origin / step / dims / dist / workspace' in err(), kw
    from invr import _abi
    raw = C.CDLL(_abi.LIB_PATH).invr_distance_volume          # (the table's array types take no NULL: an untyped handle of the same library)
    raw.restype = C.c_int
    vp = C.c_void_p
    for k in (2, 3, 4):
        args = [vp(a), C.c_int32(n), o, s, dims, vp(a), vp(a), vp(a), C.c_size_t(nb), vp(0)]
        args[k] = vp(0)
        assert raw(*args) != 0 and b'invr_distance_volume: null verts / origin / step / dims / dist / workspace' in err(), k
    assert call(nearest=None, n_verts=0) != 0 and b'n_verts must be' in err()          # nearest may be NULL: the next check answers
    for bad in (0, -5, 2 ** 20 + 1):
        assert call(n_verts=bad) != 0 and b'invr_distance_volume: n_verts must be in [1, 2^20]' in err(), bad
    for bad in (i3(0, 5, 4), i3(3, -1, 4), i3(3, 5, 0)):
        assert call(dims=bad) != 0 and b'invr_distance_volume: every dimension must be >= 1' in err()
    for bad in (i3(513, 512, 512), i3(2 ** 27 + 1, 1, 1), i3(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), i3(1, 2 ** 14, 2 ** 14)):
        assert call(dims=bad) != 0 and b'invr_distance_volume: more than 2^27 lattice points' in err()
    for bad in (d3(0.025, 0.0, 0.025), d3(-0.025, 0.025, 0.025), d3(0.025, 0.025, nan), d3(inf, 0.025, 0.025)):
        assert call(step=bad) != 0 and b'invr_distance_volume: step must be finite and > 0' in err()
    for bad in (d3(nan, 0.0, 0.0), d3(0.0, inf, 0.0), d3(0.0, 0.0, -inf)):
        assert call(origin=bad) != 0 and b'invr_distance_volume: origin must be finite' in err()
    assert call(ws=a + 64) != 0 and b'256-byte aligned' in err()
    assert call(ws_bytes=nb - 1) != 0 and b'invr_distance_volume: workspace too small' in err()
    assert call(n_verts=2 ** 20, ws_bytes=L.invr_distance_volume_workspace_bytes(2 ** 20) - 1) != 0 and b'workspace too small' in err()
