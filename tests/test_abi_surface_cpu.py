"""CPU: include/invr_surface.h against the library and its binding table (invr._abi.SIGNATURES_SURFACE) — what
tests/test_abi_posescene_cpu.py does for include/invr_posescene.h: every declared symbol is exported, the table states each prototype
with the header's types (by kind and width) in the header's order, the workspace size is monotone and 0 outside the limits, and the
argument checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_surface.h')


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


def test_library_exports_surface_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 3 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_SURFACE)
    others = (_abi.SIGNATURES, _abi.SIGNATURES_PERCEPTUAL, _abi.SIGNATURES_MESH, _abi.SIGNATURES_BATCH, _abi.SIGNATURES_SAMPLE, _abi.SIGNATURES_VERTEX,
              _abi.SIGNATURES_POSESCENE)
    assert not any(set(_abi.SIGNATURES_SURFACE) & set(t) for t in others)          # the other tables are untouched
    assert L.invr_version() == _abi.ABI_VERSION == 2                                # include/invr.h did not move
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_SURFACE[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)
    src = open(HEADER).read()
    for line in ('#define INVR_SURFACE_MAX_VERTS ((int32_t)1 << 20)', '#define INVR_SURFACE_MAX_FACES ((int32_t)1 << 20)',
                 '#define INVR_SURFACE_MAX_POINTS ((int64_t)1 << 27)', '#define INVR_SURFACE_MAX_CHANNELS 64'):
        assert line in src, line


def test_workspace_size_is_monotone_and_zero_outside_the_limits():
    L = lib()
    size = L.invr_surface_volume_workspace_bytes
    prev = 0
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 1000, 13776, 13777, 2 ** 16, 2 ** 20 - 1, 2 ** 20):
        b = size(n)
        assert b >= 80 * n and b % 256 == 0 and b >= prev, n          # a 48-byte record and a 32-byte sphere per face
        prev = b
    for n in (0, -1, -2 ** 31, 2 ** 20 + 1, 2 ** 31 - 1):
        assert size(n) == 0, n


def test_volume_argument_checks_return_a_status_and_launch_nothing():
    L = lib()
    err = L.invr_last_error
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    nv, nf = 100, 150
    nb = L.invr_surface_volume_workspace_bytes(nf)
    o, s, dims = d3(0.0, 0.0, 0.0), d3(0.025, 0.025, 0.025), i3(3, 5, 4)
    inf, nan = float('inf'), float('nan')
    null = b'invr_surface_volume: null verts / faces / origin / step / dims / face / workspace'

    def call(verts=a, n_verts=nv, faces=a, n_faces=nf, origin=o, step=s, dims=dims, face=a, bary=a, dist=a, ws=a, ws_bytes=nb):
        return L.invr_surface_volume(verts, n_verts, faces, n_faces, origin, step, dims, face, bary, dist, ws, ws_bytes, None)

    for kw in (dict(verts=None), dict(faces=None), dict(face=None), dict(ws=None)):
        assert call(**kw) != 0 and null in err(), kw
    from invr import _abi
    raw = C.CDLL(_abi.LIB_PATH).invr_surface_volume          # (the table's array types take no NULL: an untyped handle of the same library)
    raw.restype = C.c_int
    vp = C.c_void_p
    for k in (4, 5, 6):
        args = [vp(a), C.c_int32(nv), vp(a), C.c_int32(nf), o, s, dims, vp(a), vp(a), vp(a), vp(a), C.c_size_t(nb), vp(0)]
        args[k] = vp(0)
        assert raw(*args) != 0 and null in err(), k
    assert call(bary=None, dist=None, n_verts=0) != 0 and b'n_verts must be' in err()          # bary and dist may be NULL: the next check answers
    for bad in (0, -5, 2 ** 20 + 1):
        assert call(n_verts=bad) != 0 and b'invr_surface_volume: n_verts must be in [1, 2^20]' in err(), bad
        assert call(n_faces=bad) != 0 and b'invr_surface_volume: n_faces must be in [1, 2^20]' in err(), bad
    for bad in (i3(0, 5, 4), i3(3, -1, 4), i3(3, 5, 0)):
        assert call(dims=bad) != 0 and b'invr_surface_volume: every dimension must be >= 1' in err()
    for bad in (i3(513, 512, 512), i3(2 ** 27 + 1, 1, 1), i3(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), i3(1, 2 ** 14, 2 ** 14)):
        assert call(dims=bad) != 0 and b'invr_surface_volume: more than 2^27 lattice points' in err()
    for bad in (d3(0.025, 0.0, 0.025), d3(-0.025, 0.025, 0.025), d3(0.025, 0.025, nan), d3(inf, 0.025, 0.025)):
        assert call(step=bad) != 0 and b'invr_surface_volume: step must be finite and > 0' in err()
    for bad in (d3(nan, 0.0, 0.0), d3(0.0, inf, 0.0), d3(0.0, 0.0, -inf)):
        assert call(origin=bad) != 0 and b'invr_surface_volume: origin must be finite' in err()
    assert call(ws=a + 64) != 0 and b'256-byte aligned' in err()
    assert call(ws_bytes=nb - 1) != 0 and b'invr_surface_volume: workspace too small' in err()
    assert call(n_faces=2 ** 20, ws_bytes=L.invr_surface_volume_workspace_bytes(2 ** 20) - 1) != 0 and b'workspace too small' in err()


def test_interpolate_argument_checks_return_a_status_and_launch_nothing():
    L = lib()
    err = L.invr_last_error
    a = 256

    def call(attr=a, n_verts=100, nc=24, faces=a, n_faces=150, face=a, bary=a, n_points=1000, out=a, stride=25, offset=0):
        return L.invr_surface_interpolate(attr, n_verts, nc, faces, n_faces, face, bary, n_points, out, stride, offset, None)

    for bad in (0, -1, 65, 2 ** 31 - 1):
        assert call(nc=bad, stride=2 ** 20) != 0 and b'invr_surface_interpolate: n_channels must be in [1, 64]' in err(), bad
    for bad in (0, -5, 2 ** 20 + 1):
        assert call(n_verts=bad) != 0 and b'invr_surface_interpolate: n_verts must be in [1, 2^20]' in err(), bad
        assert call(n_faces=bad) != 0 and b'invr_surface_interpolate: n_faces must be in [1, 2^20]' in err(), bad
    for bad in (-1, 2 ** 27 + 1, 2 ** 62):
        assert call(n_points=bad) != 0 and b'invr_surface_interpolate: n_points must be in [0, 2^27]' in err(), bad
    for stride, offset in ((23, 0), (25, 2), (25, -1), (0, 0), (-25, 0), (2 ** 20 + 1, 0), (-2 ** 63, 0), (25, 2 ** 63 - 1)):
        assert call(stride=stride, offset=offset) != 0 and b'out_offset + n_channels <= out_stride' in err(), (stride, offset)
    for kw in (dict(attr=None), dict(faces=None), dict(face=None), dict(bary=None), dict(out=None)):
        assert call(**kw) != 0 and b'invr_surface_interpolate: null attr / faces / face / bary / out' in err(), kw
    assert call(n_points=0, attr=None, out=None) == 0          # no points: nothing to do
    assert call(stride=24, offset=0, out=None) != 0 and b'null attr' in err()
