"""CPU: include/invr_geomaps.h against the library and its binding table (invr._abi.SIGNATURES_GEOMAPS) — what
tests/test_abi_mesh_cpu.py does for include/invr_mesh.h: every declared symbol is exported, the table states each prototype with the
header's types (by kind and width) in the header's order, the struct mirrors the header's field list and invr_sizeof knows it, and the
argument checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_geomaps.h')


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


def test_library_exports_geomaps_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 4 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_GEOMAPS)
    assert not set(_abi.SIGNATURES_GEOMAPS) & (set(_abi.SIGNATURES) | set(_abi.SIGNATURES_MESH) | set(_abi.SIGNATURES_SURFACE))
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_GEOMAPS[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)
    # the render with geometry takes the tracked render's arguments and one more
    geo, tracked = [p for _, n, p in protos if n == 'invr_render_fwd_geo'][0], _abi.SIGNATURES['invr_render_fwd_tracked'][1]
    assert len(geo) == len(tracked) + 1 and 'InvrGeoOut' in geo[-1]


def test_struct_mirrors_the_header_and_invr_sizeof_knows_it():
    from invr import _abi
    L = lib()
    body = re.search(r'typedef struct InvrGeoOut \{(.*?)\} InvrGeoOut;', header_text(), re.S).group(1)
    fields = [d.strip() for d in body.split(';') if d.strip()]
    assert [f.split()[-1].lstrip('*') for f in fields] == [k for k, _ in _abi.InvrGeoOut._fields_]
    for decl, (k, t) in zip(fields, _abi.InvrGeoOut._fields_):
        assert ctypes_kind(t) == c_kind(decl), (decl, t)
    which = int(re.search(r'#define INVR_SIZEOF_GEO_OUT (\d+)', open(HEADER).read()).group(1))
    assert which == _abi.SIZEOF_GEO_OUT
    assert L.invr_sizeof(which) == C.sizeof(_abi.InvrGeoOut) == 32
    assert L.invr_sizeof(which + 1) == 0
    hdr = open(os.path.join(ROOT, 'include', 'invr.h')).read()
    assert int(re.search(r'#define INVR_ABI_VERSION (\d+)', hdr).group(1)) == _abi.ABI_VERSION == 2          # include/invr.h is as it was


def test_argument_checks_return_a_status_and_launch_nothing():
    from invr import _abi
    L = lib()
    err = L.invr_last_error
    a = 256                                             # a non-null address that is never dereferenced: every call stops before its launch
    nan, inf = float('nan'), float('inf')
    # invr_depth_fwd
    assert L.invr_depth_fwd(a, a, a, None, 4, 1, 0.0, 0.5, a, a, a, None) != 0 and b'invr_depth_fwd: need n_rays >= 0 and n_samples >= 2' in err()
    assert L.invr_depth_fwd(a, a, a, None, -1, 8, 0.0, 0.5, a, a, a, None) != 0 and b'invr_depth_fwd: need n_rays' in err()
    for level in (nan, inf, -inf):
        assert L.invr_depth_fwd(a, a, a, None, 4, 8, 0.0, level, a, a, a, None) != 0 and b'invr_depth_fwd: level and eps must be finite' in err()
    assert L.invr_depth_fwd(a, a, a, None, 4, 8, nan, 0.5, a, a, a, None) != 0 and b'must be finite' in err()
    assert L.invr_depth_fwd(None, a, a, None, 4, 8, 0.0, 0.5, a, a, a, None) != 0 and b'invr_depth_fwd: null occ' in err()
    assert L.invr_depth_fwd(a, None, a, None, 4, 8, 0.0, 0.5, a, a, a, None) != 0 and b'neither z_vals nor near / far' in err()
    assert L.invr_depth_fwd(a, a, None, None, 4, 8, 0.0, 0.5, a, a, a, None) != 0 and b'neither z_vals nor near / far' in err()
    assert L.invr_depth_fwd(None, None, None, None, 0, 8, 0.0, 0.5, None, None, None, None) == 0          # no rays: nothing to do
    assert L.invr_depth_fwd(a, a, a, None, 4, 8, 0.0, 0.5, None, None, None, None) == 0                   # no output asked for
    # invr_surface_stencil
    for h in (0.0, -0.01, nan, inf):
        assert L.invr_surface_stencil(a, a, a, a, 3, h, a, a, None) != 0 and b'invr_surface_stencil: h must be finite and > 0' in err(), h
    for k in (0, 1, 2, 3, 6, 7):
        args = [a, a, a, a, 3, 0.005, a, a]
        args[k] = None
        assert L.invr_surface_stencil(*args, None) != 0 and b'invr_surface_stencil: null pointer' in err(), k
    assert L.invr_surface_stencil(a, a, a, a, -1, 0.005, a, a, None) != 0 and b'invr_surface_stencil: n out of range' in err()
    assert L.invr_surface_stencil(None, None, None, None, 0, 0.005, None, None, None) == 0
    # invr_stencil_normals
    for k in (0, 1, 3, 4):
        args = [a, a, 3, a, a]
        args[k] = None
        assert L.invr_stencil_normals(*args, None) != 0 and b'invr_stencil_normals: null pointer' in err(), k
    assert L.invr_stencil_normals(a, a, -2, a, a, None) != 0 and b'invr_stencil_normals: n out of range' in err()
    assert L.invr_stencil_normals(None, None, 0, None, None, None) == 0
    # invr_render_fwd_geo: its own checks come ahead of the render's
    scene, model = _abi.InvrScene(), _abi.InvrModel()
    geo = _abi.InvrGeoOut(nan, a, a, a)
    head = (C.byref(scene), C.byref(model), a, a, a, a)
    assert L.invr_render_fwd_geo(*head, None, 4, 8, a, a, a, None, None, None, a, a, 1 << 20, 0, None, None, 0, C.byref(geo)) != 0
    assert b'invr_render_fwd_geo: level must be finite' in err()
    geo.level = 0.5
    assert L.invr_render_fwd_geo(*head, a, 4, 8, a, a, a, None, None, None, a, a, 1 << 20, 0, None, None, 0, C.byref(geo)) != 0
    assert b'invr_render_fwd_geo: a call with jitter needs z_vals' in err()
    # ... and with raw_dirty it takes the tracked call's rules
    assert L.invr_render_fwd_geo(*head, None, 4, 8, a, a, None, None, None, None, a, a, 1 << 20, 0, None, a, 32, C.byref(geo)) != 0
    assert b'invr_render_fwd_geo: null raw / raw_dirty' in err()
    assert L.invr_render_fwd_geo(*head, None, 4, 8, a, a, a, a, None, None, a, a, 1 << 20, 0, None, a, 32, C.byref(geo)) != 0
    assert b'invr_render_fwd_geo: occ and weights must be NULL' in err()
    assert L.invr_render_fwd_geo(*head, None, 4, 8, a, a, a, None, None, None, a, a, 1 << 20, 0, None, a, 31, C.byref(geo)) != 0
    assert b'invr_render_fwd_geo: raw_rows 31 < n_rays * n_samples' in err()
    assert L.invr_render_fwd_geo(*head, None, 0, 8, None, None, None, None, None, None, a, a, 1 << 20, 0, None, None, 0, C.byref(geo)) == 0          # no rays
