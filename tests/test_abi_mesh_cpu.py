"""CPU: include/invr_mesh.h against the library and its binding table (invr._abi.SIGNATURES_MESH) — what
tests/test_abi_perceptual_cpu.py does for include/invr_perceptual.h: every declared symbol is exported, the table states each
prototype with the header's types (by kind and width) in the header's order, the layout struct mirrors the header's field list, the
workspace arrays are disjoint and aligned, and the argument checks return a status with a message and launch nothing (there is no
GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_mesh.h')
SHAPES = ((1, 1, 1), (2, 2, 2), (1, 1, 70), (70, 1, 1), (3, 5, 4), (17, 9, 33), (33, 16, 65), (15, 15, 15), (4, 4, 4))


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


def f3(*v):
    return (C.c_float * 3)(*v)


def test_library_exports_mesh_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 5 and sorted(n for _, n, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_MESH)
    assert not set(_abi.SIGNATURES_MESH) & (set(_abi.SIGNATURES) | set(_abi.SIGNATURES_PERCEPTUAL))          # the other tables are untouched
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_MESH[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)


def test_layout_struct_mirrors_the_header():
    from invr import _abi
    body = re.search(r'typedef struct InvrMeshLayout \{(.*?)\} InvrMeshLayout;', header_text(), re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            assert decl.startswith('int64_t '), decl
            fields += [f.strip() for f in decl[len('int64_t '):].split(',')]
    assert fields == [k for k, _ in _abi.InvrMeshLayout._fields_]
    assert all(t is C.c_int64 for _, t in _abi.InvrMeshLayout._fields_)
    assert int(re.search(r'#define INVR_MESH_SCAN_ITEMS (\d+)', open(HEADER).read()).group(1)) == 4096


def test_workspace_layout_is_disjoint_aligned_and_sized():
    from invr import _abi
    L = lib()
    for dims in SHAPES:
        lay = _abi.InvrMeshLayout()
        assert L.invr_mesh_workspace_layout(i3(*dims), C.byref(lay)) == 0
        n = (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2)
        assert lay.n_points == n and lay.n_blocks == (n + 4095) // 4096
        size = {'masks': n, 'tcounts': n, 'voffsets': 4 * n, 'toffsets': 4 * n, 'counts': 32, 'partials': 8 * lay.n_blocks}
        end = 0
        for k in _abi.InvrMeshLayout.ARRAYS:
            off = getattr(lay, k)
            assert off % 256 == 0 and off >= end, (dims, k)
            end = off + size[k]
        assert end <= lay.bytes == L.invr_mesh_workspace_bytes(i3(*dims))


def test_size_limit():
    L = lib()
    assert L.invr_mesh_workspace_bytes(i3(510, 510, 510)) > 0                   # 512^3 = 2^27 padded points: the limit itself
    assert L.invr_mesh_workspace_bytes(i3(511, 510, 510)) == 0
    assert L.invr_mesh_workspace_bytes(i3(0, 4, 4)) == 0 and L.invr_mesh_workspace_bytes(i3(4, 4, -1)) == 0
    assert L.invr_mesh_workspace_bytes(i3(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)) == 0


def test_argument_checks_return_a_status_and_launch_nothing():
    from invr import _abi
    L = lib()
    err = L.invr_last_error
    lay = _abi.InvrMeshLayout()
    dims, big = i3(3, 5, 4), i3(511, 510, 510)
    assert L.invr_mesh_workspace_layout(dims, None) != 0 and b'null layout' in err()
    assert L.invr_mesh_workspace_layout(i3(3, 0, 4), C.byref(lay)) != 0 and b'every dimension must be >= 1' in err()
    assert L.invr_mesh_workspace_layout(big, C.byref(lay)) != 0 and b'more than 2^27 padded points' in err()
    a = 256                                             # a non-null, aligned address that is never dereferenced: every call stops before its launch
    nb = L.invr_mesh_workspace_bytes(dims)
    o, v = f3(0, 0, 0), f3(1, 1, 1)
    for level, what in ((0.0, b'level must be finite and > 0'), (-0.1, b'level must be'), (float('nan'), b'level must be'), (float('inf'), b'level must be')):
        assert L.invr_mesh_count(a, dims, level, a, nb, a, None) != 0 and b'invr_mesh_count: ' + what in err(), level
        assert L.invr_mesh_emit(a, dims, o, v, level, a, nb, a, 1, a, 1, a, None) != 0 and b'invr_mesh_emit: ' + what in err(), level
    assert L.invr_mesh_count(a, i3(3, 5, 0), 0.1, a, nb, a, None) != 0 and b'invr_mesh_count: every dimension' in err()
    assert L.invr_mesh_count(a, big, 0.1, a, nb, a, None) != 0 and b'invr_mesh_count: more than 2^27' in err()
    for args in ((None, dims, 0.1, a, nb, a), (a, dims, 0.1, None, nb, a), (a, dims, 0.1, a, nb, None)):
        assert L.invr_mesh_count(*args, None) != 0 and b'invr_mesh_count: null volume / workspace / counts' in err()
    assert L.invr_mesh_count(a, dims, 0.1, a + 64, nb, a, None) != 0 and b'256-byte aligned' in err()
    assert L.invr_mesh_count(a, dims, 0.1, a, nb - 1, a, None) != 0 and b'workspace too small' in err()
    assert L.invr_mesh_emit(a, dims, o, v, 0.1, a, nb - 1, a, 1, a, 1, a, None) != 0 and b'invr_mesh_emit: workspace too small' in err()
    assert L.invr_mesh_emit(a, dims, o, v, 0.1, a + 128, nb, a, 1, a, 1, a, None) != 0 and b'256-byte aligned' in err()
    assert L.invr_mesh_emit(a, dims, o, v, 0.1, a, nb, None, 1, a, 1, a, None) != 0 and b'null vertices / triangles' in err()
    assert L.invr_mesh_emit(a, dims, o, v, 0.1, a, nb, a, 1, None, 1, a, None) != 0 and b'null vertices / triangles' in err()
    assert L.invr_mesh_emit(a, dims, o, v, 0.1, a, nb, a, -1, a, 1, a, None) != 0 and b'negative capacity' in err()
    assert L.invr_mesh_emit(a, dims, o, f3(1, 0, 1), 0.1, a, nb, a, 1, a, 1, a, None) != 0 and b'voxel must be finite and > 0' in err()
    assert L.invr_grid_points(o, v, dims, 0, 61, a, None) != 0 and b'leaves the grid' in err()
    assert L.invr_grid_points(o, v, dims, -1, 4, a, None) != 0 and b'leaves the grid' in err()
    assert L.invr_grid_points(o, v, dims, 0, 60, None, None) != 0 and b'null xyz' in err()
    assert L.invr_grid_points(o, v, i3(0, 1, 1), 0, 0, a, None) != 0 and b'invr_grid_points: every dimension' in err()
    assert L.invr_grid_points(o, v, dims, 60, 0, None, None) == 0          # nothing to write
