"""CPU: the C-ABI shared library loads and exports every symbol include/invr.h declares
(no compute calls: there is no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'invr.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', src)))


def header_prototypes():
    """-> [(return type, name, [parameter declarations])] of every function include/invr.h declares, in its order."""
    src = open(os.path.join(ROOT, 'include', 'invr.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', src, flags=re.M)
    return [(ret.strip(), name, [a.strip() for a in args.split(',') if a.strip() != 'void']) for ret, name, args in protos]


def c_kind(decl):
    """Class of a C return type / parameter declaration: 'ptr', or (kind, bytes) with kind 'int' / 'uint' / 'float'."""
    import ctypes as C
    if '*' in decl or '[' in decl:
        return 'ptr'
    base = re.sub(r'\bconst\b', '', decl).split()[0]
    return {'int': ('int', C.sizeof(C.c_int)), 'int32_t': ('int', 4), 'int64_t': ('int', 8), 'uint8_t': ('uint', 1), 'uint32_t': ('uint', 4),
            'uint64_t': ('uint', 8), 'size_t': ('uint', C.sizeof(C.c_size_t)), 'float': ('float', 4), 'double': ('float', 8)}[base]


def ctypes_kind(t):
    """The same class of a ctypes type, by kind and sizeof (c_int32 is c_int and c_size_t is c_ulong on this ABI)."""
    import ctypes as C
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return 'ptr'
    code = t._type_
    assert code in 'bhilqBHILQfd', t
    return ('float' if code in 'fd' else 'int' if code.islower() else 'uint', C.sizeof(t))


def test_library_exports_header_symbols():
    from invr import _abi
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = _abi.lib()
    names = declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(L, n), n
    assert sorted(_abi.EXPORTS) == names
    assert L.invr_version() == _abi.ABI_VERSION == 2
    import re
    hdr = open(os.path.join(ROOT, 'include', 'invr.h')).read()
    assert int(re.search(r'#define INVR_ABI_VERSION (\d+)', hdr).group(1)) == _abi.ABI_VERSION
    # every declaration parses as a prototype, and the binding's one table states each with the header's types, in the header's order
    protos = header_prototypes()
    assert len(protos) == 54
    assert sorted(name for _, name, _ in protos) == names, 'an invr_ declaration of the header did not parse as a prototype'
    assert [name for _, name, _ in protos] == list(_abi.SIGNATURES) == _abi.EXPORTS
    for ret, name, params in protos:
        restype, argtypes = _abi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)


def test_signature_classes_tell_widths_apart():
    """The comparison above is by kind and size: a 32-bit type where the header says int64_t, or a float for a double, is a mismatch."""
    import ctypes as C
    assert ctypes_kind(C.c_int32) == c_kind('int32_t which') == c_kind('int') != c_kind('int64_t n')
    assert ctypes_kind(C.c_int64) == c_kind('int64_t n') != ctypes_kind(C.c_uint64) == c_kind('size_t workspace_bytes')
    assert ctypes_kind(C.c_float) == c_kind('float eps') != ctypes_kind(C.c_double) == c_kind('double beta1')
    assert ctypes_kind(C.c_int32 * 3) == c_kind('const int32_t dims[3]') == c_kind('float* const* dW') == ctypes_kind(C.POINTER(C.c_void_p)) == 'ptr'
    assert ctypes_kind(C.c_char_p) == c_kind('const char*') == 'ptr'


def default_model():
    """An InvrModel with the default layer shapes (occ 19-64-17, rgb 70-64-64-3) and no tables or weights: for calls that must stop
    at an argument check."""
    from invr import _abi
    m = _abi.InvrModel()
    for p in range(_abi.NUM_PARTS):
        part = m.part[p]
        part.occ.n_linear, part.rgb.n_linear = 2, 3
        part.occ.dims[:3] = [19, 64, 17]
        part.rgb.dims[:4] = [70, 64, 64, 3]
        part.latent_dim, part.num_latent_code = 8, 1
    m.n_dir_freq, m.geo_feature_dim = 4, 16
    return m


def test_part_mlp_backward_refuses_what_the_forward_refuses():
    """One shape rule for the part MLPs: a 70-64-32-3 colour MLP (the kernels stage a 64 x 64 middle layer) is refused by the stand-alone
    backward entry points with the forward's message, ahead of the data-pointer checks — nothing is launched."""
    import ctypes as C
    from invr import _abi
    L = _abi.lib()
    li = (C.c_int64 * 1)(0)
    out = _abi.InvrMlpBwdOut()
    cnt = (C.c_int32 * 1)(4)

    def calls(m):
        yield L.invr_part_mlp_bwd(C.byref(m), 0, li, None, None, 4, None, C.byref(out), None)
        yield L.invr_part_mlp_bwd_lists(C.byref(m), 0, li, None, None, 4, 4, cnt, None, None, C.byref(out), 0, None)
    m = default_model()
    for st in calls(m):          # the default shapes pass the rule: the call stops at its NULL data pointers
        assert st != 0 and b'null pointer' in L.invr_last_error(), L.invr_last_error()
    m.part[0].rgb.dims[2] = 32
    for st in calls(m):
        assert st != 0 and b'part MLP kernel supports occ 19-64-17 and rgb 70-64(-64)-3' in L.invr_last_error(), L.invr_last_error()


def test_workspace_query_and_error_path():
    from invr import _abi
    L = _abi.lib()
    small = L.invr_workspace_bytes(4096, 64, 0)
    big = L.invr_workspace_bytes(8192, 64, 0)
    capped = L.invr_workspace_bytes(8192, 64, 1000)
    assert 0 < small < big and capped < big
    # argument errors are reported through the status code + invr_last_error (no exceptions, no GPU touched)
    import ctypes as C
    st = L.invr_render_fwd(None, None, None, None, None, None, None, 1, 8, None, None, None, None, None, None, None,
                           None, 0, 0, None)
    assert st != 0 and b'null' in L.invr_last_error()
    st = L.invr_composite_fwd(None, 4, 0, None, None, None, None)
    assert st != 0


def test_merge_bwd_argument_checks():
    """invr_merge_bwd stops at its argument checks (nothing is launched): the merge mode, the sizes, the pointers, the workspace's size
    and alignment."""
    import ctypes as C
    from invr import _abi
    L = _abi.lib()
    need = L.invr_workspace_bytes(64, 8, 0)
    buf = C.create_string_buffer(512)
    base = (C.addressof(buf) + 255) & ~255
    g = C.cast(buf, C.c_void_p)
    for args, msg in (((4, base, need, 64, 8, 0, g, g, None), b'aggr 4'),
                      ((-1, base, need, 64, 8, 0, g, g, None), b'aggr -1'),
                      ((1, base, need, 64, 0, 0, g, g, None), b'n_samples >= 1'),
                      ((1, base, need, 1 << 26, 64, 0, g, g, None), b'< 2^31'),
                      ((1, base, need, 64, 8, 0, None, g, None), b'null g_rawfull'),
                      ((1, base, need, 64, 8, 0, g, None, None), b'null g_rawfull'),
                      ((1, None, need, 64, 8, 0, g, g, None), b'workspace too small'),
                      ((1, base, need - 1, 64, 8, 0, g, g, None), b'workspace too small'),
                      ((1, base + 16, need, 64, 8, 0, g, g, None), b'256-byte aligned')):
        assert L.invr_merge_bwd(*args) != 0 and msg in L.invr_last_error(), (args, L.invr_last_error())
    assert L.invr_merge_bwd(1, None, 0, 0, 8, 0, None, None, None) == 0          # no rays: nothing to do


def test_struct_sizes_match_header():
    """ctypes mirrors must have the C layout (checked against sizes computed from the header's field lists)."""
    import ctypes as C
    from invr import _abi
    assert C.sizeof(_abi.InvrGrid) == 3 * 8 + 4 * 4 + 8 + 16 * 4 + 16 * 4 + 16 * 8 + 3 * 4 + 4 + 8
    assert C.sizeof(_abi.InvrMlp) == 8 * 8 + 5 * 4 + 4
    assert C.sizeof(_abi.InvrPart) == C.sizeof(_abi.InvrGrid) + 2 * C.sizeof(_abi.InvrMlp) + 8 + 8
    L = _abi.lib()
    assert C.sizeof(_abi.InvrAdamTensor) == 4 * 8 + 8 + 4 * 4 + 8 + 2 * 4
    assert C.sizeof(_abi.InvrTrainGrads) == 5 * (8 + 4 * 4 * 8 + 8) + 2 * 8 + 2 * 4 * 8 + 8
    for i, t in enumerate((_abi.InvrGrid, _abi.InvrMlp, _abi.InvrPart, _abi.InvrModel, _abi.InvrScene, _abi.InvrWsLayout, _abi.InvrMlpBwdOut,
                           _abi.InvrAdamTensor, _abi.InvrTrainGrads, _abi.InvrDeformBwdOut)):
        assert L.invr_sizeof(i) == C.sizeof(t), t


def test_workspace_layout_fields_match_header():
    """InvrWsLayout, field by field: the binding lists the header's fields in the header's order (all int64_t, arrays of INVR_NUM_PARTS),
    `dslice` after `byte_off`, then the merge's inputs `pdist`, `feat`, `gcount` — appended, so that no older field moved; the library
    fills every offset inside the workspace, 256-byte aligned (gcount: behind the 16 counters, 64-byte aligned), the slice table
    DF_SLICE_MAX float2 entries long and overlapping no other exported array, pdist / feat / gcount with room for their documented
    lengths before the next exported array."""
    import ctypes as C
    from invr import _abi
    src = open(os.path.join(ROOT, 'include', 'invr.h')).read()
    body = re.search(r'typedef struct InvrWsLayout \{(.*?)\} InvrWsLayout;', src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            assert decl.startswith('int64_t '), decl
            for name in decl[len('int64_t '):].split(','):
                m = re.fullmatch(r'\s*([a-z_0-9]+)(\[INVR_NUM_PARTS\])?\s*', name)
                fields.append((m.group(1), C.c_int64 * _abi.NUM_PARTS if m.group(2) else C.c_int64))
    assert [(n, t) for n, t in _abi.InvrWsLayout._fields_] == fields
    assert [n for n, _ in fields][-5:] == ['byte_off', 'dslice', 'pdist', 'feat', 'gcount']
    arrays5 = ('l_slot', 'l_nn', 'l_w', 'l_x', 'l_d', 'l_r', 'emb', 'occp', 'wl', 'feat')
    assert [n for n, t in fields if t is not C.c_int64] == list(arrays5)
    pipeline = open(os.path.join(_abi.HERE, 'csrc', 'pipeline.h')).read()
    assert int(re.search(r'#define DF_SLICE_MAX (\d+)', pipeline).group(1)) == _abi.DF_SLICE_MAX == 4096
    L = _abi.lib()
    for n_rays, S, cap in ((1, 1, 0), (1600, 32, 0), (4096, 64, 1000)):
        lay = _abi.InvrWsLayout()
        for n, _ in fields:                                         # (a field the library does not fill keeps this)
            setattr(lay, n, (C.c_int64 * _abi.NUM_PARTS)(*[-1] * _abi.NUM_PARTS) if n in arrays5 else -1)
        assert L.invr_workspace_layout(n_rays, S, cap, C.byref(lay)) == 0
        total = L.invr_workspace_bytes(n_rays, S, cap)
        offs = []
        for n, t in fields:
            if n in ('cap', 'lcap', 'n_groups'):
                assert getattr(lay, n) > 0, n
                continue
            vals = list(getattr(lay, n)) if t is not C.c_int64 else [getattr(lay, n)]
            for v in vals:
                # (gcount shares the counters' allocation — one memset clears both: it follows them inside it)
                assert 0 <= v < total and v % (64 if n == 'gcount' else 256) == 0, (n, v, total)
            offs += vals
        assert len(set(offs)) == len(offs)

        def room(off):
            return min(o for o in offs + [total] if o > off) - off
        assert _abi.DF_SLICE_MAX * 8 <= room(lay.dslice), (lay.dslice, room(lay.dslice), total)
        lc = lay.lcap
        assert lc == lay.cap + 1 and lay.n_groups == (lc + 4095) // 4096
        assert lc * 5 * 4 <= room(lay.pdist), (lay.pdist, room(lay.pdist))
        for p in range(_abi.NUM_PARTS):
            assert lc * 4 * 16 <= room(lay.feat[p]), (p, lay.feat[p], room(lay.feat[p]))
        assert lay.counters + 16 * 4 <= lay.gcount and lay.n_groups * 5 * 4 <= room(lay.gcount), (lay.counters, lay.gcount, room(lay.gcount))


def test_product_path_has_no_cpu_route():
    """The render path is the HIP library or nothing: the binding refuses host tensors, and nothing in the product tree, bench.py or
    __graft_entry__.py knows about the test-only host build of the kernels (tests/hostsim) or imports the oracle outside bench.py's
    cpu_baseline leg / smoke()'s check."""
    import os
    import re
    import pytest
    import torch
    from invr import _abi
    with pytest.raises(AssertionError):
        _abi.ptr(torch.zeros(4))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, 'bench.py'), os.path.join(root, '__graft_entry__.py')]
    for d, _, names in os.walk(os.path.join(root, 'instant-nvr_amd')):
        files += [os.path.join(d, n) for n in names if n.endswith(('.py', '.hip', '.h'))]
    for f in files:
        text = open(f).read()
        assert 'hostsim' not in text.lower(), f
        if not f.endswith(('bench.py', '__graft_entry__.py')):
            assert not re.search(r'^\s*(from|import)\s+(oracle|tests)\b', text, re.M), f
