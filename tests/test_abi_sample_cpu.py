"""CPU: include/invr_sample.h against the library and its binding table (invr._abi.SIGNATURES_SAMPLE) — what tests/test_abi_batch_cpu.py
does for include/invr_batch.h: the declared symbol is exported, the table states the prototype with the header's types (by kind and
width) in the header's order under names disjoint from the other tables, include/invr.h's own table and ABI version are untouched, and
the argument checks return a status with a message and launch nothing (there is no GPU here)."""
import ctypes as C
import os
import re

from tests.test_abi_symbols import ROOT, c_kind, ctypes_kind

HEADER = os.path.join(ROOT, 'include', 'invr_sample.h')


def header_text():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return re.sub(r'//[^\n]*', '', src)


def header_prototypes():
    protos = re.findall(r'^[ \t]*((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*(invr_[a-z_0-9]+)\s*\(([^;{)]*)\)\s*;', header_text(), flags=re.M)
    return [(ret.strip(), name, [' '.join(a.split()) for a in args.split(',') if a.strip() != 'void']) for ret, name, args in protos]


def lib():
    from invr import _abi
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _abi.lib()


def test_library_exports_sample_header_symbols():
    from invr import _abi
    L = lib()
    names = sorted(set(re.findall(r'\b(invr_[a-z_0-9]+)\s*\(', header_text())))
    protos = header_prototypes()
    assert len(protos) == 1 and sorted(n for _, n, _ in protos) == names == ['invr_ray_batch'], 'an invr_ declaration of the header did not parse'
    assert [n for _, n, _ in protos] == list(_abi.SIGNATURES_SAMPLE)
    others = set(_abi.SIGNATURES) | set(_abi.SIGNATURES_PERCEPTUAL) | set(_abi.SIGNATURES_MESH) | set(_abi.SIGNATURES_BATCH)
    assert not set(_abi.SIGNATURES_SAMPLE) & others                                    # the other tables are untouched
    assert list(_abi.SIGNATURES_BATCH) == ['invr_patch_batch']
    assert _abi.EXPORTS == list(_abi.SIGNATURES) and L.invr_version() == _abi.ABI_VERSION == 2
    for ret, name, params in protos:
        assert hasattr(L, name), name
        restype, argtypes = _abi.SIGNATURES_SAMPLE[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name          # lib() applied the table
        assert ctypes_kind(restype) == c_kind(ret), (name, 'return type', ret, restype)
        assert len(argtypes) == len(params) == 20, (name, params, argtypes)
        for i, (decl, t) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(t) == c_kind(decl), (name, i, decl, t)
    from invr import trainset
    assert int(re.search(r'#define INVR_RAY_BATCH_MAX (\d+)', open(HEADER).read()).group(1)) == 1048576 == trainset.MAX_RAYS


def test_invr_h_does_not_declare_it():
    hdr = open(os.path.join(ROOT, 'include', 'invr.h')).read() + open(os.path.join(ROOT, 'include', 'invr_batch.h')).read()
    assert 'invr_ray_batch' not in hdr and 'INVR_RAY_BATCH_MAX' not in hdr
    assert int(re.search(r'#define INVR_ABI_VERSION (\d+)', hdr).group(1)) == 2


def test_build_lists_the_source_and_the_header():
    from invr import build
    assert 'k_sample.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'k_sample.hip'))
    assert os.path.abspath(HEADER) in [os.path.abspath(h) for h in build.headers()]


def test_argument_checks_return_a_status_and_launch_nothing():
    L = lib()
    err = L.invr_last_error
    a = 256                                             # a non-null address that is never dereferenced: every call stops before its launch
    kinv, bounds = (C.c_double * 9)(*[1, 0, 0, 0, 1, 0, 0, 0, 1]), (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    R, T, o = (C.c_double * 9)(*[1, 0, 0, 0, 1, 0, 0, 0, 1]), (C.c_double * 3)(0, 0, 3), (C.c_double * 3)(0, 0, -3)

    def call(img=a, occ=a, planes=a, prefix=a, H=96, W=80, sel=a, n=16, kinv=kinv, R=R, T=T, o=o, bounds=bounds, outs=(a,) * 6):
        return L.invr_ray_batch(img, occ, planes, prefix, H, W, sel, n, kinv, R, T, o, bounds, *outs, None)

    assert call(img=None) != 0 and b'invr_ray_batch: null img / occ_msk' in err()
    assert call(occ=None) != 0 and b'null img / occ_msk' in err()
    for k in ('planes', 'prefix', 'sel'):
        assert call(**{k: None}) != 0 and b'invr_ray_batch: null planes / row_prefix / sel' in err(), k
    for k in ('kinv', 'R', 'T', 'o', 'bounds'):
        assert call(**{k: None}) != 0 and b'null k_inv / R / T / cam_o / bounds' in err(), k
    for i in range(6):
        assert call(outs=(a,) * i + (None,) + (a,) * (5 - i)) != 0 and b'invr_ray_batch: null output' in err(), i
    assert call(H=0) != 0 and b'at least 1 x 1' in err()
    assert call(W=-3) != 0 and b'at least 1 x 1' in err()
    for n in (0, -1, 1048577, 2 ** 31 - 1):
        assert call(n=n) != 0 and b'n must be in 1..1048576' in err(), n
