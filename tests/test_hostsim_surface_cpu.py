"""CPU: the bodies of tests/test_gpu_surface_volume.py and the tensor comparisons of tests/test_gpu_novel_subject.py on the wave machine
(tests/hostsim: the kernel SOURCES compiled for the host and executed wave by wave, one workgroup after another) — the closest point
on a mesh and the interpolation bit for bit against the contract's brute force, and a subject's canonical volumes against the host
restatement, without a GPU.  Lattices of more than 20,000 points are left out (the 33 x 16 x 65 one; the production lattice is cut to
its first 12 x 16 x 24 points, the subject's to 16 x 16 x 8) unless HOSTSIM_FULL=1; the renders of the novel subject are left to
-m gpu."""
import os

import pytest

import tests.test_gpu_novel_subject as N
import tests.test_gpu_surface_volume as V
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = V.DEV, V.MAX_POINTS, V.PRODUCTION_CROP, N.DEV, N.LATTICE_CROP
    V.DEV = N.DEV = 'cpu'
    if not FULL:
        V.MAX_POINTS, V.PRODUCTION_CROP, N.LATTICE_CROP = 20000, (12, 16, 24), (16, 16, 8)
    V.production.cache_clear()
    V.production_run.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        V.DEV, V.MAX_POINTS, V.PRODUCTION_CROP, N.DEV, N.LATTICE_CROP = old
        V.production.cache_clear()
        V.production_run.cache_clear()


for _m, _names in ((V, [n for n in dir(V) if n.startswith('test_')]), (N, N.TENSOR_TESTS)):
    for _n in _names:
        globals()['test_hostsim__' + _n[5:]] = getattr(_m, _n)
