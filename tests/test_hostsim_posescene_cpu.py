"""CPU: the bodies of tests/test_gpu_distance_volume.py and the tensor comparisons of tests/test_gpu_posescene.py on the wave machine
(tests/hostsim: the kernel SOURCES compiled for the host and executed wave by wave, one workgroup after another) — the distance
volume bit for bit against the contract's brute force and a posed frame's scene tensors against the host restatement, without a GPU.
Lattices of more than 20,000 points are left out (the 33 x 16 x 65 one; the production lattice is cut to its first 20 x 40 x 24
points) unless HOSTSIM_FULL=1; the renders of the posed frames are left to -m gpu."""
import os

import pytest

import tests.test_gpu_distance_volume as D
import tests.test_gpu_posescene as P
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))
posed, reference_volume = P.posed, P.reference_volume          # the fixtures of the bodies below


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = D.DEV, D.MAX_POINTS, D.PRODUCTION_CROP, P.DEV, P.LATTICE_CROP
    D.DEV = P.DEV = 'cpu'
    if not FULL:
        D.MAX_POINTS, D.PRODUCTION_CROP, P.LATTICE_CROP = 20000, (20, 40, 24), (40, 20, 24)
    D.production.cache_clear()
    D.production_run.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        D.DEV, D.MAX_POINTS, D.PRODUCTION_CROP, P.DEV, P.LATTICE_CROP = old
        D.production.cache_clear()
        D.production_run.cache_clear()


for _m, _names in ((D, [n for n in dir(D) if n.startswith('test_')]), (P, P.TENSOR_TESTS)):
    for _n in _names:
        globals()['test_hostsim__' + _n[5:]] = getattr(_m, _n)
