"""CPU: the bodies of tests/test_gpu_warp_in_deformer.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host
and executed wave by wave) — the pair lists of k_deform_pairs, which warps each pair itself: boundary list counts, values against the
dense entry points, nothing stored past a list, and placement independence bit for bit.  The frame with a second batch per workgroup
(more than 131,072 pairs in a part) is left to -m gpu."""
import pytest

import tests.test_gpu_warp_in_deformer as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV
    M.DEV = 'cpu'
    M._CACHE.clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.DEV = old
        M._CACHE.clear()


GPU_ONLY = {'test_second_batch_of_a_workgroup'}
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n not in GPU_ONLY:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
