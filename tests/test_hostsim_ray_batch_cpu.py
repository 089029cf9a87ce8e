"""CPU: the bodies of tests/test_gpu_ray_batch.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the select of k_ray_batch (the row search in the prefix counts, the word walk, the popcount bisection), its
float64 rays and slab test and its gathers against the contract and the reference's recorded outputs, without a GPU."""
import pytest

import tests.test_gpu_ray_batch as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV
    M.DEV = 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.DEV = old


for _n in [n for n in dir(M) if n.startswith('test_')]:
    globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
