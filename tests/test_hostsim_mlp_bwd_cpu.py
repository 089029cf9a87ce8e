"""CPU: the bodies of tests/test_gpu_mlp_bwd.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — k_part_mlp_bwd and k_wgrad element by element against the float64 reference, without a GPU.  Every case of
at most 5,000 pairs runs in the default CPU suite; the two persistent-loop cases (32,785 pairs, 49,452 rows) only under
HOSTSIM_FULL=1.  What the device adds — the hardware's exp2 / log2 / sin / cos / rcp pipes instead of libm, float atomics from
concurrent workgroups — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_mlp_bwd as M
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


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_mlp_bwd_persistent_loop', 'test_wgrad_persistent_loop'}
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n not in LARGE:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
