"""CPU: the bodies of tests/test_gpu_deform_bwd.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — k_deform_bwd, k_wgrad with the deformer's three jobs and k_deform_slice_bwd / the generic table backward
element by element against the float64 reference, without a GPU.  Every case of at most 5,000 entries runs in the default CPU suite;
the three persistent-loop cases (49,452 / 263,144 / 524,805 entries) only under HOSTSIM_FULL=1.  What the device adds — the
hardware's exp2 / log2 / rcp pipes instead of libm, float atomics from concurrent workgroups — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_deform_bwd as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV
    M.DEV = 'cpu'
    M._dev_model.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.DEV = old
        M._dev_model.cache_clear()


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_deform_bwd_persistent_loop'}
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n not in LARGE:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
