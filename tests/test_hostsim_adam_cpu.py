"""CPU: the bodies of tests/test_gpu_adam_step.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and executed
wave by wave) — the fused Adam step element by element against the float64 reference, without a GPU.  Every case of at most 200,000
elements runs in the default CPU suite, the larger ones under HOSTSIM_FULL=1.  What the device adds — the gfx950 code of the fp32
divide and square root, the double pow of invr_adam_advance, nontemporal float4 stores — is left to -m gpu.
(tests/test_adam_cases_cpu.py holds the checker to account on its own, without any kernel.)"""
import os

import pytest

import tests.test_gpu_adam_step as A
from tests.hostsim import harness

BORROWED = [A]


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = [m.DEV for m in BORROWED]
    for m in BORROWED:
        m.DEV = 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        for m, d in zip(BORROWED, old):
            m.DEV = d


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_adam_step_single_large', 'test_adam_step_row_scalar_gradient_large'}
for _m in BORROWED:
    for _n in [n for n in dir(_m) if n.startswith('test_')]:
        if _n not in LARGE:
            globals()['test_hostsim__' + _n[5:]] = getattr(_m, _n)
