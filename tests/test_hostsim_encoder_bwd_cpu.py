"""CPU: the bodies of tests/test_gpu_encoder_bwd.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the encoder backward kernels element by element against the float64 reference, without a GPU — and of
tests/test_gpu_train_stages.py (distortion regulariser, training objective).  Every case
with n <= 20,000 runs in the default CPU suite; the large-n cases (tile lengths 32 / 64, the persistent grid looping: 38 s of kernel
time for n = 132,000) only under HOSTSIM_FULL=1.  What the device adds — real float atomics from 512 concurrent workgroups,
compare-and-swap races on the cache slots — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_encoder_bwd as E
import tests.test_gpu_train_stages as S              # (the small training-side entry points: distortion, objective)
from tests.hostsim import harness

BORROWED = [E, S]


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = [m.DEV for m in BORROWED]
    for m in BORROWED:
        m.DEV = 'cpu'
    E._dev_tables.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        for m, d in zip(BORROWED, old):
            m.DEV = d
        E._dev_tables.cache_clear()


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_encoder_bwd_large', 'test_encoder_bwd_lists_large'}
for _m in BORROWED:
    for _n in [n for n in dir(_m) if n.startswith('test_')]:
        if _n not in LARGE:
            globals()['test_hostsim__' + _n[5:]] = getattr(_m, _n)


def test_hostsim_encoder_bwd_does_not_depend_on_lane_or_wave_order():
    """k_part_encode_bwd hands sgx / sgo between the lanes of a wave through LDS with only wave-barrier annotations; the generic
    kernel shares LDS accumulators between the waves of a workgroup: a few cases of each again with the lanes in a pseudo-random
    order and the waves reversed (a separate process: the order is fixed when the library loads)."""
    import subprocess
    import sys
    env = dict(os.environ, HOSTSIM_LANE_ORDER='shuffle:7', HOSTSIM_WAVE_ORDER='reverse')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                        'part-small-rays-1000 or part-small-uniform-65 or part-prod-one-1000 or part-onetable-far-1000 or '
                        'deformer-far-1023 or rowscalar-generic-rays-1024 or lists and part-small-17'],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
