"""CPU: the bodies of tests/test_gpu_encoder_fwd.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the encoder forward kernels element by element against the float64 reference, without a GPU.  The large
cases and the families with 134 / 336 MB tables run only under HOSTSIM_FULL=1; everything else, n = 1000 included, is in the default
CPU suite (under a minute).  What the device adds — 2048 concurrent workgroups on 8 XCDs, real LDS banks — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_encoder_fwd as E
from tests import encoder_cases as EC
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))


def default_run(case):
    tag, cloud, n = case[:3]
    return FULL or tag not in EC.BIG_TABLES


PART = [c for c in E.PART if default_run(c)]
GENERIC = [c for c in E.GENERIC if default_run(c)]


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = E.DEV
    E.DEV = 'cpu'
    E.device_grid.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        E.DEV = old
        E.device_grid.cache_clear()


@pytest.mark.parametrize('tag,cloud,n', PART, ids=E.ids(PART))
def test_hostsim__encoder_fwd_part(tag, cloud, n):
    E.run_part_case(tag, cloud, n)


@pytest.mark.parametrize('tag,cloud,n', GENERIC, ids=E.ids(GENERIC))
def test_hostsim__encoder_fwd_generic(tag, cloud, n):
    E.test_encoder_fwd_generic(tag, cloud, n)


if FULL:                                                                       # n = 65,836 / 524,325 on the wave machine
    test_hostsim__encoder_fwd_large = E.test_encoder_fwd_large


test_hostsim__families_reach_the_intended_routes = E.test_families_reach_the_intended_routes
test_hostsim__encoder_fwd_exact_division_beside_the_reciprocal_form = E.test_encoder_fwd_exact_division_beside_the_reciprocal_form
test_hostsim__encoder_fwd_five_parts_one_launch = E.test_encoder_fwd_five_parts_one_launch
test_hostsim__encoder_fwd_all_refuses_bad_arguments = E.test_encoder_fwd_all_refuses_bad_arguments
test_hostsim__grid_row_sums_elementwise = E.test_grid_row_sums_elementwise


def test_hostsim_encoder_fwd_does_not_depend_on_lane_or_wave_order():
    """k_part_encode hands the level sums of a tile between the lanes of a wave through wave-private LDS with only a wave-barrier
    annotation, and the XCD kernel stages a dense level for the whole workgroup between two barriers: a handful of cases again with the
    lanes in a pseudo-random order and the waves reversed (a separate process: the order is fixed when the library loads)."""
    import subprocess
    import sys
    env = dict(os.environ, HOSTSIM_LANE_ORDER='shuffle:7', HOSTSIM_WAVE_ORDER='reverse')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                        'part-small-rays-64 or part-small-one-65 or part-prod-ties-1000 or part-base16-faces-63 or part-t9-ties-63 or '
                        'five_parts and 300-0-1-700-256 or exact_division and part-small'],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'no tests ran' not in r.stdout, r.stdout[-500:]
