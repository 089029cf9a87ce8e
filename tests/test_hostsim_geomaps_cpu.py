"""CPU: the bodies of checks 1 to 4 of tests/test_gpu_geomaps.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the
host and executed wave by wave) — the dense depth and first crossing against the contract, the depth pass behind a render against the
dense form bit for bit in both survivor orders and every kernel path, the stencil and the normals, without a GPU.  Cut for the wave
machine: the frame of check 2 is 32 x 32 instead of 64 x 64 (the same paths: S = 128 / 64 words kernel and windowed order, 32 generic
and windowed, 24 generic and ray-major, aggr 'mean', random_bg, max_active below the survivor count).  What the device adds — concurrent
workgroups, frames in flight — and the host layer (checks 5 and 6) are left to -m gpu."""
import pytest

import tests.test_gpu_geomaps as G
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = (G.DEV, G.RES)
    G.DEV, G.RES = 'cpu', 32
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        G.DEV, G.RES = old


for _n in ('test_dense_depth_and_first_crossing', 'test_dense_depth_from_a_jittered_z_vals_pointer', 'test_any_dense_output_may_be_null',
           'test_depth_pass_behind_a_render_equals_the_dense_form', 'test_depth_pass_with_overflowed_survivors_reads_zeros',
           'test_stencil_points_and_directions', 'test_normals_on_synthetic_sextuples'):
    globals()['test_hostsim__' + _n[5:]] = getattr(G, _n)
