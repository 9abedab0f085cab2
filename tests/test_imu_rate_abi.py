"""The IMU-rate record of include/airvision.h ("IMU-rate odometry") as the C compiler lays it out, against its ctypes and NumPy mirrors;
the symbols; and the refusals that need no batch (CPU: compiles a probe, no kernel is launched)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

FIELDS = ('t', 'p', 'q', 'v', 'w')


def test_record_and_symbols_match_the_header():
    from uav_airvision_amd import _native as N
    from uav_airvision_amd import msckf_ops as M
    probe = ('#include "airvision.h"\n#include <stdio.h>\n#include <stddef.h>\n'
             'int main(){printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(av_imu_state), offsetof(av_imu_state, t), offsetof(av_imu_state, p), '
             'offsetof(av_imu_state, q), offsetof(av_imu_state, v), offsetof(av_imu_state, w), AV_IMU_STATE_BYTES);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'p.c'); exe = os.path.join(d, 'p')
        open(c, 'w').write(probe)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == v[6] == 112 == ctypes.sizeof(N.ImuState) == M.IMU_STATE_DTYPE.itemsize
    assert v[1:6] == [getattr(N.ImuState, f).offset for f in FIELDS] == [M.IMU_STATE_DTYPE.fields[f][1] for f in FIELDS] == [0, 8, 32, 64, 88]
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ('av_msckf_batch_set_imu_rate', 'av_msckf_batch_next_imu_rate', 'av_msckf_predict_ops_dev_rate'):
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert len(N.SIGNATURES['av_msckf_predict_ops_dev_rate'][1]) == len(N.SIGNATURES['av_msckf_predict_ops_dev'][1]) + 3


def test_unpack_imu_states_returns_the_written_records():
    from uav_airvision_amd.msckf_ops import IMU_STATE_DTYPE, unpack_imu_states
    rec = np.zeros((2, 4), IMU_STATE_DTYPE)
    rec['t'] = np.arange(8).reshape(2, 4)
    n = np.array([[6, 4], [2, 2]], np.int32)
    assert unpack_imu_states(rec, n, 0)['t'].tolist() == [0, 1, 2, 3] and unpack_imu_states(rec, n, 1)['t'].tolist() == [4, 5]


def test_calls_without_a_batch_are_refused_with_a_text():
    """No batch, a cap outside 0 .. 4096, no destination: AV_E_INVALID and a text that names the call, before anything is touched.  (The
    refusals that need a batch -- after the first step, next without set -- are in tests/test_gpu_imu_rate.py:
    creating a batch needs a device.)"""
    from uav_airvision_amd import _native as N
    lib = N.lib()
    for cap in (-1, 0, 32, 4097):
        assert lib.av_msckf_batch_set_imu_rate(None, cap) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_imu_rate' in lib.av_last_error()
    assert lib.av_msckf_batch_next_imu_rate(None, None, None) == N.AV_E_INVALID
    assert b'av_msckf_batch_next_imu_rate' in lib.av_last_error()
