"""The landmark record of include/airvision.h ("Landmark map") as the C compiler lays it out, against its ctypes and NumPy mirrors and
the Python constants (CPU: compiles a probe, no GPU call)."""
import ctypes
import os
import subprocess
import tempfile

from conftest import ROOT


def test_landmark_record_and_constants_match_the_header():
    from uav_airvision_amd import _native as N
    from uav_airvision_amd import msckf_ops as M
    probe = ('#include "airvision.h"\n#include <stdio.h>\n#include <stddef.h>\n'
             'int main(){printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(av_landmark), offsetof(av_landmark, id), offsetof(av_landmark, p), '
             'offsetof(av_landmark, flags), offsetof(av_landmark, n_obs), AV_LANDMARK_BYTES, AV_LM_USED, AV_LM_REJECTED, AV_LM_TRACKED, AV_LM_NEW);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'p.c'); exe = os.path.join(d, 'p')
        open(c, 'w').write(probe)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == v[5] == 40 == ctypes.sizeof(N.Landmark) == M.LANDMARK_DTYPE.itemsize
    offs = [N.Landmark.id.offset, N.Landmark.p.offset, N.Landmark.flags.offset, N.Landmark.n_obs.offset]
    assert v[1:5] == offs == [M.LANDMARK_DTYPE.fields[f][1] for f in ('id', 'p', 'flags', 'n_obs')]
    assert v[6:] == [M.LM_USED, M.LM_REJECTED, M.LM_TRACKED, M.LM_NEW] == [1, 2, 4, 8]
    for name in ('av_msckf_batch_set_landmarks', 'av_msckf_batch_next_landmarks'):
        assert name in N.SIGNATURES and hasattr(ctypes.CDLL(N.LIB_PATH), name)


def test_unpack_landmarks_returns_the_written_records():
    import numpy as np
    from uav_airvision_amd.msckf_ops import LANDMARK_DTYPE, unpack_landmarks
    rec = np.zeros((2, 4), LANDMARK_DTYPE)
    rec['id'] = np.arange(8).reshape(2, 4)
    n = np.array([[6, 4], [2, 2]], np.int32)
    assert unpack_landmarks(rec, n, 0)['id'].tolist() == [0, 1, 2, 3] and unpack_landmarks(rec, n, 1)['id'].tolist() == [4, 5]
