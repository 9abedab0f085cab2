"""The innovation-statistics record of include/airvision.h ("Innovation statistics") as the C compiler lays it out, against its ctypes
and NumPy mirrors, the reference's dtype and the Python constants (CPU: compiles a probe, no GPU call)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

FIELDS = ('n_cand', 'n_pos', 'n_eval', 'n_pass', 'dof_eval', 'dof_pass', 'rows', 'flags', 'gamma_eval', 'gamma_pass', 'dx_pos', 'dx_rot')


def test_stats_record_and_constants_match_the_header():
    import filter_stats_ref as R
    from uav_airvision_amd import _native as N
    from uav_airvision_amd import msckf_ops as M
    probe = ('#include "airvision.h"\n#include <stdio.h>\n#include <stddef.h>\n'
             'int main(){printf("%zu %zu %zu %d %d %d", sizeof(av_filter_stats), sizeof(av_update_stats), offsetof(av_filter_stats, upd[1]), '
             'AV_FILTER_STATS_BYTES, AV_FS_RAN, AV_FS_CUT);\n'
             + ''.join('printf(" %%zu", offsetof(av_update_stats, %s));' % f for f in FIELDS) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'p.c'); exe = os.path.join(d, 'p')
        open(c, 'w').write(probe)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v[0] == v[3] == 128 == ctypes.sizeof(N.FilterStats) == 2 * M.FILTER_STATS_DTYPE.itemsize == M.FILTER_STATS_BYTES
    assert v[1] == v[2] == 64 == ctypes.sizeof(N.UpdateStats) == N.FilterStats.upd.size // 2
    assert v[4:6] == [M.FS_RAN, M.FS_CUT] == [R.FS_RAN, R.FS_CUT] == [1, 2]
    offs = [getattr(N.UpdateStats, f).offset for f in FIELDS]
    assert v[6:] == offs == [M.FILTER_STATS_DTYPE.fields[f][1] for f in FIELDS] == [R.STATS_DTYPE.fields[f][1] for f in FIELDS]
    assert M.FILTER_STATS_DTYPE.names == FIELDS and M.FILTER_STATS_DTYPE == R.STATS_DTYPE
    assert np.zeros((3, 2), M.FILTER_STATS_DTYPE).nbytes == 3 * 128
    for name in ('av_msckf_batch_set_stats', 'av_msckf_batch_next_stats'):
        assert name in N.SIGNATURES and hasattr(ctypes.CDLL(N.LIB_PATH), name)


def test_unpack_filter_stats_normalises_both_ways_and_marks_empty_blocks():
    from uav_airvision_amd.msckf_ops import FILTER_STATS_DTYPE, filter_stats_rows, unpack_filter_stats
    rec = np.zeros((2, 2), FILTER_STATS_DTYPE)
    # stream 0: four lost features of 4, 4, 4 and 3 observations (dof 3 + 3 + 3 + 2), one rejected; two pruning candidates, both accepted
    rec[0, 0] = (5, 4, 4, 3, 11, 9, 39, 1, 24.0, 12.0, 0.01, 0.002)
    rec[0, 1] = (2, 2, 2, 2, 4, 4, 10, 1, 5.0, 5.0, 0.001, 0.0)
    u = unpack_filter_stats(rec)
    rows_eval, rows_pass = filter_stats_rows(rec)
    assert rows_eval.tolist() == [[48, 10], [0, 0]] and rows_pass.tolist() == [[39, 10], [0, 0]] and (rows_pass == rec['rows']).all()
    assert u['nis_dof'][0].tolist() == [24.0 / 11, 5.0 / 4] and u['nis_rows'][0].tolist() == [24.0 / 48, 5.0 / 10]
    assert u['reject_rate'][0].tolist() == [0.25, 0.0] and u['rows_eval'].tolist() == rows_eval.tolist()
    for n in ('nis_dof', 'nis_rows', 'reject_rate'):
        assert np.isnan(u[n][1]).all() and u[n].shape == (2, 2)
    assert u['n_cand'].tolist() == [[5, 2], [0, 0]] and u['gamma_pass'][0, 0] == 12.0


def test_sweep_helpers_format_a_line_and_sum_a_run():
    from uav_airvision_amd.msckf_ops import FILTER_STATS_DTYPE
    from uav_airvision_amd.sweep import format_nis_line, innovation_summary
    rec = np.zeros((2, 2), FILTER_STATS_DTYPE)
    rec[0, 0] = (5, 4, 4, 3, 11, 9, 39, 1, 24.0, 12.0, 0.01, 0.002)
    rec[1, 1] = (2, 2, 2, 2, 4, 4, 10, 1, 5.0, 5.0, 0.001, 0.0)
    tok = format_nis_line(12.5, rec[0]).split()
    assert len(tok) == 25 and float(tok[0]) == 12.5 and [int(t) for t in tok[1:17]] == [5, 4, 4, 3, 11, 9, 39, 1] + [0] * 8
    assert [float(t) for t in tok[17:]] == [24.0, 12.0, 0.01, 0.002, 0.0, 0.0, 0.0, 0.0]
    s = innovation_summary(rec)
    assert s == dict(nis_rows=29.0 / 58, reject_rate=1.0 - 5 / 6)
    assert innovation_summary(rec[:0]) == dict(nis_rows=None, reject_rate=None)
