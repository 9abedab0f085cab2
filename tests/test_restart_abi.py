"""The two stream-restart entries of include/airvision.h ("Stream restart"): declared, exported and bound with the same signature, their
argument checks run without a device, and every layer above them has its `restart` (CPU: no GPU call)."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

from conftest import ROOT

ENTRIES = {'av_msckf_batch_restart': 'int av_msckf_batch_restart(av_msckf_batch* b, const int32_t* stream_idx, int n);',
           'av_frontend_restart': 'int av_frontend_restart(av_frontend* fe, const int32_t* stream_idx, int n, void* stream);'}


def _header():
    return open(os.path.join(ROOT, 'include', 'airvision.h')).read()


def test_header_exports_and_ctypes_rows_agree():
    from uav_airvision_amd import _native as N
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    flat = re.sub(r'\s+', ' ', src)
    lib = ctypes.CDLL(N.LIB_PATH)
    P = ctypes.c_void_p
    rows = {'av_msckf_batch_restart': (ctypes.c_int, [P, P, ctypes.c_int]), 'av_frontend_restart': (ctypes.c_int, [P, P, ctypes.c_int, P])}
    for name, decl in ENTRIES.items():
        assert decl in flat, name
        assert hasattr(lib, name), 'missing export: ' + name
        assert N.SIGNATURES[name] == rows[name], name
    # the declarations compile as C and have the types the table gives them
    probe = ('#include "airvision.h"\n'
             'int (*f0)(av_msckf_batch*, const int32_t*, int) = av_msckf_batch_restart;\n'
             'int (*f1)(av_frontend*, const int32_t*, int, void*) = av_frontend_restart;\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'p.c')
        open(c, 'w').write(probe)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', c, '-o', os.path.join(d, 'p.o')])


def test_the_contract_is_written_down():
    text = _header()
    sec = text[text.index('/* Stream restart:'):text.index('int  av_msckf_batch_restart(')]
    for must in ('Not reset', 'av_msckf_batch_counters', 'bit for bit', 'Nothing is allocated', '200 new samples', 'generation',
                 'av_frontend_prestage', 'masks', 'frame store'):
        assert must in sec, must


def test_argument_checks_run_without_a_device():
    from uav_airvision_amd import _native as N
    lib = N.lib()
    idx = (ctypes.c_int32 * 2)(0, 1)
    assert lib.av_msckf_batch_restart(None, idx, 2) == N.AV_E_INVALID
    assert b'av_msckf_batch_restart' in lib.av_last_error()
    assert lib.av_frontend_restart(None, idx, 2, None) == N.AV_E_INVALID
    assert b'av_frontend_restart' in lib.av_last_error()
    assert lib.av_msckf_batch_restart(None, None, 0) == N.AV_E_INVALID and lib.av_frontend_restart(None, None, 0, None) == N.AV_E_INVALID


def test_every_layer_has_its_restart():
    import sys
    drop = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if drop not in sys.path:
        sys.path.insert(0, drop)
    from image_processing import ImageProcessor
    from msckf import MSCKF
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    for cls in (BatchedMSCKF, FrontendEngine, EngineSet, FilterSet):
        assert list(inspect.signature(cls.restart).parameters) == ['self', 'streams'], cls
    for cls in (MSCKF, ImageProcessor):
        assert list(inspect.signature(cls.restart).parameters) == ['self'], cls
        assert isinstance(inspect.getattr_static(cls, 'generation'), property), cls
    for cls in (EngineSet, FilterSet):
        assert isinstance(inspect.getattr_static(cls, 'generation'), property), cls
