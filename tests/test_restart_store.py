"""The store half of the stream restart (include/airvision.h, "Stream restart"): avs_restart of uav_airvision_amd/csrc/msckf_store.h --
the function the kernel dk_restart calls, here compiled for the CPU with a one-thread team -- applied to a store whose frame slots,
feature table, free stack, insertion counter and overflow word are all in use.  Check one: every persistent array equals a newly allocated
store's.  Check two: a second random message sequence replayed into both leaves identical arrays and identical results after every frame.
Under ASan / UBSan, as a stand-alone program: no GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'uav_airvision_amd', 'csrc')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp('restart_store')
    exe = d / 'restart_store_test'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'restart_harness.cpp'), '-o', str(exe)])
    return str(exe)


@pytest.mark.parametrize('seed,before,after,per', [(1, 60, 80, 40), (2, 45, 60, 150), (3, 90, 90, 5), (4, 33, 50, 300)])
def test_a_restarted_store_is_a_new_store(harness, seed, before, after, per):
    out = subprocess.run([harness, str(seed), str(before), str(after), str(per)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('OK'), out.stdout
    assert int(out.stdout.split()[1]) > 18 * after


def test_the_kernel_calls_the_function_the_harness_checks():
    """dk_restart resets the store through avs_restart and nothing else: one function, shared by the device and the CPU model."""
    dev = open(os.path.join(CSRC, 'msckf_dev.inc')).read()
    body = dev[dev.index('void dk_restart('):]
    body = body[:body.index('\n}\n')]
    assert 'avs_restart(T, dev_store(a, s))' in body
    for own in ('fr_n[', 'pos_of[', 'births', 'hdr['):
        assert own not in body, own
    assert 'atomic' not in body and '__shared__' not in body
    assert 'AVS_FN void avs_restart(' in open(os.path.join(CSRC, 'msckf_store.h')).read()
