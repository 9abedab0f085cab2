"""Who owns device memory, pinned memory, events and streams (uav_airvision_amd/csrc/av_resources.h), without a GPU:

 * the owner itself, compiled for the CPU against a stand-in HIP runtime (tests/native/fake_hip) and run under ASan / UBSan: a
   create-like sequence once clean and once for every k with the k-th acquisition failing -- the failure is reported, the live counts
   return to zero, nothing leaks and nothing is released twice;
 * a source rule: no other file of the library acquires or releases such a resource on its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'uav_airvision_amd', 'csrc')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp('resources') / 'resources_test'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'tests', 'native', 'fake_hip'), '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'native', 'resources_harness.cpp'), '-o', str(exe)])
    return str(exe)


def test_owner_releases_everything_whichever_acquisition_fails(harness):
    out = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith('OK'), out.stdout
    assert int(out.stdout.split()[1]) > 40          # acquisitions of the clean run = failure points tried


CALLS = ('hipMalloc(', 'hipHostMalloc(', 'hipFree(', 'hipHostFree(', 'hipEventCreate', 'hipEventDestroy(', 'hipStreamCreate', 'hipStreamDestroy(')
# (file, text the line holds): the reason it may stay
ALLOWED = {
    # AV_LK_PROF's counters: allocated once behind the switch and kept for the life of the process -- a static destructor would free
    # them after the HIP runtime has gone
    ('lk.hip', 'hipMalloc(&g_lk_prof,'),
    # the DevStamps statics of AV_DEV_FPROF / AV_DEV_UPROF: the same
    ('msckf_dev_host.inc', 'hipMalloc((void**)&dev, 256)'),
}


def test_only_the_owner_acquires_and_releases():
    found, used = [], set()
    for name in sorted(os.listdir(CSRC)):
        if name == 'av_resources.h':
            continue
        for no, line in enumerate(open(os.path.join(CSRC, name), errors='replace'), 1):
            if not any(c in line for c in CALLS):
                continue
            ok = [a for a in ALLOWED if a[0] == name and a[1] in line]
            used.update(ok)
            if not ok:
                found.append('%s:%d: %s' % (name, no, line.strip()))
    assert not found, 'resources acquired or released outside av_resources.h:\n' + '\n'.join(found)
    assert used == ALLOWED, 'allow-list entries that match nothing any more: %s' % sorted(ALLOWED - used)
