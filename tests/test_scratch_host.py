"""The owner of device buffers (optiml_amd/csrc/bq_scratch.h: bq_scratch for a one-shot entry point, bq_owner as a member of a
long-lived object) is compiled into a stand-alone host program, tests/c/scratch_check.cpp, against counting stubs of
bq_device_malloc / bq_device_free (no HIP runtime): for 0..6 requests with any one of them refused, every later request returns
null without reaching the allocator, error() is the first failure, and the destructor frees exactly what was handed out, once each;
a zero-count request asks the allocator, gets a null pointer and frees nothing; release() frees one buffer at once and never again
(null and foreign pointers: nothing), a request after it is served, and bq_owner takes 40 requests and frees all 40 once.  The
program is built with AddressSanitizer and UndefinedBehaviorSanitizer, which own the double-free and leak reports."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_scratch_owner_frees_what_it_handed_out_and_stops_at_the_first_failure(tmp_path):
    exe = str(tmp_path / 'scratch_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'scratch_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}'
    assert 'scratch_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
