"""The blocked Cholesky's schedule (optiml_amd/csrc/bq_chol_sched.h: the block-id -> tile decodes of the update kernels, the choices
by size, and the plan of one factorisation that bq_chol_factor issues step by step) is compiled into a stand-alone host program,
tests/c/chol_sched_check.cpp.  It checks the decodes for T = 1 .. 200 in both tile orders, the forward sweep's slices, and, for
nb = 1 .. 80 block columns x P = 1 .. 4 x look-ahead off and on, that the plan replayed in issue order gives every tile every update
exactly once and in time, reads every image where it was written, and leaves no two conflicting steps unordered between its streams.
The program is built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_cholesky_schedule_decodes_choices_plan_and_stream_order(tmp_path):
    exe = str(tmp_path / 'chol_sched_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'chol_sched_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}'
    assert 'chol_sched_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
