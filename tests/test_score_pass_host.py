"""One scoring pass (optiml_amd/csrc/bq_score_pass.h: what the held-out entry points of bq_mscore.hip repeat around their launches) is
compiled into a stand-alone host program, tests/c/score_pass_check.cpp, against counting stubs of bq_device_malloc / bq_device_free
and of the copy and set calls (no HIP runtime; the stubs really copy, so a wrong byte count overruns a buffer): for 0..8 mixed
requests with any one request or any one copy refused, with a pending launch error and with a launcher's own code, nothing after
the failure reaches the allocator or a copy, the code is BQ_ERR_NOMEM only for an out-of-memory failure of the set-up and BQ_ERR_HIP
otherwise under the stage's message, finish() copies every ledger entry exactly once with its byte count and nothing after a
failure, a null-host output is never copied, and every buffer is freed once.  The program is built with AddressSanitizer and
UndefinedBehaviorSanitizer, which own the overrun, double-free and leak reports."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_score_pass_stops_at_the_first_failure_and_copies_every_output_once(tmp_path):
    exe = str(tmp_path / 'score_pass_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), '-I', os.path.join(REPO, 'include'),
                        os.path.join(REPO, 'tests', 'c', 'score_pass_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}'
    assert 'score_pass_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
