"""The Hessian image format (optiml_amd/csrc/bq_h52.h: fl(K + 1) as a 52-bit code in three planes, tile rows in lane order) is compiled
into a stand-alone host program, tests/c/h52_check.cpp, which checks that encode / decode round-trip bit for bit over the domain
{1.0} u [1 + 2^-15, 2.0] (the named edge values and four million random K), that the escape code is produced by 2.0 alone, that values
outside the domain are refused, that the lane order is a bijection of a tile row and that, composed with bq_sym_addr at nb = 1, 8, 9, 17,
every access stays inside the 6.5-byte allocation.  The program is built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_h52_codes_round_trip_and_the_lane_order_stays_inside_the_image(tmp_path):
    exe = str(tmp_path / 'h52_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'h52_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}'
    assert 'h52_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
