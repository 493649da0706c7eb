"""The address function of the packed symmetric panel (optiml_amd/csrc/bq_sym_layout.h: tile rows concatenated, inside a tile row
the strips of 8 tiles one after another, each a row-major 256 x W block) is compiled into a stand-alone host program,
tests/c/sym_layout_check.cpp, which checks for nb = 1 .. 40 that (I, r, c) -> address is a bijection onto [0, elems) and that the
strip rows keep their alignment.  The program is built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_packed_layout_address_map_is_a_bijection_with_aligned_strip_rows(tmp_path):
    exe = str(tmp_path / 'sym_layout_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'sym_layout_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}'
    assert 'sym_layout_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
