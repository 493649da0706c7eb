"""Host checks of the compact fp64 panel code (csrc/bq_c7.h): which values have a 7-byte code and that every one of them comes back
bit for bit through the three planes, +0.0 (the zero pad) included."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include "bq_c7.h"
int main() {
    unsigned long long b;
    while (scanf("%llx", &b) == 1) {
        const uint64_t u = b;
        const uint32_t lo = (uint32_t)u, mid = (uint32_t)(u >> 32) & 0xFFFFu, top = (uint32_t)(u >> 48) & 0xFFu;
        printf("%d %016llx\n", bq_c7_encodable(u) ? 1 : 0, (unsigned long long)bq_c7_bits(lo, mid, top));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def codec(tmp_path_factory):
    d = tmp_path_factory.mktemp('c7')
    src, exe = d / 'c7.cpp', d / 'c7'
    src.write_text(PROGRAM)
    r = subprocess.run(['hipcc', '-x', 'hip', '--offload-arch=gfx950', '-std=c++17', '-O1',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), str(src), '-o', str(exe)], capture_output=True, text=True)
    if r.returncode != 0:
        raise AssertionError(r.stderr)

    def run(values):
        bits = np.asarray(values, dtype=np.float64).view(np.uint64)
        out = subprocess.run([str(exe)], input='\n'.join('%x' % int(b) for b in bits) + '\n', capture_output=True, text=True,
                             check=True).stdout.split()
        ok = np.array([int(t) for t in out[0::2]], dtype=bool)
        back = np.array([int(t, 16) for t in out[1::2]], dtype=np.uint64).view(np.float64)
        return ok, back
    return run


def test_edge_values(codec):
    below_one = np.nextafter(1.0, 0.0)
    good = [1.0, 2.0 ** -14, below_one, 0.0, np.nextafter(2.0 ** -15, 1.0), 1.9999999999999998, 0.5, np.exp(-3.0)]
    ok, back = codec(good)
    assert ok.all()
    assert np.array_equal(back.view(np.uint64), np.asarray(good).view(np.uint64))
    bad = [2.0 ** -15, 2.0, -1.0, -0.0, 2.0 ** -16, np.nan, np.inf, 1e-300]
    ok, _ = codec(bad)
    assert not ok.any()


def test_random_values_in_the_eligible_range(codec):
    rs = np.random.RandomState(0)
    v = np.exp(-rs.uniform(0, 14 * np.log(2), 20000))
    ok, back = codec(v)
    assert ok.all()
    assert np.array_equal(back.view(np.uint64), v.view(np.uint64))
