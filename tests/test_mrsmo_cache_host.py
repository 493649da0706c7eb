"""The multi-request resolution of the batched row-based SMO's row cache (optiml_amd/csrc/bq_mrsmo_cache.h), one function for the
device and the host, in a stand-alone program (tests/c/mrsmo_cache_check.cpp, built with ASan + UBSan) against a Python model of the
rule on seeded steps: equal rows of a call share a slot (one miss, then hits), hits are stamped before misses pick victims, a
victim is the least recently stamped slot and never one this call pinned or handed out, at the minimum cache of 2 k rows too."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    path = str(tmp_path_factory.mktemp('mrsmo_cache') / 'mrsmo_cache_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-I', os.path.join(REPO, 'optiml_amd', 'csrc'),
                        os.path.join(REPO, 'tests', 'c', 'mrsmo_cache_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


class Model:
    def __init__(self, R):
        self.R, self.clock, self.hits, self.misses = R, 0, 0, 0
        self.slot_of, self.stamp = {}, [0] * R   # row -> slot; per slot the clock of its last use

    def _touch(self, slot):
        self.clock += 1
        self.stamp[slot] = self.clock

    def call(self, pins, rows):
        start, slots, missed = self.clock, [-1] * len(rows), []
        for p in pins:
            if p >= 0:
                self._touch(self.slot_of[p])
        hit = [r >= 0 and r in self.slot_of for r in rows]   # as the call finds the cache: these are stamped first
        for q, r in sorted(enumerate(rows), key=lambda qr: not hit[qr[0]]):   # (stable: request order within each pass)
            if r < 0:
                continue
            if r in self.slot_of:   # there from the start, or brought in by an earlier request of this call
                self.hits += 1
            else:
                used = len(self.slot_of)
                victim = used if used < self.R else min((s for s in range(self.R) if self.stamp[s] <= start),
                                                        key=lambda s: (self.stamp[s], s))
                self.slot_of = {row: s for row, s in self.slot_of.items() if s != victim}
                self.slot_of[r] = victim
                self.misses += 1
                missed.append((r, victim))
            slots[q] = self.slot_of[r]
            self._touch(slots[q])
        return slots, missed


@pytest.mark.parametrize('n,k,R,seed', [(12, 3, 6, 0), (40, 5, 10, 1), (40, 5, 23, 2), (9, 4, 9, 3), (200, 17, 34, 4), (30, 1, 2, 5)])
def test_resolution_follows_the_model(exe, n, k, R, seed):
    rng = np.random.default_rng(seed)
    calls = []
    for _ in range(60):   # a step: the i rows (no pins), then the j rows with the i rows pinned; some columns ask for nothing
        i_rows = [int(r) if rng.random() > 0.15 else -1 for r in rng.integers(0, min(n, 8 + seed), size=k)]   # few rows: duplicates
        j_rows = [int(r) if i >= 0 else -1 for r, i in zip(rng.integers(0, n, size=k), i_rows)]
        calls += [([], i_rows), (i_rows, j_rows)]
    text = f'{n} {R} {len(calls)}\n' + '\n'.join(f'{len(p)} {" ".join(map(str, p))} {len(r)} {" ".join(map(str, r))}' for p, r in calls)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    out = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, f'rc={out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}'
    lines, model = out.stdout.split('\n'), Model(R)
    assert lines[len(calls)] == 'mrsmo_cache_check ok' and 'runtime error' not in out.stderr
    for (pins, rows), line in zip(calls, lines):
        slots, missed = model.call(pins, rows)
        want = ' '.join(map(str, slots)) + ' |' + ''.join(f' {r}:{s}' for r, s in missed) + f' | {model.hits} {model.misses}'
        assert line == want
        live = [model.slot_of[r] for r in pins + rows if r >= 0]   # every row of the step is still where it was put
        assert len(set(live)) == len({r for r in pins + rows if r >= 0})
    assert model.hits > 0 and model.misses > (R if R < n else 0)   # with fewer slots than rows, rows were evicted
