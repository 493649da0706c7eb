"""The scalar recurrence of MINRES (optiml_amd/csrc/bq_minres_rec.h: Lanczos coefficients, Givens rotation, scipy's seven stopping
tests in scipy's order) is shared by the three device forms (bq_minres.hip, bq_xstar.hip), which are held to scipy only to
rtol 1e-5.  Here a dense host MINRES around that header (tests/c/minres_rec_check.cpp) is held to scipy.sparse.linalg.minres itself
on two small systems: the same iteration count, and x to rtol 1e-12 — the per-kernel parity bar: the two differ
by the last bits of a handful of dot products, so more than that is a transcription error in the recurrence.  The program is built
with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5   # scipy's default, which the device forms use


def _systems():
    rs = np.random.RandomState(0)
    U = np.linalg.qr(rs.standard_normal((6, 6)))[0]
    b = rs.standard_normal(6)
    A = U @ np.diag([-3., -2., -1., 1., 2., 3.]) @ U.T      # indefinite
    A = (A + A.T) / 2
    B = U @ np.diag([0., 0., 1., 2., 3., 4.]) @ U.T         # rank 4: the normal equations B B x = B b, as the ActiveSet fallback
    B = (B + B.T) / 2
    return {'indefinite': (A, b), 'normal_rank4': (B @ B, B @ b)}


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    path = str(tmp_path_factory.mktemp('minres_rec') / 'minres_rec_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                        '-I', os.path.join(REPO, 'optiml_amd', 'csrc'), os.path.join(REPO, 'tests', 'c', 'minres_rec_check.cpp'),
                        '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


@pytest.mark.parametrize('name', ['indefinite', 'normal_rank4'])
def test_shared_recurrence_follows_scipy_minres(exe, name):
    from scipy.sparse.linalg import minres
    A, b = _systems()[name]
    n = len(b)
    its = []
    x_ref, info = minres(A, b, rtol=RTOL, callback=lambda xk: its.append(1))
    assert info == 0
    text = ' '.join([str(n), str(5 * n), float(RTOL).hex()] + [float(v).hex() for v in A.ravel()] + [float(v).hex() for v in b])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
    assert 'minres_rec_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split('\n')[0].split()
    itn, istop, x = int(out[0]), int(out[1]), np.array([float.fromhex(t) for t in out[2:]])
    print(f'{name}: scipy {len(its)} iterations, header {itn} (istop {istop}), max rel diff '
          f'{np.max(np.abs(x - x_ref) / np.abs(x_ref)):.3e}')
    assert itn == len(its)
    assert istop in (1, 2)      # scipy's info 0 through one of the two residual tests
    np.testing.assert_allclose(x, x_ref, rtol=1e-12, atol=0)
