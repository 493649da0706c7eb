"""The scalar rules of the row-based SMO (optiml_amd/csrc/bq_rsmo_step.h: the I_up / I_low predicates, the WSS2 score, the
two-variable update with its clipping cascades, the rho pieces, the cache's victim rule) are shared by the device solver
(bq_rsmo.hip) and by a dense host solver around the same header (tests/c/rsmo_step_check.cpp).  Here the host solver is held to
the NumPy restatement of libsvm's Solver (tests/smo_rows_reference.py, itself held to sklearn in test_smo_rows_host.py) on the
n = 300 SVC problem, the n = 300 SVR problem and the class-weighted SVC problem: the same pair sequence, and alpha, G and rho bit for
bit.  The victim rule runs a scripted request sequence with R = 2 and R = 3 against the slots worked out by hand.  The program is
built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import smo_rows_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    path = str(tmp_path_factory.mktemp('rsmo_step') / 'rsmo_step_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-I', os.path.join(REPO, 'optiml_amd', 'csrc'),
                        os.path.join(REPO, 'tests', 'c', 'rsmo_step_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _run(exe, mode, text):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
    assert 'rsmo_step_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout.split('\n')


def _hex(values):
    return ' '.join(float(v).hex() for v in np.asarray(values, dtype=float).ravel())


@pytest.mark.parametrize('name,weighted', [('svc300', False), ('svr300', False), ('svc300', True)])
def test_host_solver_reproduces_the_reference_bit_for_bit(exe, name, weighted):
    X, y, gamma, signs, p, C = ref.case_problem(name, weighted)
    K = ref.rbf(X, gamma)
    want = ref.solve(K, signs, p, C, TOL)
    assert want.status == 'optimal' and want.steps > 100
    text = ' '.join([str(len(K)), str(len(signs)), float(TOL).hex(), str(10 ** 7), _hex(K), _hex(signs), _hex(p), _hex(C)])
    out = _run(exe, 'solve', text)
    steps, status = (int(v) for v in out[0].split())
    pairs = [int(v) for v in out[1].split()]
    alpha = np.array([float.fromhex(v) for v in out[2].split()])
    G = np.array([float.fromhex(v) for v in out[3].split()])
    rho, gmax, gmax2 = (float.fromhex(v) for v in out[4].split())
    print(f'{name} weighted={weighted}: {steps} steps (reference {want.steps})')
    assert status == 1
    assert list(zip(pairs[0::2], pairs[1::2])) == want.pairs
    assert steps == want.steps
    assert alpha.tobytes() == want.alpha.tobytes()
    assert G.tobytes() == want.G.tobytes()
    assert rho == want.rho and gmax == want.gmax and gmax2 == want.gmax2


def test_host_solver_stops_at_the_cap(exe):
    X, y, gamma, signs, p, C = ref.case_problem('svc300')
    K = ref.rbf(X, gamma)
    want = ref.solve(K, signs, p, C, TOL, max_steps=17)
    assert want.status == 'stopped' and want.steps == 17
    out = _run(exe, 'solve', ' '.join([str(len(K)), str(len(signs)), float(TOL).hex(), '17', _hex(K), _hex(signs), _hex(p), _hex(C)]))
    assert [int(v) for v in out[0].split()] == [17, 2]
    assert np.array([float.fromhex(v) for v in out[2].split()]).tobytes() == want.alpha.tobytes()


# (row, row whose slot must stay) -> (slot, hit), by hand: slots never used go first in order, then the smallest stamp, never the
# slot of the row to keep
VICTIM_SCRIPTS = {
    2: [((5, -1), (0, 0)), ((7, 5), (1, 0)), ((5, -1), (0, 1)), ((9, 5), (1, 0)),   # 7 goes: 5 is kept (and fresher)
        ((8, 9), (0, 0)),                                                           # 5 goes: 9 is kept
        ((3, 9), (0, 0)),                                                           # 8 goes although it is the fresher: 9 is kept
        ((9, 3), (1, 1)), ((4, -1), (0, 0))],                                       # nothing kept: the older (3) goes
    3: [((1, -1), (0, 0)), ((2, 1), (1, 0)), ((3, 2), (2, 0)), ((1, -1), (0, 1)),
        ((4, 1), (1, 0)),    # stamps 4, 2, 3: row 2 is the oldest
        ((5, 3), (0, 0)),    # stamps 4, 5, 3: row 3 is the oldest but kept, the next oldest (row 1) goes
        ((3, 5), (2, 1)), ((6, -1), (1, 0))],   # stamps 6, 5, 7: row 4 goes
}


@pytest.mark.parametrize('R', [2, 3])
def test_victim_rule_on_a_scripted_sequence(exe, R):
    script = VICTIM_SCRIPTS[R]
    text = ' '.join([str(R), str(len(script))] + ['%d %d' % req for req, _ in script])
    out = _run(exe, 'victim', text)
    got = [tuple(int(v) for v in line.split()) for line in out[:len(script)]]
    assert got == [want for _, want in script]
