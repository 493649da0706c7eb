"""The scalar rules the general entry of the row-based SMO adds to optiml_amd/csrc/bq_rsmo_step.h (Solver_NU's per-sign scans and
score, the two-sided stop test, r1 / r2, the victim rule with two slots to keep) are shared by the device solver (bq_rsmo.hip) and by
a dense host solver around the same header (tests/c/rsmo_nu_step_check.cpp).  Here the host solver is held to the NumPy restatement
(tests/smo_nu_reference.py, itself held to sklearn in test_smo_nu_host.py) on the n = 300 one-class, nu-SVC and nu-SVR problems at
tol 1e-3, from the same start (alpha0, G0): the same pair sequence, and alpha, G, rho and r bit for bit; the cap gives status 2.
The two-keep victim rule runs scripted request sequences with R = 3 and R = 4 against the slots worked out by hand.  The program
is built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import smo_nu_reference as nu
import smo_rows_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    path = str(tmp_path_factory.mktemp('rsmo_nu_step') / 'rsmo_nu_step_check')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-I', os.path.join(REPO, 'optiml_amd', 'csrc'),
                        os.path.join(REPO, 'tests', 'c', 'rsmo_nu_step_check.cpp'), '-o', path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _run(exe, mode, text):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=97', UBSAN_OPTIONS='halt_on_error=1:exitcode=98')
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
    assert 'rsmo_nu_step_check ok' in r.stdout
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout.split('\n')


def _hex(values):
    return ' '.join(float(v).hex() for v in np.asarray(values, dtype=float).ravel())


def _problem(name):
    X, y, gamma, (signs, p, C, alpha0, rule) = nu.case_problem(name)
    K = ref.rbf(X, gamma)
    G0 = nu.product_start_gradient(K, signs, p, alpha0)
    return K, signs, p, C, alpha0, G0, rule


def _text(K, signs, p, C, alpha0, G0, rule, cap):
    return ' '.join([str(len(K)), str(len(signs)), '1' if rule == 'nu' else '0', float(TOL).hex(), str(cap), _hex(K), _hex(signs),
                     _hex(p), _hex(C), _hex(alpha0), _hex(G0)])


@pytest.mark.parametrize('name', ['oc300', 'nusvc300', 'nusvr300'])
def test_host_solver_reproduces_the_reference_bit_for_bit(exe, name):
    K, signs, p, C, alpha0, G0, rule = _problem(name)
    want = nu.solve(rule, K, signs, p, C, TOL, alpha0, G0)
    assert want.status == 'optimal' and want.steps > 100
    out = _run(exe, 'solve', _text(K, signs, p, C, alpha0, G0, rule, 10 ** 7))
    steps, status = (int(v) for v in out[0].split())
    pairs = [int(v) for v in out[1].split()]
    alpha = np.array([float.fromhex(v) for v in out[2].split()])
    G = np.array([float.fromhex(v) for v in out[3].split()])
    scalars = [float.fromhex(v) for v in out[4].split()]
    print(f'{name}: {steps} steps (reference {want.steps})')
    assert status == 1
    assert list(zip(pairs[0::2], pairs[1::2])) == want.pairs
    assert steps == want.steps
    assert alpha.tobytes() == want.alpha.tobytes()
    assert G.tobytes() == want.G.tobytes()
    if rule == 'nu':
        assert scalars == [want.rho, want.r, want.gap_p, want.gap_n]
    else:
        assert scalars == [want.rho, want.gmax, want.gmax2]


@pytest.mark.parametrize('name', ['oc300', 'nusvc300', 'nusvr300'])
def test_host_solver_stops_at_the_cap(exe, name):
    K, signs, p, C, alpha0, G0, rule = _problem(name)
    want = nu.solve(rule, K, signs, p, C, TOL, alpha0, G0, max_steps=17)
    assert want.status == 'stopped' and want.steps == 17
    out = _run(exe, 'solve', _text(K, signs, p, C, alpha0, G0, rule, 17))
    assert [int(v) for v in out[0].split()] == [17, 2]
    assert np.array([float.fromhex(v) for v in out[2].split()]).tobytes() == want.alpha.tobytes()


# (row, the two rows whose slots must stay) -> (slot, hit), by hand: slots never used go first in order, then the smallest stamp,
# never the slot of a row to keep.  The comments give the stamps of the slots after the request.
VICTIM2_SCRIPTS = {
    3: [((1, -1, -1), (0, 0)),   # 1 0 0
        ((2, 1, -1), (1, 0)),    # 1 2 0
        ((3, 1, 2), (2, 0)),     # 1 2 3   rows 1 2 3
        ((4, 2, 3), (0, 0)),     # 4 2 3   both others kept: row 1 goes            rows 4 2 3
        ((2, -1, -1), (1, 1)),   # 4 5 3
        ((5, 4, 2), (2, 0)),     # 4 5 6   row 3 goes                              rows 4 2 5
        ((6, 4, 5), (1, 0)),     # 4 7 6   row 2 goes although row 4 is older: 4 and 5 are kept   rows 4 6 5
        ((7, -1, -1), (0, 0)),   # 8 7 6   nothing kept: the oldest (row 4) goes   rows 7 6 5
        ((8, 6, -1), (2, 0))],   # 8 7 9   one kept: the older of rows 7 and 5 goes
    4: [((1, -1, -1), (0, 0)),   # 1 0 0 0
        ((2, 1, -1), (1, 0)),    # 1 2 0 0
        ((3, 1, 2), (2, 0)),     # 1 2 3 0
        ((4, 1, 3), (3, 0)),     # 1 2 3 4  the slot never used goes first          rows 1 2 3 4
        ((5, 1, 2), (2, 0)),     # 1 2 5 4  the two oldest are kept: row 3 goes     rows 1 2 5 4
        ((1, -1, -1), (0, 1)),   # 6 2 5 4
        ((6, 2, 4), (2, 0)),     # 6 2 7 4  rows 2 and 4 (the two oldest) kept: row 5 goes   rows 1 2 6 4
        ((7, 6, -1), (1, 0)),    # 6 8 7 4  row 2 goes                              rows 1 7 6 4
        ((4, 7, 6), (3, 1)),     # 6 8 7 9
        ((8, -1, -1), (0, 0))],  # row 1 goes
}


@pytest.mark.parametrize('R', [3, 4])
def test_two_keep_victim_rule_on_a_scripted_sequence(exe, R):
    script = VICTIM2_SCRIPTS[R]
    text = ' '.join([str(R), str(len(script))] + ['%d %d %d' % req for req, _ in script])
    out = _run(exe, 'victim2', text)
    got = [tuple(int(v) for v in line.split()) for line in out[:len(script)]]
    assert got == [want for _, want in script]
