"""OneVsOneNuSVC on the host: the entry point's declaration, binding and device-free refusals, the estimator's refusals and path
selection, the column plan of a solve, and the per-pair NumPy reference (tests/ovo_nu_reference.py) against sklearn's
OneVsOneClassifier(NuSVC) under the conditions the device test (test_gpu_ovo_nu.py) then holds the kernels to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ovo_nu_reference as onr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_data_is_the_issue_s():
    X, Xnew, codes, y = onr.est_data()
    assert X.shape == (600, 4) and Xnew.shape == (50, 4)
    assert tuple(np.bincount(codes)) == onr.EST_COUNTS and set(y) == {3, 5, 11}
    _, _, cols = onr.traj_columns()
    assert len(cols) == 12 and len({pair for pair, _ in cols}) == 6


def test_entry_point_is_declared_and_bound():
    from optiml_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bcqp.h')).read()
    assert re.search(r'^int bq_msolver_create_simplex2_pairs\(bq_problem \*p, int ncls, const int \*cls_tiles, int m, '
                     r'const int \*pairs, const double \*UB,\s+const double \*mass, const double \*x0, double tol, '
                     r'int64_t max_iter, bq_msolver \*\*out\);', header, re.M)
    assert 'still 3: bq_msolver_create_simplex2_pairs was added' in header
    assert re.search(r'#define BQ_ABI_VERSION 3\b', header)
    lib = _lib.load()
    assert lib.bq_abi_version() == 3
    fn = lib.bq_msolver_create_simplex2_pairs
    assert fn.restype is C.c_int and len(fn.argtypes) == 11


def test_null_arguments_and_counts_are_refused_without_a_device():
    from optiml_amd import _lib
    lib = _lib.load()
    ct = np.array([0, 1, 2], dtype=np.int32)
    pr = np.array([0, 1], dtype=np.int32)
    ub, mass = np.ones(512), np.ones(2)
    h = C.c_void_p()
    fake = C.c_void_p(1)   # never dereferenced: the NULL and count checks come first
    full = [fake, 2, _lib.iptr(ct), 1, _lib.iptr(pr), _lib.ptr(ub), _lib.ptr(mass), None, 1e-3, 10, C.byref(h)]
    for hole in (0, 2, 4, 5, 6, 10):
        args = list(full)
        args[hole] = None
        assert lib.bq_msolver_create_simplex2_pairs(*args) == _lib.ERR_BADARG, hole
        assert b'NULL argument' in lib.bq_last_error()
    for m in (0, -3):
        args = list(full)
        args[3] = m
        assert lib.bq_msolver_create_simplex2_pairs(*args) == _lib.ERR_BADARG
        assert b'm must be >= 1' in lib.bq_last_error()
    assert not h.value


def test_refusals_and_path_selection():
    from optiml_amd.ml.svm import OneVsOneNuSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel
    from optiml_amd.ml.svm.nu_ovo import _check_pairs_feasible, uses_batched_ovo_nu
    codes = np.repeat([0, 1, 2], (10, 30, 30))
    _check_pairs_feasible(codes, 3, [0.5])            # pair (0, 1): 0.5 * 40 / 2 = 10 <= 10
    with pytest.raises(ValueError, match='specified nu is infeasible'):
        _check_pairs_feasible(codes, 3, [0.5017])
    with pytest.raises(ValueError, match='specified nu is infeasible'):
        _check_pairs_feasible(codes, 3, [0.3, 0.5017])   # any nu of a path
    X = np.zeros((70, 2))
    with pytest.raises(ValueError, match='specified nu is infeasible'):   # before the storage refusal and any device work
        OneVsOneNuSVC(nu=0.5017, storage='stream').fit(X, codes)
    with pytest.raises(ValueError, match='only one class is present'):
        OneVsOneNuSVC().fit(X, np.zeros(70))
    with pytest.raises(ValueError, match='nu must be in'):
        OneVsOneNuSVC(nu=0.0)
    assert uses_batched_ovo_nu(OneVsOneNuSVC(kernel=GaussianKernel(gamma=0.5)), 1)
    assert uses_batched_ovo_nu(OneVsOneNuSVC(kernel=GaussianKernel(gamma='auto'), storage='f32'), 1)
    assert uses_batched_ovo_nu(OneVsOneNuSVC(kernel=LinearKernel()), 1)
    assert not uses_batched_ovo_nu(OneVsOneNuSVC(kernel=GaussianKernel(gamma='scale')), 1)
    assert not uses_batched_ovo_nu(OneVsOneNuSVC(kernel=GaussianKernel(gamma=0.5)), 2)
    assert not uses_batched_ovo_nu(OneVsOneNuSVC(kernel=GaussianKernel(gamma=0.5), storage='stream'), 1)
    est = OneVsOneNuSVC(kernel=GaussianKernel(gamma=0.5), nu=0.3, tol=1e-5, max_iter=77, storage='f32')
    assert est.get_params(deep=False) == dict(kernel=est.kernel, nu=0.3, tol=1e-5, max_iter=77, storage='f32')
    one = est._binary()
    assert (one.nu, one.tol, one.max_iter, one.storage, one.kernel) == (0.3, 1e-5, 77, 'f32', est.kernel)


def test_column_plan():
    """UB is 1 exactly on the pair's data rows of the class-sorted panel, each group's mass is nu (n_i + n_j) / 2, and the columns of a
    path come in (nu, pair) order with the pairs in OneVsOneClassifier's order."""
    from optiml_amd.ml.svm.nu_ovo import ovo_nu_boxes, ovo_nu_columns
    from optiml_amd.ml.svm.onevsone import ovo_pairs, sort_plan
    _, _, codes = onr.ovo_nu_data((256, 1, 40, 300), 2)
    counts = np.bincount(codes)
    nus = [0.01, 0.004]
    cols = ovo_nu_columns(codes, 4, nus)
    assert [(t, pair) for t, pair, _ in cols] == [(t, pair) for t in range(2) for pair in ovo_pairs(4)]
    assert ovo_pairs(4) == onr.pairs_of(4)
    index, cls_tiles, n_pad = sort_plan(codes, 4)
    assert list(cls_tiles) == [0, 1, 2, 3, 5] and n_pad == 1280
    ghost = np.ones(n_pad, dtype=bool)
    ghost[index] = False
    pcode = np.repeat(np.arange(4), np.diff(cls_tiles) * 256)
    UB, mass = ovo_nu_boxes(cols, pcode, ghost)
    assert UB.shape == (12, n_pad) and mass.shape == (12, 2)
    for c, (t, (i, j), ms) in enumerate(cols):
        rows, _ = onr.pair_rows(codes, i, j)
        want = np.zeros(n_pad)
        want[index[rows]] = 1.
        assert np.array_equal(UB[c], want)
        assert UB[c].sum() == counts[i] + counts[j]
        assert ms == nus[t] * (counts[i] + counts[j]) / 2 and np.array_equal(mass[c], [ms, ms])
        assert not UB[c][ghost].any()
    # class 0 fills its tile: no ghost row; class 1 is one row and 255 ghost rows
    assert not ghost[:256].any() and ghost[256:512].sum() == 255


def test_column_chunks_keep_the_order():
    from optiml_amd.ml.svm import nu_ovo
    cols = nu_ovo.ovo_nu_columns(np.repeat([0, 1, 2], 300), 3, [0.2, 0.3])
    ct = np.array([0, 2, 4, 6], dtype=np.int32)
    per = 6 * 8 * (1536 + 256) + nu_ovo.pairs_slab_bytes(ct, [(0, 1)])
    chunks = nu_ovo.column_chunks(cols, ct, 1536, 2 * (2 * per + 1))   # MEMORY_SHARE = 0.5: two columns fit
    assert [len(c) for c in chunks] == [2, 2, 2] and [col for c in chunks for col in c] == cols
    assert nu_ovo.column_chunks(cols, ct, 1536, 1)[0] == cols[:1]   # a column alone always runs
    assert nu_ovo.column_chunks(cols, ct, 1536, 1 << 40) == [cols]


@pytest.mark.parametrize('tol', onr.TOLS)
@pytest.mark.parametrize('gamma,nu', onr.EST_GRID)
def test_reference_against_sklearn(gamma, nu, tol):
    """The per-pair reference under the device test's conditions (ovo_nu_reference.check_against_sklearn).  Measured with it over the
    grid: decision differences of at most 1.45 tol / r, at most 576 iterations (gamma = 0.5, nu = 0.3517, tol 1e-6), r between 0.158
    and 10.6, at most 2.2 % of the training rows left out (gamma = 0.5, nu = 0.3517, tol 1e-3) and none at tol 1e-6."""
    pytest.importorskip('sklearn')
    X, _, codes, _ = onr.est_data()
    mine = onr.RefOvO(X, codes, onr.EST_LABELS, gamma, nu, tol)
    onr.check_against_sklearn(mine, onr.sk_ovo(gamma, nu), gamma, nu, tol)


def test_two_class_decision_is_one_dimensional_in_the_reference_s_form():
    conf = np.array([[0.4], [-2.0]])
    Y = onr.ovo_decision(conf, 2)
    from optiml_amd.ml.svm.onevsone import ovo_decision
    assert np.array_equal(Y, ovo_decision((conf > 0).astype(int), conf, 2))
    assert Y[0, 1] > Y[0, 0] and Y[1, 0] > Y[1, 1]
