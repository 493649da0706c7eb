"""CPU checks of OneVsRestSVC: constructor validation, label binarisation, the batched-vs-fallback dispatch and the C ABI symbols of
the batched solver (no GPU needed)."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['bq_msolver_create', 'bq_msolver_run', 'bq_msolver_state', 'bq_msolver_get', 'bq_msolver_destroy',
               'bq_problem_gram_matmat']


def _bad_arguments():
    from optiml_amd.ml.svm.losses import hinge, epsilon_insensitive
    return [dict(kernel='rbf'), dict(C=0), dict(rho=-1), dict(mu=0), dict(fit_intercept=1), dict(reg_intercept='yes'),
            dict(dual=1), dict(optimizer=3), dict(tol=0), dict(loss=epsilon_insensitive), dict(loss=hinge, C=-2.)]


@pytest.mark.parametrize('i', range(11))
def test_constructor_rejects_what_svc_rejects(i):
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    kw = _bad_arguments()[i]
    with pytest.raises(Exception) as ref:
        SVC(**kw)
    with pytest.raises(type(ref.value)) as ours:
        OneVsRestSVC(**kw)
    assert str(ours.value) == str(ref.value)


def test_constructor_keeps_svc_arguments():
    import inspect
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.losses import hinge
    assert list(inspect.signature(OneVsRestSVC).parameters) == list(inspect.signature(SVC).parameters)
    est = OneVsRestSVC(loss=hinge, C=3.0, dual=True, reg_intercept=True, max_iter=7)
    assert est.C == 3.0 and est.max_iter == 7
    assert est.get_params()['max_iter'] == 7
    est.set_params(max_iter=9)
    assert est._prototype().max_iter == 9


@pytest.mark.parametrize('labels', [np.array([3, 0, 7, 3, 7, 0, 0, 7]), np.array(['b', 'a', 'c', 'a', 'c', 'b']),
                                    np.array([5, 2, 5, 2, 2]), np.array(['no', 'yes', 'yes', 'no'])])
def test_binarisation_matches_label_binarizer_and_svc_mapping(labels):
    sk = pytest.importorskip('sklearn.preprocessing')
    from optiml_amd.ml.svm.multiclass import binarize
    classes, Y = binarize(labels)
    lb = sk.LabelBinarizer().fit(labels)
    assert np.array_equal(classes, lb.classes_)
    cols = lb.transform(labels).T   # one column per class; ONE column (classes_[1]) with two classes
    assert Y.shape == cols.shape
    for col, row in zip(cols, Y):
        # SVC.fit maps the larger of the column's labels {0, 1} to +1
        assert np.array_equal(row, np.where(col == col.max(), 1., -1.))


def test_binarisation_needs_two_classes():
    from optiml_amd.ml.svm.multiclass import binarize
    with pytest.raises(ValueError):
        binarize(np.zeros(4))


def _dispatch_rows():
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    from optiml_amd.opti.constrained import ActiveSet, FrankWolfe, InteriorPoint, ProjectedGradient
    from optiml_amd.opti.unconstrained.stochastic import AdaGrad
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient)
    return [
        (dict(base), 1, True),
        (dict(base, optimizer=FrankWolfe), 1, True),
        (dict(base, storage='f32'), 1, True),
        (dict(base, storage='stream'), 1, False),
        (dict(base), 2, False),
        (dict(base, optimizer=ActiveSet), 1, False),
        (dict(base, optimizer=InteriorPoint), 1, False),
        (dict(base, optimizer='smo', reg_intercept=False), 1, False),
        (dict(base, optimizer=AdaGrad, learning_rate=1.), 1, False),
        (dict(base, reg_intercept=False), 1, False),
        (dict(base, dual=False), 1, False),
        (dict(base, loss=squared_hinge), 1, False),
    ]


@pytest.mark.parametrize('row', range(12))
def test_dispatch_rule(row):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.multiclass import uses_batched_path
    kw, world, want = _dispatch_rows()[row]
    assert uses_batched_path(SVC(**kw), world) is want


def test_make_multiclass_blobs():
    from optiml_amd.datasets import make_multiclass_blobs
    X, y = make_multiclass_blobs(103, 5, 4, seed=3)
    assert X.shape == (103, 5) and X.flags['C_CONTIGUOUS'] and y.dtype == np.int64
    assert sorted(np.unique(y)) == [0, 1, 2, 3] and np.bincount(y).min() >= 25
    np.testing.assert_allclose(X.mean(axis=0), 0, atol=1e-12)
    np.testing.assert_allclose(X.std(axis=0), 1, atol=1e-12)
    X2, y2 = make_multiclass_blobs(103, 5, 4, seed=3)
    assert np.array_equal(X, X2) and np.array_equal(y, y2)


def test_batched_abi_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3
