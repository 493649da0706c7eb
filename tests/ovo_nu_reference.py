"""One-vs-one nu-SVC in NumPy: the data of the OneVsOneNuSVC tests, the per-pair use of tests/nu_reference.py (the pair's own
sub-Gram, the larger class positive, as OneVsOneClassifier hands NuSVC.fit its rows), sklearn's vote-and-confidence decision, and
the conditions under which a one-vs-one fit is held to sklearn's OneVsOneClassifier(NuSVC) — shared by the host test, which holds
this reference to them, and the device test, which holds `OneVsOneNuSVC` to them."""
import functools

import numpy as np

import nu_reference as nur
from oracle import svm_oracle as so


def ovo_nu_data(counts, seed, d=4):
    rs = np.random.RandomState(seed)
    codes = rs.permutation(np.repeat(np.arange(len(counts)), counts))
    centers = 1.2 * rs.standard_normal((len(counts), d))
    X = centers[codes] + rs.standard_normal((len(codes), d))
    Xnew = 1.5 * rs.standard_normal((50, d))
    return X, Xnew, codes


def pairs_of(ncls):
    return [(i, j) for i in range(ncls) for j in range(i + 1, ncls)]


def pair_rows(codes, i, j):
    """the rows of classes i and j in their original order, and their labels: class j, the larger, is +1"""
    rows = np.flatnonzero((codes == i) | (codes == j))
    return rows, np.where(codes[rows] == j, 1., -1.)


def pair_gram(X, codes, i, j, gamma):
    rows, y = pair_rows(codes, i, j)
    return rows, y, so.gram('rbf', X[rows], gamma=gamma)


# ---- the estimator grid (tests 6, 8, 9, 10 of the device file; the host file holds this reference to sklearn on it) ----------------
EST_COUNTS, EST_SEED = (260, 130, 210), 0
EST_LABELS = np.array([3, 5, 11])
EST_GRID = ((1.0 / 8, 0.5017), (0.5, 0.5017), (0.5, 0.3517))
TOLS = (1e-3, 1e-6)


@functools.lru_cache(maxsize=None)
def est_data():
    X, Xnew, codes = ovo_nu_data(EST_COUNTS, EST_SEED)
    for a in (X, Xnew, codes):
        a.setflags(write=False)
    return X, Xnew, codes, EST_LABELS[codes]


@functools.lru_cache(maxsize=None)
def sk_ovo(gamma, nu):
    """sklearn's OneVsOneClassifier(NuSVC) at tol 1e-12 on the estimator data (the caller has checked that sklearn is there)"""
    from sklearn.multiclass import OneVsOneClassifier
    from sklearn.svm import NuSVC
    X, _, _, y = est_data()
    return OneVsOneClassifier(NuSVC(kernel='rbf', gamma=gamma, nu=nu, tol=1e-12)).fit(X, y)


def ovo_decision(conf, ncls):
    """sklearn's `_ovr_decision_function` with the votes taken from the confidences' signs"""
    votes = np.zeros((conf.shape[0], ncls))
    total = np.zeros((conf.shape[0], ncls))
    for k, (i, j) in enumerate(pairs_of(ncls)):
        total[:, i] -= conf[:, k]
        total[:, j] += conf[:, k]
        votes[conf[:, k] <= 0, i] += 1
        votes[conf[:, k] > 0, j] += 1
    return votes + total / (3 * (np.abs(total) + 1))


class RefPair:
    """nu_reference.fit_nu_svc on one pair's rows, with the attributes of a fitted NuSVC that `check_against_sklearn` reads"""

    def __init__(self, X, codes, i, j, gamma, nu, tol, max_iter=1000):
        rows, y, K = pair_gram(X, codes, i, j, gamma)
        out = nur.fit_nu_svc(K, y, nu, tol=tol, max_iter=max_iter)
        self._X, self._gamma, self._coef = X[rows], gamma, out['coef']
        self.alphas_, self.margin_scale_, self.intercept_ = out['x'], out['r'], out['intercept']
        self.status_, self.n_iter_, self.kkt_violation_ = out['status'], out['iter'], float(out['rows'][-1, 2])
        self.support_ = np.flatnonzero(out['x'] > 0)

    def decision_function(self, Z):
        return so.gram('rbf', Z, self._X, gamma=self._gamma) @ self._coef + self.intercept_


class RefOvO:
    """the per-pair reference fits of one (gamma, nu, tol) on (X, codes), with OneVsOneNuSVC's attributes"""

    def __init__(self, X, codes, labels, gamma, nu, tol):
        self.classes_ = np.asarray(labels)
        self.estimators_ = [RefPair(X, codes, i, j, gamma, nu, tol) for i, j in pairs_of(len(labels))]

    def decision_function(self, Z):
        return ovo_decision(np.stack([e.decision_function(Z) for e in self.estimators_], axis=1), len(self.classes_))

    def predict(self, Z):
        return self.classes_[self.decision_function(Z).argmax(axis=1)]


def clear_rows(sk, bounds, Z):
    """(clear, sure): the rows of Z where every pair's sklearn |decision| exceeds its bound, and those of them where sklearn's top two
    values also differ by more than twice sum_p bound_p / 3"""
    clear = np.all([np.abs(e.decision_function(Z)) > b for e, b in zip(sk.estimators_, bounds)], axis=0)
    top = np.sort(sk.decision_function(Z), axis=1)
    return clear, clear & (top[:, -1] - top[:, -2] > 2 * sum(bounds) / 3)


def check_against_sklearn(mine, sk, gamma, nu, tol, max_iter=1000):
    """`mine` (estimators_ of NuSVC attributes in pair order, decision_function, predict) against sklearn's fit `sk` of the estimator
    data.  Per pair p, with bound_p = 10 tol / r_p: 'optimal' within max_iter; each class's alpha sums to nu (n_i + n_j) / 2 to 1e-10
    relative; the violation recomputed in NumPy from alphas_ is within tol + 1e-9 and the reported one within tol; the decision values
    on the pair's rows and on Xnew lie within bound_p of sklearn's pair estimator; at tol 1e-6 the support set is sklearn's (sorted).
    Whole estimator, on X and Xnew: on the rows where every pair's sklearn |decision| exceeds its bound (there the votes agree, and a
    class's summed confidence moves by at most sum_p bound_p, its monotone map's slope being at most 1/3) decision_function lies
    within sum_p bound_p / 3 of sklearn's, and predict agrees where sklearn's top two values also differ by more than twice that.
    Those conditions may leave out at most 5 % of the training rows.  Returns the figures it prints."""
    X, Xnew, codes, y = est_data()
    ncls = len(EST_LABELS)
    pairs = pairs_of(ncls)
    assert len(mine.estimators_) == len(pairs) == len(sk.estimators_)
    bounds, worst, iters, rs = [], 0.0, [], []
    for p, (i, j) in enumerate(pairs):
        est, ref = mine.estimators_[p], sk.estimators_[p]
        rows, yp, K = pair_gram(X, codes, i, j, gamma)
        n = len(rows)
        assert est.status_ == 'optimal' and est.n_iter_ <= max_iter, (p, est.status_, est.n_iter_)
        a, r = est.alphas_, est.margin_scale_
        assert a.shape == (n,) and a.min() >= 0 and a.max() <= 1 and r > 0
        for cls in (1., -1.):
            assert abs(a[yp == cls].sum() - nu * n / 2) <= 1e-10 * nu * n / 2
        viol = nur.violation2(a, yp * (K @ (yp * a)), np.ones(n), nur.Layout(n, yp))
        assert viol <= tol + 1e-9 and est.kkt_violation_ <= tol, (p, viol, est.kkt_violation_)
        bound = 10 * tol / r
        for Z in (X[rows], Xnew):
            diff = float(np.abs(est.decision_function(Z) - ref.decision_function(Z)).max())
            worst = max(worst, r * diff / tol)
            assert diff <= bound, (p, diff, bound)
        if tol == 1e-6:
            assert np.array_equal(est.support_, np.sort(ref.support_)), p
        bounds.append(bound)
        iters.append(est.n_iter_)
        rs.append(r)
    total = sum(bounds) / 3
    left_out = 0.0
    for Z in (X, Xnew):
        theirs = sk.decision_function(Z)
        clear, sure = clear_rows(sk, bounds, Z)
        ours = mine.decision_function(Z)
        assert ours.shape == theirs.shape
        assert np.abs(ours - theirs)[clear].max() <= total
        assert np.array_equal(mine.predict(Z)[sure], sk.predict(Z)[sure])
        if Z is X:
            left_out = float((~sure).mean())
            assert (~sure).sum() <= 0.05 * len(X), left_out
    figures = dict(worst=worst, iters=max(iters), r_min=min(rs), r_max=max(rs), left_out=left_out)
    print('gamma=%g nu=%g tol=%g: at most %d iterations, r in [%.3g, %.3g], r |decision difference| / tol <= %.2f, %.1f %% of the '
          'training rows left out' % (gamma, nu, tol, figures['iters'], figures['r_min'], figures['r_max'], worst, 100 * left_out))
    return figures


# ---- the solver-level columns (tests 1, 2 and 4 of the device file) ------------------------------------------------------------------
TRAJ_COUNTS, TRAJ_SEED, TRAJ_GAMMA, TRAJ_ITERS = (1100, 300, 130, 257), 1, 3.0, 20
TRAJ_FRACTIONS = (0.3517, 0.8017)   # a group's mass as a fraction of the pair's smaller class


def traj_columns():
    """(X, codes, [(pair, mass), ...]): the 6 pairs at each fraction, 12 columns, every pair twice"""
    X, _, codes = ovo_nu_data(TRAJ_COUNTS, TRAJ_SEED)
    counts = np.bincount(codes)
    cols = [((i, j), fr * min(counts[i], counts[j])) for fr in TRAJ_FRACTIONS for i, j in pairs_of(len(counts))]
    return X, codes, cols


def solve_column(X, codes, pair, mass, gamma, tol, max_iter, u=None, x0=None, K=None):
    """nu_reference.solve of one column on the pair's own sub-Gram (K: that Gram, else built here); u, x0: on the pair's rows.
    Returns (rows, y, K, result)."""
    rows, y = pair_rows(codes, *pair)
    K = so.gram('rbf', X[rows], gamma=gamma) if K is None else K
    u = np.ones(len(rows)) if u is None else u
    masses = (mass, mass) if np.isscalar(mass) else tuple(mass)
    return rows, y, K, nur.solve(K, u, masses, sgn=y, tol=tol, max_iter=max_iter, x0=x0)


@functools.lru_cache(maxsize=None)
def trajectory_reference():
    """The reference's 20 iterations of the 12 columns, and per column the largest spread of its final x over three seeded draws of
    K perturbed by one ulp per entry (test_gpu_nu._trajectory_reference's figure).  Every column is still far from its optimum."""
    X, codes, cols = traj_columns()
    grams, out = {}, []
    for pair, mass in cols:
        if pair not in grams:
            grams[pair] = so.gram('rbf', X[pair_rows(codes, *pair)[0]], gamma=TRAJ_GAMMA)
        K = grams[pair]
        rows, y, _, base = solve_column(X, codes, pair, mass, TRAJ_GAMMA, 0.0, TRAJ_ITERS, K=K)
        assert base['status'] == 'stopped' and base['iter'] == TRAJ_ITERS and base['rows'][-1, 2] > 1e-3   # far from its optimum
        spread = 0.0
        for seed in range(3):
            up = np.random.RandomState(seed).rand(*K.shape) < 0.5
            r = solve_column(X, codes, pair, mass, TRAJ_GAMMA, 0.0, TRAJ_ITERS, K=np.nextafter(K, np.where(up, np.inf, -np.inf)))[3]
            assert r['iter'] == base['iter']
            spread = max(spread, float(np.abs(r['x'] - base['x']).max()))
        out.append((rows, base, spread))
    return X, codes, cols, out
