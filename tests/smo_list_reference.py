"""Reference side of the support-list edge tests (tests/test_smo_list_host.py, tests/test_gpu_smo_list_edges.py): plain NumPy.

The device walker (csrc/bq_smo.hip) keeps the samples with a non-zero multiplier in an ascending list and edits it in place after every
pair step (`sup_apply`): an insert shifts the entries behind the position one to the right, an erase one to the left, SMO_T entries per
trip of the shift loop, and the first SMO_CAP positions live in LDS while the rest live in global memory only.  `SupportListModel`
restates that list on the host and classifies every edit, so that a run of the CPU oracle (oracle/smo_oracle.py, followed through its
`on_step` callback) can say how often the walker's list met each of those edges:

  long insert / long erase        more than SMO_T entries shifted: the shift loop runs more than once
  crossing insert / erase         an entry moves from position SMO_CAP - 1 to SMO_CAP, or back: between the two homes of the list
  long dot                        an error sum over more than SMO_CAP entries (counted where it led to a pair step: a lower bound)

The two draws are the ones whose counts were measured; `run_oracle` is the oracle with the walker's tie rule and summation order.
"""
import numpy as np

from oracle import smo_oracle as smo

SMO_T = 1024     # csrc/bq_smo.hip: threads of the walker workgroup = entries shifted per trip of sup_apply's loops
SMO_CAP = 4096   # csrc/bq_smo.hip: entries of the support list mirrored in LDS

EVENT_CLASSES = ('long_inserts', 'long_erases', 'crossing_inserts', 'crossing_erases', 'long_dots')


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def rbf_gamma(X):
    """gamma='scale' of the kernels: 1 / (d var X)"""
    return 1.0 / (X.shape[1] * X.var())


def compact_gamma(X):
    """a gamma at which the panel is stored in the compact 7-byte layout (csrc/bq_c7.h: exp(-gamma 4 max|x|^2) >= 2^-14, here
    2^-12.6); neither draw is eligible at gamma='scale' (about 1e-6 and 1e-7)"""
    return 0.9 * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())


def rbf_gram(X, gamma):
    sq = (X * X).sum(axis=1)
    return np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))


def svc_draw(n=4800):
    """(X, y, parameters): n x 10 standard normal rows with coin-flip labels — nearly every sample ends with a multiplier"""
    rs = np.random.RandomState(11)
    X = rs.standard_normal((n, 10))
    y = np.where(rs.uniform(size=n) < 0.5, 1., -1.)
    return X, y, dict(C=0.1, tol=1e-2)


def svr_draw(n=4600):
    rs = np.random.RandomState(12)
    X = rs.standard_normal((n, 8))
    y = np.sin(X[:, 0]) + 0.5 * rs.standard_normal(n)
    return X, y, dict(C=0.1, epsilon=0.01, tol=1e-2)


def row_list_draw(n=6000):
    """the SVC recipe at n rows for a two-column batched solve: (X, Y, rows, parameters).  Column 0: every row, labels sign(X[:, 0]);
    column 1: the ascending list without every fifth row, coin-flip labels."""
    X, y, par = svc_draw(n)
    rows = np.flatnonzero(np.arange(n) % 5 != 4)
    return X, np.stack([np.where(X[:, 0] > 0, 1., -1.), y]), [np.arange(n), rows], par


# ---- the list ---------------------------------------------------------------------------------------------------------------------
class Edit:
    """one call of sup_apply: kind 'none' | 'update' | 'insert' | 'erase'; pos, the list position of the sample; shifted, the entries
    that change position; trips of the shift loop; crossing, whether an entry moves between positions SMO_CAP - 1 and SMO_CAP"""

    def __init__(self, kind, pos, shifted, crossing):
        self.kind, self.pos, self.shifted, self.crossing = kind, pos, shifted, crossing
        self.trips = -(-shifted // SMO_T)

    def __repr__(self):
        return 'Edit(%s at %d, %d shifted, crossing=%s)' % (self.kind, self.pos, self.shifted, self.crossing)


class SupportListModel:
    """the ascending support list of n samples, empty at the start, and the count of every event class"""

    def __init__(self, n):
        self.member = np.zeros(n, dtype=bool)
        self.nnz = 0
        self.largest = 0
        self.counts = dict.fromkeys(EVENT_CLASSES, 0)

    def apply(self, idx, member):
        """sup_apply(idx, member): the list reflects sample idx, whose multipliers are non-zero now (member) or all zero"""
        pos = int(np.count_nonzero(self.member[:idx]))   # lower bound of idx
        found, nnz = bool(self.member[idx]), self.nnz
        if member and found:
            return Edit('update', pos, 0, False)
        if member:      # [pos, nnz) one to the right
            e = Edit('insert', pos, nnz - pos, pos <= SMO_CAP - 1 <= nnz - 1)
            self.member[idx] = True
            self.nnz = nnz + 1
            self.largest = max(self.largest, self.nnz)
            self.counts['long_inserts'] += e.shifted > SMO_T
            self.counts['crossing_inserts'] += e.crossing
            return e
        if found:       # (pos, nnz) one to the left
            e = Edit('erase', pos, nnz - 1 - pos, pos + 1 <= SMO_CAP <= nnz - 1)
            self.member[idx] = False
            self.nnz = nnz - 1
            self.counts['long_erases'] += e.shifted > SMO_T
            self.counts['crossing_erases'] += e.crossing
            return e
        return Edit('none', pos, 0, False)

    def pair_step(self, i1, i2, member1, member2, summed2):
        """one pair step: sample i2 was examined — with an error sum over the list as it stood when `summed2` — and the list then
        takes i1 and i2 in this order, as the walker does"""
        if summed2 and self.nnz > SMO_CAP:
            self.counts['long_dots'] += 1
        return self.apply(i1, member1), self.apply(i2, member2)


# ---- the oracle run ---------------------------------------------------------------------------------------------------------------
class Snapshots:
    """spy of the oracle: the state after every outer iteration — the multipliers (what `_Snap` of tests/test_gpu_smo.py keeps), the
    thresholds, the step count and the event counts so far"""

    def __init__(self, keys, model):
        self.keys, self.model = keys, model
        self.rows, self.up, self.low, self.steps, self.events = [], [], [], [], []

    def __call__(self, it, s):
        self.rows.append(np.concatenate([getattr(s, k) for k in self.keys]))
        self.up.append(s.b_up)
        self.low.append(s.b_low)
        self.steps.append(s.steps)
        self.events.append(dict(self.model.counts))


def run_oracle(kind, K, y, max_outer, C, tol, epsilon=None):
    """oracle(tie='index', dot='tree') on K for max_outer outer iterations: dict(snap: Snapshots, ref: the oracle's result, counts:
    {event class: times}, largest: the longest the list ever was)"""
    n = len(y)
    model = SupportListModel(n)
    if kind == 'svc':
        snap = Snapshots(('a',), model)

        def on_step(i1, i2, old, new):
            model.pair_step(i1, i2, new[0] != 0, new[1] != 0, not 0 < old[1] < C)
        ref = smo.smo_svc(K, y, C=C, tol=tol, max_outer=max_outer, spy=snap, tie='index', dot='tree', on_step=on_step)
        final = ref['alphas'] != 0
    else:
        snap = Snapshots(('ap', 'an'), model)

        def on_step(i1, i2, old, new):
            p2, m2 = old[1]
            model.pair_step(i1, i2, new[0][0] != 0 or new[0][1] != 0, new[1][0] != 0 or new[1][1] != 0,
                            not (0 < p2 < C or 0 < m2 < C))
        ref = smo.smo_svr(K, y, C=C, epsilon=epsilon, tol=tol, max_outer=max_outer, spy=snap, tie='index', dot='tree',
                          on_step=on_step)
        final = (ref['alphas_p'] != 0) | (ref['alphas_n'] != 0)
    assert np.array_equal(model.member, final)   # the model followed every edit
    return dict(snap=snap, ref=ref, counts=dict(model.counts), largest=model.largest)


def missing_events(counts):
    """the event classes that did not occur"""
    return [k for k in EVENT_CLASSES if counts[k] == 0]
