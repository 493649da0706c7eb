// The one-vs-one vote of one row: sklearn's _ovr_decision_function (svm/onevsone.py: ovo_decision) and np.argmax, statement for
// statement.  One thread per row; the row's ncls sums of confidences and vote counts live in LDS, class c of lane l at
// conf[c * BQ_VOTE_ROWS + l] / votes[c * BQ_VOTE_ROWS + l]: a wave's access to one class touches 64 consecutive words, every bank
// once, and a lane walks its own column only.  The pairs come in ovo_pairs order, (0,1), (0,2), ..., (1,2), ...: every `+=` that
// class i receives (from the pairs (a, i), a < i) precedes every `-=` it gives (to the pairs (i, j), j > i), so the inner loop keeps
// class i's sum and count in registers without changing the order of any sum.  No fused multiply-add (the includer's kernels switch
// contraction off), IEEE division, no atomics and nothing of another row: Y has NumPy's bits and a row's result is the same alone,
// at any position and in any batch.
#pragma once
#include "bq_common.h"

constexpr int BQ_VOTE_ROWS = 64;      // rows (threads) per workgroup: one wavefront
constexpr int BQ_VOTE_MAX_CLS = 64;   // svm/coupling.py: MAX_CLASSES
static inline size_t bq_vote_lds_bytes(int ncls) { return (size_t)ncls * BQ_VOTE_ROWS * (sizeof(double) + sizeof(int)); }

// dec(k): the row's decision value of pair k, positive towards the pair's larger class.  lds: bq_vote_lds_bytes(ncls) bytes, 16-byte
// aligned; lane: the thread's index in [0, BQ_VOTE_ROWS).  Y: null, or the row's ncls entries of the decision matrix (stride 1).
// Returns np.argmax of those entries: the first NaN if there is one, else the first maximum.  With ncls = 2 that is
// OneVsOneSVC.predict's class, 1 exactly when Y[1] > 0: a positive value votes for 1 and adds less than 1/3 to it, any other finite
// value votes for 0, and a NaN or an infinity makes both entries NaN, which argmax answers with 0 as `NaN > 0` does.
template <class Dec>
__device__ __forceinline__ int bq_ovo_vote_row(int ncls, Dec dec, double *lds, int lane, double *__restrict__ Y) {
#pragma clang fp contract(off)
    double *conf = lds + lane;
    int *votes = reinterpret_cast<int *>(lds + ncls * BQ_VOTE_ROWS) + lane;
    for (int c = 0; c < ncls; ++c) {
        conf[c * BQ_VOTE_ROWS] = 0.0;
        votes[c * BQ_VOTE_ROWS] = 0;
    }
    int k = 0;
    for (int i = 0; i < ncls; ++i) {
        double ci = conf[i * BQ_VOTE_ROWS];
        int vi = votes[i * BQ_VOTE_ROWS];
        for (int j = i + 1; j < ncls; ++j, ++k) {
            const double d = dec(k);
            ci -= d;
            conf[j * BQ_VOTE_ROWS] += d;
            if (d > 0.0) votes[j * BQ_VOTE_ROWS] += 1;
            else vi += 1;
        }
        conf[i * BQ_VOTE_ROWS] = ci;
        votes[i * BQ_VOTE_ROWS] = vi;
    }
    int best = 0;
    double ybest = 0.0;
    bool open = true;   // no NaN met yet
    for (int c = 0; c < ncls; ++c) {
        const double cf = conf[c * BQ_VOTE_ROWS];
        const double y = (double)votes[c * BQ_VOTE_ROWS] + cf / (3.0 * (fabs(cf) + 1.0));
        if (Y) Y[c] = y;
        if (c == 0) {
            ybest = y;
        } else if (open && (y != y || y > ybest)) {
            best = c;
            ybest = y;
        }
        if (y != y) open = false;
    }
    return best;
}
