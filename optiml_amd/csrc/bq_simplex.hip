// The nu-one-class dual on the resident Gram panel: min 1/2 x'Kx over the capped simplex {0 <= x <= u, sum x = r}, k columns with
// their own (u, r) on one panel (sklearn OneClassSVM: u = 1, r = nu n; a column's zero-width rows are rows it does not train on).
// The equality row cannot be regularised away as in the SVC / SVR duals (without it x = 0 is optimal), so the feasible set is not a
// box and the step is a Euclidean projection onto the capped simplex:
//   P(v) = clip(v - tau, 0, u),  tau a root of phi(tau) = sum_i clip(v_i - tau, 0, u_i) = r.
// Around it runs a nonmonotone spectral projected-gradient iteration (Birgin, Martinez & Raydan's SPG with a Barzilai-Borwein step
// and an exact minimiser on the segment where the nonmonotone test refuses the full step).  Per iteration of all live columns:
//   top      (one workgroup)      the record of the iteration, the stop tests (libsvm's maximal-violating-pair measure <= tol,
//                                 max_iter), and the live columns in column order -> pos[], *nlive (mlive_kernel's job)
//   project  (one workgroup per column)  d = P(x - s g) - x, W[:, pos[c]] = d, g'd, d'd; g'd >= 0 stops the column
//   product  bq_launch_symmw, one panel stream per 16 live columns
//   close    (one workgroup per column)  d'Qd, the step length, x, g, f, s, the window of f, the violation at the new point
// The projection holds nothing of size n: it reads x, g, u from L2 in passes of 1024 threads, thread t the elements t, t + 1024, ...
// in ascending order.  tau is bracketed by an 8-section search — a pass evaluates phi at the 7 interior points of the bracket and
// counts, in the same pass, the breakpoints (v_i and v_i - u_i) below and at every point — and is finished exactly: once no
// breakpoint lies strictly inside the bracket, phi is one linear piece there and tau is its root.  Every reduction is the fixed
// tree of sx_block (a butterfly inside each wavefront, the 16 wavefronts in order), so a column's bits depend on its own
// (x, g, s, u, r) alone: not on the batch, not on its slot.  A column is one workgroup; nothing waits on another workgroup.
//
// The two-group layouts (LABELS, PAIRED: the nu-SVC / nu-SVR duals, libsvm's solve_nu_svc / solve_nu_svr) are min 1/2 b'Kb + q'x
// with b the signed, folded x, over the product of two capped simplices on disjoint groups of variables.  The projection onto a
// product is the two projections taken independently: the search runs on one workgroup per (column, group), sx_tau_kernel, each
// leaving its tau in the column's state, and the column's direction pass, sx_dir_kernel, follows.  Every kernel is one template over
// the layout; ONE (one group, no labels, no linear term) is decided at compile time, so its instantiations hold none of the other
// layouts' arithmetic (q + K b would turn a -0.0 of K b into +0.0) and search inside the direction pass, as one launch.
//
// BLOCKS is the two-group column of a class pair (a, b), a < b, on a class-sorted panel (bq_symmp.hip: class c is the rows
// [256 ct[c], 256 ct[c + 1])), the nu-SVC dual of one-vs-one classification: group 0 is class b's row range with sign +1, group 1
// class a's with sign -1, with no labels vector and no linear term.  The search and the offsets run on a group's own range (no
// predicate), the other passes walk the concatenation of the two ranges, class a's rows first, and no row outside them is read or
// written: the routed product (bq_launch_symmp) reads W and writes OUT on the pair's rows only, by column, so pos[] is the identity.
#include "bq_common.h"
#include "bq_scratch.h"
#include "bq_simplex.h"

#include <cmath>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)   // x - s g, x + a d, the scalar recurrences: the roundings of the NumPy statements, no fused multiply-add

constexpr int SX_T = 1024, SX_WAVES = SX_T / 64;
constexpr int SX_M = 8;   // sections per pass of the search
// Every pass cuts the bracket to an eighth, and a bracket of two adjacent doubles holds no breakpoint: from the widest bracket the
// entry points admit (below 2^1023) to adjacent subnormals that is under 2100 / 3 = 700 passes.  Reached only when tau lies next to a
// breakpoint many binades below the bracket's width; about log8(2 n) passes otherwise.  The cap is never the exit for finite input.
constexpr int SX_MAX_PASS = 1024;

enum { SX_SUM = 0, SX_MAX = 1 };

// a value every lane holds alike, moved to scalar registers (the search's points and totals are uniform over the workgroup)
__device__ inline double sx_uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the workgroup's fixed tree over NV values per thread: butterfly over the wavefront, then the 16 wavefronts in ascending order;
// every thread returns with the totals.  lds: (SX_WAVES + 1) * NV doubles
template <int OP, int NV>
__device__ inline void sx_block(double (&v)[NV], double *lds) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(v[i], off, 64);
            v[i] = OP == SX_SUM ? v[i] + o : fmax(v[i], o);
        }
    __syncthreads();   // the totals of the call before have been read
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[wv * NV + i] = v[i];
    __syncthreads();
    if (tid < NV) {
        double s = lds[tid];
        for (int w = 1; w < SX_WAVES; ++w) s = OP == SX_SUM ? s + lds[w * NV + tid] : fmax(s, lds[w * NV + tid]);
        lds[SX_WAVES * NV + tid] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = sx_uniform(lds[SX_WAVES * NV + i]);
}

// sx_block<SX_SUM> for counts (the integer sum is exact in any order; the same walk)
template <int NV>
__device__ inline void sx_block_count(int (&v)[NV], int *lds) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[wv * NV + i] = v[i];
    __syncthreads();
    if (tid < NV) {
        int s = lds[tid];
        for (int w = 1; w < SX_WAVES; ++w) s += lds[w * NV + tid];
        lds[SX_WAVES * NV + tid] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = __builtin_amdgcn_readfirstlane(lds[SX_WAVES * NV + i]);
}

constexpr int SX_LDS = (SX_WAVES + 1) * (2 * SX_M);   // doubles; the widest call: the search pass's 2 SX_M counts (ints)

// v_i = x_i - s g_i (x null: 0; g null: x_i), two roundings
__device__ inline double sx_v(const double *__restrict__ x, const double *__restrict__ g, double s, long long i) {
    const double xi = x ? x[i] : 0.0;
    return g ? xi - s * g[i] : xi;
}

// phi's term of a row at a point tau of the search: clip(v - tau, 0, u), decided by comparing tau with the row's breakpoints v and
// b = fl(v - u)
__device__ inline double sx_clip(double v, double b, double u, double tau) {
    if (v <= tau) return 0.0;
    if (b >= tau) return u;
    return fmin(fmax(v - tau, 0.0), u);
}

// tau as the projection leaves it: the closed bracket [lo, hi] that holds it and has no breakpoint strictly inside, and tau itself
// as an unevaluated sum th + tl (|tl| <= ulp(th) / 2).  With tau in one double, sum P moves in steps of (free rows) x ulp(tau);
// with the pair, P_i = (v_i - th) - tl carries the rounding of its own value only.
struct sx_tau {
    double lo, hi, th, tl;
};

// P_i from the bracket: rows whose upper breakpoint v is at or below it give exactly 0, rows whose lower breakpoint b = fl(v - u) is
// at or above it exactly u, the others clip((v - th) - tl, 0, u)
__device__ inline double sx_point(double v, double b, double u, const sx_tau &t) {
    if (v <= t.lo) return 0.0;
    if (b >= t.hi) return u;
    return fmin(fmax((v - t.th) - t.tl, 0.0), u);
}

// s + e = a + b exactly
__device__ inline void sx_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// (h, l) += (a, b) in double-double
__device__ inline void sx_dd_add(double &h, double &l, double a, double b) {
    double s, e;
    sx_two_sum(h, a, s, e);
    e += l + b;
    h = s + e;
    l = e - (h - s);
}
// sx_block<SX_SUM> for one double-double value per thread (the two operands of every step enter alike: both lanes of a butterfly
// step hold the same bits)
__device__ inline void sx_block_dd(double &h, double &l, double *lds) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double oh = __shfl_xor(h, off, 64), ol = __shfl_xor(l, off, 64);
        double s, e;
        sx_two_sum(h, oh, s, e);
        e += l + ol;
        h = s + e;
        l = e - (h - s);
    }
    __syncthreads();
    if (lane == 0) {
        lds[2 * wv] = h;
        lds[2 * wv + 1] = l;
    }
    __syncthreads();
    if (tid == 0) {
        double th = lds[0], tl = lds[1];
        for (int w = 1; w < SX_WAVES; ++w) sx_dd_add(th, tl, lds[2 * w], lds[2 * w + 1]);
        lds[2 * SX_WAVES] = th;
        lds[2 * SX_WAVES + 1] = tl;
    }
    __syncthreads();
    h = sx_uniform(lds[2 * SX_WAVES]);
    l = sx_uniform(lds[2 * SX_WAVES + 1]);
}

// the box of row i as one group's search sees it: ub[i], or with labels ub[i] on the rows whose sign is the group's (want) and 0 on
// the others, which the search then passes over like any row without a box (sgn null: the group is an index range with its own
// pointers; a null the caller writes as such is decided at compile time)
__device__ inline double sx_box(const double *__restrict__ ub, const double *__restrict__ sgn, double want, long long i) {
    if (sgn != nullptr && sgn[i] != want) return 0.0;
    return ub[i];
}

// tau of P(x - s g) onto {0 <= p <= ub, sum p = mass}; full: mass >= sum ub (P = ub).  Every thread returns the same value.
__device__ __forceinline__ sx_tau sx_find_tau(long long n, const double *__restrict__ x, const double *__restrict__ g, double s,
                                              const double *__restrict__ ub, const double *__restrict__ sgn, double want, double mass,
                                              int full, double *lds) {
    const int tid = threadIdx.x;
    double lo, hi;
    {   // the bracket: phi(min (v - u)) = sum u >= mass > 0 = phi(max v)
        double m[2] = {-INFINITY, -INFINITY};
        for (long long i = tid; i < n; i += SX_T) {
            const double u = sx_box(ub, sgn, want, i);
            if (u > 0.0) {
                const double v = sx_v(x, g, s, i);
                m[0] = fmax(m[0], v);
                m[1] = fmax(m[1], -(v - u));
            }
        }
        sx_block<SX_MAX>(m, lds);
        hi = m[0];
        lo = -m[1];
    }
    if (!(hi > -INFINITY)) return sx_tau{INFINITY, INFINITY, INFINITY, 0.0};   // no row with a box: P = 0
    if (full) return sx_tau{-INFINITY, -INFINITY, -INFINITY, 0.0};            // below every breakpoint: sx_point gives ub itself
    for (int pass = 0; pass < SX_MAX_PASS; ++pass) {
        double t[SX_M + 1];
        const double w = hi - lo;
        t[0] = lo;
        t[SX_M] = hi;
#pragma unroll
        for (int j = 1; j < SX_M; ++j) t[j] = fmin(fmax(lo + w * (j * (1.0 / SX_M)), lo), hi);
        double phi[SX_M - 1];
        int below[SX_M + 1], upto[SX_M + 1];   // breakpoints < t[j], <= t[j] (2 n < 2^31)
#pragma unroll
        for (int j = 0; j < SX_M - 1; ++j) phi[j] = 0.0;
#pragma unroll
        for (int j = 0; j <= SX_M; ++j) below[j] = upto[j] = 0;
#pragma unroll 1
        for (long long i = tid; i < n; i += SX_T) {
            const double u = sx_box(ub, sgn, want, i);
            if (!(u > 0.0)) continue;
            const double v = sx_v(x, g, s, i), b = v - u;
#pragma unroll
            for (int j = 1; j < SX_M; ++j) phi[j - 1] += sx_clip(v, b, u, t[j]);
#pragma unroll
            for (int j = 0; j <= SX_M; ++j) {
                below[j] += (v < t[j]) + (b < t[j]);
                upto[j] += (v <= t[j]) + (b <= t[j]);
            }
        }
        sx_block<SX_SUM>(phi, lds);
        int cnt[2 * SX_M];   // below[1 .. SX_M], upto[0 .. SX_M - 1]
#pragma unroll
        for (int j = 0; j < SX_M; ++j) {
            cnt[j] = below[j + 1];
            cnt[SX_M + j] = upto[j];
        }
        sx_block_count(cnt, (int *)lds);
        // the section up to the first point with phi < mass (phi(hi) < mass by the invariant) and the breakpoints strictly inside it;
        // constant indices only: the arrays stay in registers
        bool found = false;
        int inside = 0;
#pragma unroll
        for (int j = 1; j <= SX_M; ++j) {
            const bool take = !found && (j == SX_M || phi[j < SX_M ? j - 1 : 0] < mass);
            if (take) {
                lo = t[j - 1];
                hi = t[j];
                inside = cnt[j - 1] - cnt[SX_M + j - 1];
                found = true;
            }
        }
        if (inside <= 0) break;
    }
    // the linear piece on [lo, hi]: rows with v <= lo give 0, rows with v - u >= hi give u, the others v - tau, so
    // tau = lo + (sum (v - lo) + sum u - mass) / (free rows); the sums in double-double (v - lo split exactly)
    double sh = 0.0, sl = 0.0;
    int cnt[1] = {0};
    for (long long i = tid; i < n; i += SX_T) {
        const double u = sx_box(ub, sgn, want, i);
        if (!(u > 0.0)) continue;
        const double v = sx_v(x, g, s, i), b = v - u;
        if (v <= lo) continue;
        if (b >= hi) sx_dd_add(sh, sl, u, 0.0);
        else {
            double dh, dl;
            sx_two_sum(v, -lo, dh, dl);
            sx_dd_add(sh, sl, dh, dl);
            cnt[0] += 1;
        }
    }
    sx_block_dd(sh, sl, lds);
    sx_block_count(cnt, (int *)lds);
    sx_tau t{lo, hi, lo, 0.0};
    if (cnt[0] > 0) {
        const double delta = ((sh - mass) + sl) / (double)cnt[0];
        sx_two_sum(lo, delta, t.th, t.tl);
        if (t.th < lo || (t.th == lo && t.tl < 0.0)) t.th = lo, t.tl = 0.0;
        if (t.th > hi || (t.th == hi && t.tl > 0.0)) t.th = hi, t.tl = 0.0;
    }
    return t;
}

// bq_simplex_project: P[:, column] = P(V[:, column]), the same search and the same clip
__global__ __launch_bounds__(SX_T) void sx_project_only_kernel(long long n, const double *__restrict__ V, const double *__restrict__ UB,
                                                               const double *__restrict__ mass, const int *__restrict__ full,
                                                               double *__restrict__ P) {
    __shared__ double lds[SX_LDS];
    const double *v = V + (long long)blockIdx.x * n, *ub = UB + (long long)blockIdx.x * n;
    double *p = P + (long long)blockIdx.x * n;
    const sx_tau tau = sx_find_tau(n, v, nullptr, 0.0, ub, nullptr, 0.0, mass[blockIdx.x], full[blockIdx.x], lds);
    for (long long i = threadIdx.x; i < n; i += SX_T) {
        const double u = ub[i], vi = v[i];
        p[i] = u > 0.0 ? sx_point(vi, vi - u, u, tau) : 0.0;
    }
}

// group t of a column as the search and the offsets take it: an index range with its own pointers (ONE: the column; PAIRED: the rows
// t n ... t n + n - 1; sgn null) or a predicate on the labels (LABELS: all n rows, the rows with sgn = +1 for t = 0, -1 for t = 1)
// (BLOCKS: the group's own row range of the class-sorted panel, len rows of it: no predicate, and no row of another class is read)
struct sx_group {
    long long off;
    const double *sgn;
    double want;
    long long len;
};
template <int L>
__device__ inline sx_group sx_group_of(const bq_sx_col &c, int t) {
    if constexpr (L == BQ_SX_LABELS) return sx_group{0, c.sgn, t == 0 ? 1.0 : -1.0, c.n};
    else if constexpr (L == BQ_SX_BLOCKS) return sx_group{t == 0 ? c.goff[0] : c.goff[1], nullptr, 0.0, t == 0 ? c.glen[0] : c.glen[1]};
    else return sx_group{t * c.n, nullptr, 0.0, c.n};
}
template <int L>
constexpr int SX_GROUPS = L == BQ_SX_ONE ? 1 : 2;
template <int L>
constexpr bool SX_LINEAR = L == BQ_SX_LABELS || L == BQ_SX_PAIRED;   // the layouts with a linear term q

// the panel rows a column's kernels walk: e = 0 ... sx_rows - 1 is panel row sx_row_at(e).  BLOCKS: the concatenation of the two
// ranges, class a's rows (group 1) first; else the n rows
template <int L>
__device__ inline long long sx_rows(const bq_sx_col &c) {
    if constexpr (L == BQ_SX_BLOCKS) return c.glen[1] + c.glen[0];
    else return c.n;
}
template <int L>
__device__ inline long long sx_row_at(const bq_sx_col &c, long long e) {
    if constexpr (L == BQ_SX_BLOCKS) return e < c.glen[1] ? c.goff[1] + e : c.goff[0] + (e - c.glen[1]);
    else return e;
}

// the variables of panel row i, fn(j, group, s_j v): the variable, its group and the panel's value v there under the variable's sign
template <int L, class F>
__device__ inline void sx_row(const bq_sx_col &c, long long i, double v, F &&fn) {
    if constexpr (L == BQ_SX_PAIRED) {
        fn(i, 0, v);
        fn(c.n + i, 1, -v);
    } else if constexpr (L == BQ_SX_LABELS) {
        const double sg = c.sgn[i];
        fn(i, sg > 0.0 ? 0 : 1, sg * v);
    } else if constexpr (L == BQ_SX_BLOCKS) {   // (class a's range lies below class b's)
        if (i >= c.goff[0]) fn(i, 0, v);
        else fn(i, 1, -v);
    } else {
        fn(i, 0, v);
    }
}

// the search of a two-group projection: workgroup (column blockIdx.x, group blockIdx.y) leaves its group's tau in the column's
// tau[4 t ...].  init: of P(0), for the columns without an x0; else of P(x - s g), for the live columns
template <int L>
__global__ __launch_bounds__(SX_T) void sx_tau_kernel(const bq_sx_col *__restrict__ cols, int init) {
    static_assert(L != BQ_SX_ONE, "the one-group column searches inside sx_dir_kernel");
    __shared__ double lds[SX_LDS];
    const bq_sx_col c = cols[blockIdx.x];
    const int t = blockIdx.y;
    if (init ? c.has_x0 : c.sc->done) return;
    const sx_group gr = sx_group_of<L>(c, t);
    const double mass = t == 0 ? c.mass[0] : c.mass[1];   // (constant indices: the column stays in registers)
    const int full = t == 0 ? c.full[0] : c.full[1];
    const sx_tau tau = sx_find_tau(gr.len, init ? nullptr : c.x + gr.off, init ? nullptr : c.g + gr.off, init ? 0.0 : c.st->s,
                                   c.ub + gr.off, gr.sgn, gr.want, mass, full, lds);
    if (threadIdx.x == 0) {
        double *o = c.tau + 4 * t;
        o[0] = tau.lo;
        o[1] = tau.hi;
        o[2] = tau.th;
        o[3] = tau.tl;
    }
}

__device__ inline sx_tau sx_load_tau(const double *tau, int t) {
    return sx_tau{sx_uniform(tau[4 * t]), sx_uniform(tau[4 * t + 1]), sx_uniform(tau[4 * t + 2]), sx_uniform(tau[4 * t + 3])};
}

// the direction pass of column blockIdx.x (two groups: after sx_tau_kernel; ONE: the search first, here), thread i, i + 1024, ... on
// panel row i (ONE: the variable i; LABELS: the variable i of the group its label names; PAIRED: the variables i of group 0 and n + i
// of group 1).  init: x = P(0) per group (the columns without an x0) and W[:, column] = the signed, folded x.  Else, for a live
// column: d = P(x - s g) - x with each variable's own group's tau, W[:, pos[column]] = d (ONE), sgn o d (LABELS) or d_i - d_{n + i}
// (PAIRED), g'd and d'd over all m variables; g'd >= 0: 'optimal'.  BLOCKS: thread e, e + 1024, ... on element e of the two ranges'
// concatenation (sx_row_at), the variable of that row in the group whose range holds it, W = d on class b's rows and -d on class a's
template <int L>
__global__ __launch_bounds__(SX_T) void sx_dir_kernel(const bq_sx_col *__restrict__ cols, const int *__restrict__ pos,
                                                      double *__restrict__ W, int64_t ldw, int init) {
    __shared__ double lds[SX_LDS];
    const bq_sx_col c = cols[blockIdx.x];
    const long long n = c.n;
    const int tid = threadIdx.x;
    if (!init && c.sc->done) return;
    const bool fresh = init && !c.has_x0;   // x is written here
    const double s = init ? 0.0 : c.st->s;
    sx_tau tau[2] = {sx_tau{0.0, 0.0, 0.0, 0.0}, sx_tau{0.0, 0.0, 0.0, 0.0}};
    if constexpr (L == BQ_SX_ONE) {
        if (fresh) tau[0] = sx_find_tau(n, nullptr, nullptr, 0.0, c.ub, nullptr, 0.0, c.mass[0], c.full[0], lds);
        else if (!init) tau[0] = sx_find_tau(n, c.x, c.g, s, c.ub, nullptr, 0.0, c.mass[0], c.full[0], lds);
    } else if (!init || fresh) {
        tau[0] = sx_load_tau(c.tau, 0);
        tau[1] = sx_load_tau(c.tau, 1);
    }
    double *w = W + (int64_t)(init ? (int)blockIdx.x : pos[blockIdx.x]) * ldw;
    double a[2] = {0.0, 0.0};
    // the new value of variable j in group t: the start point, or the direction (its terms of g'd and d'd added)
    auto variable = [&](long long j, int t) -> double {
        const double u = c.ub[j];
        if (init) {
            if (fresh) c.x[j] = u > 0.0 ? sx_point(0.0, 0.0 - u, u, tau[t]) : 0.0;
            return c.x[j];
        }
        const double xj = c.x[j], gj = c.g[j];
        const double v = xj - s * gj;
        const double p = u > 0.0 ? sx_point(v, v - u, u, tau[t]) : 0.0;
        const double d = p - xj;
        c.d[j] = d;
        a[0] += gj * d;
        a[1] += d * d;
        return d;
    };
    const long long rows = sx_rows<L>(c);
    for (long long e = tid; e < rows; e += SX_T) {
        const long long i = sx_row_at<L>(c, e);
        if constexpr (L == BQ_SX_PAIRED) {
            const double lo = variable(i, 0), hi = variable(n + i, 1);
            w[i] = lo - hi;
        } else if constexpr (L == BQ_SX_LABELS) {
            const double sg = c.sgn[i];
            w[i] = sg * variable(i, sg > 0.0 ? 0 : 1);
        } else if constexpr (L == BQ_SX_BLOCKS) {
            if (i >= c.goff[0]) w[i] = variable(i, 0);
            else w[i] = -variable(i, 1);
        } else {
            w[i] = variable(i, 0);
        }
    }
    if (init) return;
    sx_block<SX_SUM>(a, lds);
    if (tid == 0) {
        c.st->gd = a[0];
        c.st->dd = a[1];
        if (a[0] >= 0.0) {
            c.sc->status = BQ_STATUS_OPTIMAL;
            c.sc->done = 1;
        }
    }
}

// libsvm's measure, per group max_{u > 0, x > 0} g - min_{u > 0, x < u} g (a group with an empty side gives -inf) and the maximum
// over the groups (Solver_NU).  m: per group the max of g over x > 0 and the max of -g over x < u, of the elements a thread holds
template <int NM>
__device__ inline void sx_viol_add(double (&m)[NM], int t, double x, double g, double u) {
    if (u > 0.0) {
        if (x > 0.0) m[2 * t] = fmax(m[2 * t], g);
        if (x < u) m[2 * t + 1] = fmax(m[2 * t + 1], -g);
    }
}
template <int NM>
__device__ inline double sx_viol(const double (&m)[NM]) {
    double v = (m[0] > -INFINITY && m[1] > -INFINITY) ? m[0] + m[1] : -INFINITY;
    if constexpr (NM == 4) v = fmax(v, (m[2] > -INFINITY && m[3] > -INFINITY) ? m[2] + m[3] : -INFINITY);
    return v;
}

// one thread: the state of a column at its start point: f, the violation, s = 1 and the window [f]
__device__ inline void sx_begin(bq_scal *sc, bq_sx_state &st, double f, double viol) {
    sc->f = f;
    st.viol = viol;
    st.s = 1.0;
    st.alpha = 0.0;
    st.win[0] = f;
    st.nwin = 1;
    if (!(fabs(f) <= 1.7976931348623157e308)) {
        sc->status = BQ_ERR_NONFINITE;
        sc->done = 1;
    }
}

// the step of an iteration from d'Qd and the column's state (every thread, before thread 0 writes the state): a = 1 if
// f + g'd + 1/2 d'Qd <= max(window) + 1e-4 g'd, else the minimiser -g'd / d'Qd of the segment; f at the new point;
// s = clamp(d'd / d'Qd) (1e10 where d'Qd <= 0)
struct sx_step {
    double alpha, fnew, snew;
    int nwin;
};
__device__ inline sx_step sx_step_of(const bq_scal *sc, const bq_sx_state *st, double dQd) {
    const double f = sc->f, gd = st->gd, dd = st->dd;
    const int nwin = st->nwin;
    double fmx = st->win[0];
    for (int j = 1; j < nwin; ++j) fmx = fmax(fmx, st->win[j]);
    double alpha = 1.0;
    if (!(f + gd + 0.5 * dQd <= fmx + 1e-4 * gd)) alpha = -gd / dQd;
    const double fnew = f + (alpha * gd + 0.5 * alpha * alpha * dQd);
    const double snew = dQd > 0.0 ? fmin(fmax(dd / dQd, 1e-10), 1e10) : 1e10;
    return sx_step{alpha, fnew, snew, nwin};
}

// one thread: the state at the new point, the window, iter + 1
__device__ inline void sx_commit(bq_scal *sc, bq_sx_state &st, const sx_step &p, double viol) {
    sc->f = p.fnew;
    st.alpha = p.alpha;
    st.s = p.snew;
    st.viol = viol;
    if (p.nwin < BQ_SX_WINDOW) {
        st.win[p.nwin] = p.fnew;
        st.nwin = p.nwin + 1;
    } else {
        for (int j = 1; j < BQ_SX_WINDOW; ++j) st.win[j - 1] = st.win[j];
        st.win[BQ_SX_WINDOW - 1] = p.fnew;
    }
    sc->iter += 1;
    if (!(fabs(p.fnew) <= 1.7976931348623157e308)) {
        sc->status = BQ_ERR_NONFINITE;
        sc->done = 1;
    }
}

// after the start-up product (OUT[:, column] = K b, b the folded x), column blockIdx.x: g_j = q_j + s_j (K b)_{j mod n},
// f = 1/2 x'(g - q) + q'x (ONE: g = K x, f = 1/2 x'g, nothing added), the violation, s = 1 and the window [f]
template <int L>
__global__ __launch_bounds__(SX_T) void sx_start_kernel(const bq_sx_col *__restrict__ cols, const double *__restrict__ out, int64_t ldw) {
    __shared__ double lds[SX_LDS];
    const bq_sx_col c = cols[blockIdx.x];
    const double *Kb = out + (int64_t)blockIdx.x * ldw;
    double a[SX_LINEAR<L> ? 2 : 1] = {}, m[2 * SX_GROUPS<L>];
    for (double &v : m) v = -INFINITY;
    const long long rows = sx_rows<L>(c);
    for (long long e = threadIdx.x; e < rows; e += SX_T) {
        const long long i = sx_row_at<L>(c, e);
        sx_row<L>(c, i, Kb[i], [&](long long j, int t, double sKb) {
            const double xj = c.x[j];
            double gj = sKb;
            if constexpr (!SX_LINEAR<L>) {
                a[0] += xj * gj;
            } else {
                const double qj = c.q ? c.q[j] : 0.0;
                gj = qj + sKb;
                a[0] += xj * (gj - qj);
                a[1] += qj * xj;
            }
            c.g[j] = gj;
            sx_viol_add(m, t, xj, gj, c.ub[j]);
        });
    }
    sx_block<SX_SUM>(a, lds);
    sx_block<SX_MAX>(m, lds);
    double f = 0.5 * a[0];
    if constexpr (SX_LINEAR<L>) f += a[1];
    if (threadIdx.x == 0) sx_begin(c.sc, *c.st, f, sx_viol(m));
}

// the close of an iteration, live column blockIdx.x, Qd_j = s_j OUT[j mod n, pos[column]]: d'Qd over all m variables; a = 1 if
// f + g'd + 1/2 d'Qd <= max(window) + 1e-4 g'd, else the minimiser -g'd / d'Qd of the segment; f, x, g at the new point, the window,
// s = clamp(d'd / d'Qd) (1e10 where d'Qd <= 0), the violation there, iter + 1
template <int L>
__global__ __launch_bounds__(SX_T) void sx_close_kernel(const bq_sx_col *__restrict__ cols, const int *__restrict__ pos,
                                                        const double *__restrict__ out, int64_t ldw) {
    __shared__ double lds[SX_LDS];
    const bq_sx_col c = cols[blockIdx.x];
    if (c.sc->done) return;
    const double *Kd = out + (int64_t)pos[blockIdx.x] * ldw;
    const int tid = threadIdx.x;
    double a[1] = {0.0};
    const long long rows = sx_rows<L>(c);
    for (long long e = tid; e < rows; e += SX_T) {
        const long long i = sx_row_at<L>(c, e);
        sx_row<L>(c, i, Kd[i], [&](long long j, int, double Qd) { a[0] += c.d[j] * Qd; });
    }
    sx_block<SX_SUM>(a, lds);
    const sx_step p = sx_step_of(c.sc, c.st, a[0]);
    double m[2 * SX_GROUPS<L>];
    for (double &v : m) v = -INFINITY;
    for (long long e = tid; e < rows; e += SX_T) {
        const long long i = sx_row_at<L>(c, e);
        sx_row<L>(c, i, Kd[i], [&](long long j, int t, double Qd) {
            const double xj = c.x[j] + p.alpha * c.d[j], gj = c.g[j] + p.alpha * Qd;
            c.x[j] = xj;
            c.g[j] = gj;
            sx_viol_add(m, t, xj, gj, c.ub[j]);
        });
    }
    sx_block<SX_MAX>(m, lds);   // (its barriers: every thread has read the state before thread 0 writes it)
    if (tid == 0) sx_commit(c.sc, *c.st, p, sx_viol(m));
}

// the top of an iteration (one workgroup): thread c, c + 1024, ... writes the record of its live column (iter, f, violation, the
// last step length, s) and takes the stop tests; then thread 0 numbers the live columns in column order (mlive_kernel)
__global__ __launch_bounds__(SX_T) void sx_top_kernel(const bq_sx_col *__restrict__ cols, int k, int *__restrict__ pos, int *__restrict__ nlive) {
    for (int c = threadIdx.x; c < k; c += SX_T) {
        const bq_sx_col &col = cols[c];
        bq_scal *sc = col.sc;
        if (sc->done) continue;
        const bq_sx_state &st = *col.st;
        const long long r = sc->iter - sc->stat_base;
        if (col.stats != nullptr && r >= 0 && r < sc->stat_cap) col.stats[r] = bq_iter_stat{(int64_t)sc->iter, sc->f, st.viol, st.alpha, st.s};
        if (st.viol <= sc->eps) {
            sc->status = BQ_STATUS_OPTIMAL;
            sc->done = 1;
        } else if (sc->iter >= sc->max_iter) {
            sc->status = BQ_STATUS_STOPPED;
            sc->done = 1;
        }
    }
    if (pos == nullptr) return;   // the routed product: column = pair, and its plan's live kernel follows
    __syncthreads();
    if (threadIdx.x != 0) return;
    int s = 0;
    for (int c = 0; c < k; ++c)
        if (!cols[c].sc->done) pos[c] = s++;
    *nlive = s;
}

// libsvm's calculate_rho over the rows with a box (sx_box: of one group), exact comparisons: the support and free
// counts, the largest g at the upper bound and the smallest at 0 by the tree; the free rows' sum of g in index order — the first
// wavefront loads 64 rows at a time and adds the free ones among them one after another, lowest row first.  Thread 0 writes.
__device__ inline void sx_offsets_of(long long n, const double *__restrict__ xs, const double *__restrict__ gs,
                                     const double *__restrict__ ub, const double *__restrict__ sgn, double want, double *lds,
                                     double *__restrict__ rho, long long *__restrict__ n_sv, long long *__restrict__ n_free) {
    double m[2] = {-INFINITY, -INFINITY};   // m[0]: max g at x = u; m[1]: max -g at x = 0
    int cnt[2] = {0, 0};                    // rows with x > 0; rows with 0 < x < u
    for (long long i = threadIdx.x; i < n; i += SX_T) {
        const double u = sx_box(ub, sgn, want, i), x = xs[i], g = gs[i];
        if (!(u > 0.0)) continue;
        cnt[0] += x > 0.0;
        cnt[1] += x > 0.0 && x < u;
        if (x == u) m[0] = fmax(m[0], g);
        if (x == 0.0) m[1] = fmax(m[1], -g);
    }
    sx_block_count(cnt, (int *)lds);
    sx_block<SX_MAX>(m, lds);
    if (threadIdx.x >= 64) return;
    double r;
    if (cnt[1] > 0) {
        double s = 0.0;
        for (long long base = 0; base < n; base += 64) {
            const long long i = base + threadIdx.x;
            bool fr = false;
            double gv = 0.0;
            if (i < n) {
                const double u = sx_box(ub, sgn, want, i), x = xs[i];
                fr = u > 0.0 && x > 0.0 && x < u;
                gv = gs[i];
            }
            unsigned long long mask = __ballot(fr);
            while (mask) {   // (the same for every lane)
                s += __shfl(gv, __ffsll((long long)mask) - 1, 64);
                mask &= mask - 1;
            }
        }
        r = s / (double)cnt[1];
    } else {
        r = (-m[1] + m[0]) / 2;
    }
    if (threadIdx.x != 0) return;
    *rho = r;
    *n_sv = cnt[0];
    *n_free = cnt[1];
}

// workgroup (column blockIdx.x, group blockIdx.y) -> r / n_sv / n_free[groups x column + group]
template <int L>
__global__ __launch_bounds__(SX_T) void sx_offsets_kernel(const bq_sx_col *__restrict__ cols, double *__restrict__ r,
                                                          long long *__restrict__ n_sv, long long *__restrict__ n_free) {
    __shared__ double lds[SX_LDS];
    const bq_sx_col c = cols[blockIdx.x];
    const sx_group gr = sx_group_of<L>(c, blockIdx.y);
    const int o = SX_GROUPS<L> * blockIdx.x + blockIdx.y;
    sx_offsets_of(gr.len, c.x + gr.off, c.g + gr.off, c.ub + gr.off, gr.sgn, gr.want, lds, r + o, n_sv + o, n_free + o);
}

// fn(the layout as a constant): the instantiations of a launcher, chosen once
template <class F>
static void sx_with_layout(int layout, F &&fn) {
    if (layout == BQ_SX_ONE) fn(std::integral_constant<int, BQ_SX_ONE>{});
    else if (layout == BQ_SX_PAIRED) fn(std::integral_constant<int, BQ_SX_PAIRED>{});
    else if (layout == BQ_SX_BLOCKS) fn(std::integral_constant<int, BQ_SX_BLOCKS>{});
    else fn(std::integral_constant<int, BQ_SX_LABELS>{});
}

int bq_sx_launch_project(const bq_sx_col *cols, int k, int layout, const int *pos, double *W, int64_t ldw, bool init, hipStream_t st) {
    sx_with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if constexpr (L != BQ_SX_ONE) sx_tau_kernel<L><<<dim3(k, 2), SX_T, 0, st>>>(cols, init ? 1 : 0);
        sx_dir_kernel<L><<<k, SX_T, 0, st>>>(cols, pos, W, ldw, init ? 1 : 0);
    });
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_sx_launch_start(const bq_sx_col *cols, int k, int layout, const double *out, int64_t ldw, hipStream_t st) {
    sx_with_layout(layout, [&](auto l) { sx_start_kernel<decltype(l)::value><<<k, SX_T, 0, st>>>(cols, out, ldw); });
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_sx_launch_close(const bq_sx_col *cols, int k, int layout, const int *pos, const double *out, int64_t ldw, hipStream_t st) {
    sx_with_layout(layout, [&](auto l) { sx_close_kernel<decltype(l)::value><<<k, SX_T, 0, st>>>(cols, pos, out, ldw); });
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_sx_launch_top(const bq_sx_col *cols, int k, int *pos, int *nlive, hipStream_t st) {
    sx_top_kernel<<<1, SX_T, 0, st>>>(cols, k, pos, nlive);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_sx_launch_offsets(const bq_sx_col *cols, int k, int layout, double *r, long long *n_sv, long long *n_free, hipStream_t st) {
    sx_with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        sx_offsets_kernel<L><<<dim3(k, SX_GROUPS<L>), SX_T, 0, st>>>(cols, r, n_sv, n_free);
    });
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_sx_check(int k, int64_t n, const double *UB, const double *mass, int *full) {
    for (int c = 0; c < k; ++c) {
        long double sum = 0.0L;
        for (int64_t i = 0; i < n; ++i) {
            const double u = UB[(int64_t)c * n + i];
            BQ_ARG(u >= 0.0 && u <= BQ_SX_MAX_ABS, "the boxes must lie in [0, 2^1021]");
            sum += u;
        }
        const double s = (double)sum;
        BQ_ARG(mass[c] > 0.0 && std::isfinite(mass[c]), "mass must be > 0");
        // sum u as the caller formed it may differ from this one in its last bits: a mass within n roundings of it is the whole box
        BQ_ARG(mass[c] <= s * (1.0 + (double)n * 2.220446049250313e-16), "mass must be <= the sum of the column's box");
        full[c] = mass[c] >= s ? 1 : 0;
    }
    return BQ_OK;
}

extern "C" int bq_simplex_project(bq_ctx *c, int k, int64_t n, const double *V, const double *UB, const double *mass, double *P) {
    BQ_ARG(c && V && UB && mass && P, "NULL argument");
    BQ_ARG(k >= 1 && n >= 1, "k and n must be >= 1");
    std::vector<int> full((size_t)k);
    BQ_TRY(bq_sx_check(k, n, UB, mass, full.data()));
    // (with the boxes' limit the first bracket, max v - min (v - u), stays below 2^1023: its width does not overflow)
    for (int64_t i = 0; i < (int64_t)k * n; ++i) BQ_ARG(std::fabs(V[i]) <= BQ_SX_MAX_ABS, "|V| must be at most 2^1021");
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t len = sizeof(double) * (size_t)k * (size_t)n;
    bq_scratch mem;   // freed after the closing sync
    const size_t cells = (size_t)k * (size_t)n;
    double *dV = mem.dev<double>(cells), *dU = mem.dev<double>(cells), *dP = mem.dev<double>(cells), *dm = mem.dev<double>(k);
    int *df = mem.dev<int>(k);
    hipError_t e = mem.error();
    if (e == hipSuccess) e = hipMemcpyAsync(dV, V, len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dU, UB, len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dm, mass, sizeof(double) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(df, full.data(), sizeof(int) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        sx_project_only_kernel<<<k, SX_T, 0, st>>>((long long)n, dV, dU, dm, df, dP);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(P, dP, len, hipMemcpyDeviceToHost, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("bq_simplex_project: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    return bq_ctx_sync_after(c, rc);   // the host arrays are the caller's and this frame's
}
