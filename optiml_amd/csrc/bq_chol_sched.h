// The blocked Cholesky's schedule (bq_chol.hip): the arithmetic that decides which workgroup computes which tile, which path a
// size takes, and in which order and on which stream the steps of one factorisation are issued.  Plain C++ (no HIP include), shared
// by the kernels and the driver so that a host program can check it: tests/c/chol_sched_check.cpp.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BQ_SCHED_HD __host__ __device__
#else
#define BQ_SCHED_HD
#endif

constexpr int64_t BQ_CHOL_NB = 128;        // order of a block (tile)
constexpr int BQ_CHOL_EVENTS = 8;          // events of the look-ahead (bq_chol_ws::ev)
constexpr int BQ_CHOL_MAX_PASSES = 4;      // largest P
constexpr int BQ_CHOL_MAX_SLICES = 4;      // column slices of the forward sweep's block row (bq_chol_ws::tmp holds that many)
constexpr int64_t BQ_CHOL_SUPER_MIN = 8 * 512;    // tiles of a trailing triangle from which the super-tile order is used
constexpr int64_t BQ_CHOL_FWD_SLICE = 16384;      // columns per slice of the forward sweep

// ---------------------------------------------------------------------------------------------
// block id -> tile decodes
// ---------------------------------------------------------------------------------------------
// the row r of the packed lower triangle that holds element idx: r (r + 1) / 2 <= idx < (r + 1) (r + 2) / 2
BQ_SCHED_HD inline int64_t bq_chol_tri_row(int64_t idx) {
    int64_t r = (int64_t)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= idx) ++r;
    while (r * (r + 1) / 2 > idx) --r;
    return r;
}

// super-tiles of the trailing triangle of T tile rows: 0 = plain row-major order
BQ_SCHED_HD inline int64_t bq_chol_nsuper(int64_t T, int64_t super_min) {
    const int64_t S = (T + 7) / 8, ntiles = T * (T + 1) / 2;
    // super-tiles pay off once an XCD has many of them; below ~8 rounds of the chip the even split wins
    return ntiles >= super_min ? S * (S + 1) / 2 : 0;
}
BQ_SCHED_HD inline int64_t bq_chol_syrk_grid(int64_t T, int64_t nsuper) {
    return nsuper ? ((nsuper + 7) / 8) * 8 * 64 : T * (T + 1) / 2;
}
// syrk_kernel: block bid -> tile (ti >= tj) of the T x T trailing triangle; false: the block has no tile.
// nsuper == 0: small grids (a few rounds at most): plain row-major triangle, every XCD equally loaded.  Otherwise the tiles are
// grouped into 8 x 8 super-tiles and every super-tile is dealt to ONE XCD (workgroups go round-robin over the 8 XCDs by block id);
// blocks of a diagonal super-tile that fall above the diagonal, and those past the ragged edge, have no tile.
BQ_SCHED_HD inline bool bq_chol_syrk_decode(int64_t bid, int64_t T, int64_t nsuper, int64_t *ti, int64_t *tj) {
    if (nsuper == 0) {
        if (bid >= T * (T + 1) / 2) return false;
        *ti = bq_chol_tri_row(bid);
        *tj = bid - *ti * (*ti + 1) / 2;
        return true;
    }
    const int64_t slot = bid / 8;
    const int64_t sidx = (slot / 64) * 8 + bid % 8;
    if (sidx >= nsuper) return false;
    const int64_t si = bq_chol_tri_row(sidx);
    const int64_t sj = sidx - si * (si + 1) / 2;
    const int local = (int)(slot % 64);
    *ti = 8 * si + local / 8;
    *tj = 8 * sj + local % 8;
    return *ti < T && *tj <= *ti;
}

// syrk_head_kernel: the first nc block columns of the T x T trailing triangle, column after column (column tj holds T - tj tiles)
BQ_SCHED_HD inline int64_t bq_chol_head_grid(int64_t T, int nc) {
    int64_t g = 0;
    for (int c = 0; c < nc && c < T; ++c) g += T - c;
    return g;
}
BQ_SCHED_HD inline bool bq_chol_head_decode(int64_t b, int64_t T, int nc, int64_t *ti, int64_t *tj) {
    int64_t c = 0;
    while (c < nc - 1 && b >= T - c) {   // column c holds T - c tiles
        b -= T - c;
        ++c;
    }
    *ti = b + c;
    *tj = c;
    return *ti < T;
}

// ---------------------------------------------------------------------------------------------
// choices by size (hook values come in as arguments: 0 / the default = no hook)
// ---------------------------------------------------------------------------------------------
// passes per super-pass the image buffers are sized for; a forced P (hook chol_passes) gets room for any P
BQ_SCHED_HD inline int bq_chol_super_max(int64_t cap, bool passes_hooked) {
    return passes_hooked || cap >= 24576 ? BQ_CHOL_MAX_PASSES : 2;
}
// P passes per super-pass (by size): the wide update then has K = P * 256.  A larger P cuts the C traffic and the per-tile
// prologue per flop further but lengthens the narrow chain between two wide updates.
// measured (final kernel): n=50k 622 / 608 / 621 ms, n=32k 192 / 190 / 194 ms for P = 2 / 3 / 4
BQ_SCHED_HD inline int bq_chol_passes(int64_t np, int super_max, int hook) {
    const int v = hook >= 1 && hook <= BQ_CHOL_MAX_PASSES ? hook : (np >= 65536 ? 4 : (np >= 24576 ? 3 : 2));
    return v < 1 ? 1 : (v > super_max ? super_max : v);
}
// two-stream order: from 16 blocks on, where the workspace has its streams and events; hook: -1 none, 0 off, 1 on at every order
BQ_SCHED_HD inline bool bq_chol_use_lookahead(int64_t np, bool ws_lookahead, int hook) {
    if (!ws_lookahead || hook == 0) return false;
    return hook == 1 || np >= 16 * BQ_CHOL_NB;
}
// rows of a big block of the prepared sweeps (1024 for small workspaces, 2048 from order 4096, 4096 from order 8192 on)
BQ_SCHED_HD inline int64_t bq_chol_big_block(int64_t cap, int64_t hook) {
    if (hook == 1024 || hook == 2048 || hook == 4096 || hook == 8192) return hook;
    return cap >= 8192 ? 4096 : (cap >= 4096 ? 2048 : 1024);
}
// forward sweep, block row k0 of a right-hand side that vanishes before column c0 (both multiples of 128): the span [c0, k0) is
// cut into at most four slices of `unit` columns or more, each a multiple of 512 wide
BQ_SCHED_HD inline void bq_chol_fwd_slices(int64_t span, int64_t unit, int *slices, int64_t *width) {
    const int64_t want = (span + unit - 1) / unit;
    *slices = (int)(want < BQ_CHOL_MAX_SLICES ? want : BQ_CHOL_MAX_SLICES);
    *width = ((span + *slices - 1) / *slices + 511) / 512 * 512;
}
// columns [lo, hi) of slice y (hi <= lo: the slice is empty)
BQ_SCHED_HD inline void bq_chol_fwd_slice_range(int64_t c0, int64_t k0, int64_t width, int64_t y, int64_t *lo, int64_t *hi) {
    *lo = c0 + y * width;
    *hi = *lo + width < k0 ? *lo + width : k0;
}

// ---------------------------------------------------------------------------------------------
// the plan of one factorisation of order np (a multiple of 128): its steps in issue order
// ---------------------------------------------------------------------------------------------
// Two block columns per pass p (A_p = 2p*NB, B_p = A_p + NB), P passes per SUPER-PASS q (passes qP .. qP + P - 1):
//   narrow(p): diag(A) ; TRSM(A) ; narrow update of column B ; diag(B) ; TRSM(B)        -> images of pass p
//   head_in(p): the two block columns pass p+1 factors next  -= the images of the super-pass so far
//   wide(q)  : everything behind the super-pass -= X X^T with ALL its images in ONE K = P * 256 pass — a C tile is read
//              and written once per P * 256 columns factored (tools/syrk_probe.hip, final tile kernel: 69.5 / 73.6 /
//              74.3 TFLOP/s at K = 512 / 768 / 1024; with the round-1 kernel it was 0.71 of the MFMA peak at K = 256);
//              split into head (the 2P block columns the next chain works on) and rest.
// The images of a super-pass are contiguous in k, two buffers.
// With look-ahead the narrow chain of super-pass q+1 (it touches only the 2P block columns head(q) has finished) runs on
// the high-priority side stream while rest(q) keeps the chip busy.
enum bq_chol_op {
    BQ_CHOL_DIAG = 0,     // factor + invert the diagonal block at row
    BQ_CHOL_TRSM = 1,     // block column at row: the T tiles below the diagonal block; leaves their k-major image at img
    BQ_CHOL_COL = 2,      // tiles (ti, 0) of the trailing matrix at row -= the kdim = 128 image at img
    BQ_CHOL_HEAD = 3,     // the first nc block columns of the T x T trailing triangle at row -= the kdim images at img
    BQ_CHOL_REST = 4,     // the whole T x T trailing triangle at row -= the kdim images at img; nc = nsuper
    BQ_CHOL_RECORD = 5,   // record event nc on the stream
    BQ_CHOL_WAIT = 6      // the stream waits for event nc
};
enum bq_chol_stream { BQ_CHOL_ON_CTX = 0, BQ_CHOL_ON_MAIN = 1, BQ_CHOL_ON_SIDE = 2 };
struct bq_chol_step {
    int op;
    int stream;
    int64_t row;   // first row of the diagonal block / block column / trailing matrix
    int64_t img;   // image offset in image rows: the image starts at Wt + img * ldh
    int kdim;      // image rows read (updates) or written (TRSM)
    int64_t T;     // tile rows
    int64_t nc;    // HEAD: block columns; REST: nsuper; RECORD / WAIT: event index
};

// image rows of pass p's first image (its second follows 128 rows later)
inline int64_t bq_chol_image_row(int64_t p, int P) { return ((p / P) & 1) * (int64_t)(P * 2 * BQ_CHOL_NB) + (p % P) * (2 * BQ_CHOL_NB); }

// emit(const bq_chol_step &) is called once per step, in issue order
template <class Emit>
inline void bq_chol_plan(int64_t np, int P, bool lookahead, int64_t super_min, Emit &&emit) {
    constexpr int64_t NB = BQ_CHOL_NB;
    auto step = [&](int op, int stream, int64_t row, int64_t img, int kdim, int64_t T, int64_t nc) {
        const bq_chol_step s = {op, stream, row, img, kdim, T, nc};
        emit(s);
    };
    auto narrow = [&](int64_t p, int s) {
        const int64_t a0 = 2 * p * NB;
        if (a0 >= np) return;
        const int64_t imgA = bq_chol_image_row(p, P), imgB = imgA + NB;
        step(BQ_CHOL_DIAG, s, a0, 0, 0, 1, 0);
        const int64_t b0 = a0 + NB;
        if (b0 >= np) return;
        step(BQ_CHOL_TRSM, s, a0, imgA, (int)NB, (np - b0) / NB, 0);
        step(BQ_CHOL_COL, s, b0, imgA, (int)NB, (np - b0) / NB, 1);
        step(BQ_CHOL_DIAG, s, b0, 0, 0, 1, 0);
        if (b0 + NB >= np) return;
        step(BQ_CHOL_TRSM, s, b0, imgB, (int)NB, (np - b0 - NB) / NB, 0);
    };
    // the two block columns pass p+1 factors  -=  the images of ALL passes of p's super-pass so far (K = 256 .. (P-1) 256)
    auto head_in = [&](int64_t p, int s) {
        const int64_t r0 = 2 * p * NB + 2 * NB;
        if (r0 >= np) return;
        const int64_t first = p / P * P;
        step(BQ_CHOL_HEAD, s, r0, bq_chol_image_row(first, P), (int)((p - first + 1) * 2 * NB), (np - r0) / NB, 2);
    };
    // the narrow chain of super-pass q: narrow, head_in, narrow, ..., narrow
    auto chain = [&](int64_t q, int s) {
        for (int j = 0; j < P; ++j) {
            narrow(q * P + j, s);
            if (j + 1 < P) head_in(q * P + j, s);
        }
    };
    // everything behind super-pass q  -=  X X^T with its 2P images in one K = P * 256 pass: first the 2P block columns the next
    // chain works on, then the rest
    auto wide_head = [&](int64_t q, int s) {
        const int64_t r0 = (q + 1) * P * 2 * NB;
        if (r0 >= np) return;
        step(BQ_CHOL_HEAD, s, r0, bq_chol_image_row(q * P, P), (int)(P * 2 * NB), (np - r0) / NB, 2 * P);
    };
    auto wide_rest = [&](int64_t q, int s) {
        const int64_t r0 = (q + 1) * P * 2 * NB + 2 * P * NB;
        if (r0 >= np) return;
        const int64_t T = (np - r0) / NB;
        step(BQ_CHOL_REST, s, r0, bq_chol_image_row(q * P, P), (int)(P * 2 * NB), T, bq_chol_nsuper(T, super_min));
    };
    const int64_t npass = (np + 2 * NB - 1) / (2 * NB), nsup = (npass + P - 1) / P;
    if (!lookahead) {
        for (int64_t q = 0; q < nsup; ++q) {
            chain(q, BQ_CHOL_ON_CTX);
            wide_head(q, BQ_CHOL_ON_CTX);
            wide_rest(q, BQ_CHOL_ON_CTX);
        }
        return;
    }
    const int sm = BQ_CHOL_ON_MAIN, ss = BQ_CHOL_ON_SIDE;
    step(BQ_CHOL_RECORD, BQ_CHOL_ON_CTX, 0, 0, 0, 0, 0);   // everything enqueued so far (H assembly) precedes the factorisation
    step(BQ_CHOL_WAIT, sm, 0, 0, 0, 0, 0);
    chain(0, sm);
    for (int64_t q = 0; q < nsup; ++q) {
        const int64_t e_head = 1 + (q % 3), e_narrow = 4 + (q % 3);
        wide_head(q, sm);
        step(BQ_CHOL_RECORD, sm, 0, 0, 0, 0, e_head);
        step(BQ_CHOL_WAIT, ss, 0, 0, 0, 0, e_head);
        chain(q + 1, ss);
        step(BQ_CHOL_RECORD, ss, 0, 0, 0, 0, e_narrow);
        wide_rest(q, sm);
        step(BQ_CHOL_WAIT, sm, 0, 0, 0, 0, e_narrow);
    }
    step(BQ_CHOL_RECORD, sm, 0, 0, 0, 0, 7);
    step(BQ_CHOL_WAIT, BQ_CHOL_ON_CTX, 0, 0, 0, 0, 7);   // the solves (on the context stream) follow the factorisation
}
