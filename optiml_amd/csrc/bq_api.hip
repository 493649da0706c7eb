// C-ABI entry points (include/bcqp.h): contexts, the device-resident quadratic, the one-shot wrappers (the solvers: bq_solver.hip;
// the probes and bq_problem_time_matvec: bq_probe.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <functional>

#include "bq_common.h"
#include "bq_c7.h"
#include "bq_h52.h"

static thread_local std::string g_last_error;

void bq_set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

extern "C" const char *bq_last_error(void) { return g_last_error.c_str(); }
extern "C" int bq_abi_version(void) { return BQ_ABI_VERSION; }

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
extern "C" int bq_device_count(int *count) {
    BQ_ARG(count != nullptr, "count is NULL");
    BQ_HIP(hipGetDeviceCount(count));
    return BQ_OK;
}

static int ctx_new(int device, bq_ctx **out) {
    BQ_ARG(out != nullptr, "out is NULL");
    int ndev = 0;
    BQ_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        bq_set_error("device %d out of range (%d visible)", device, ndev);
        return BQ_ERR_BADARG;
    }
    BQ_HIP(hipSetDevice(device));
    bq_ctx *c = new bq_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    BQ_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cu = prop.multiProcessorCount;
    // hipDeviceProp_t::name comes back empty on some gfx950 boxes (BENCH_r03: " (gfx950:sramecc+:xnack-)"): say what is known
    snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name[0] ? prop.name : "AMD Instinct MI350-series [name not reported by the driver]",
             prop.gcnArchName);
    BQ_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const char *mode = getenv("BQ_SYM_EXCHANGE");
    c->sym_allreduce = mode != nullptr && strcmp(mode, "allreduce") == 0;
    bq_ctx_register(c, true);
    *out = c;
    return BQ_OK;
}

extern "C" int bq_ctx_create(int device, bq_ctx **out) { return ctx_new(device, out); }

int bq_comm_init_rccl(bq_ctx *ctx, const void *uid128);  // bq_comm.cpp
void bq_comm_destroy(bq_ctx *ctx);
int bq_comm_size(const bq_ctx *ctx);

// the segment table (bq_seg_table) is a fixed-size struct passed to kernels by value: 8 * ceil(world / 8) segments must fit
#define BQ_ARG_WORLD(world) BQ_ARG(bq_sym_segments(world) <= BQ_SYM_SEG_MAX, "world is limited to 64 ranks (BQ_SYM_SEG_MAX canonical segments)")

extern "C" int bq_ctx_create_rccl(int device, int rank, int world, const void *uid128, bq_ctx **out) {
    BQ_ARG(world >= 1 && rank >= 0 && rank < world, "rank/world");
    BQ_ARG_WORLD(world);
    BQ_ARG(uid128 != nullptr, "uid is NULL");
    bq_ctx *c = nullptr;
    BQ_TRY(ctx_new(device, &c));
    c->rank = rank;
    c->world = world;
    int rc = bq_comm_init_rccl(c, uid128);
    if (rc != BQ_OK) {
        bq_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return BQ_OK;
}

extern "C" int bq_ctx_create_exchange(int device, int rank, int world, bq_exchange_fn fn, void *user, bq_ctx **out) {
    BQ_ARG(world >= 1 && rank >= 0 && rank < world, "rank/world");
    BQ_ARG(fn != nullptr || world == 1, "exchange callback is NULL");
    BQ_ARG_WORLD(world);
    bq_ctx *c = nullptr;
    BQ_TRY(ctx_new(device, &c));
    c->rank = rank;
    c->world = world;
    c->comm_kind = world > 1 ? BQ_COMM_CALLBACK : BQ_COMM_NONE;
    c->exch_fn = fn;
    c->exch_user = user;
    *out = c;
    return BQ_OK;
}

extern "C" int bq_ctx_create_share(int device, int rank, int world, bq_ctx **out) {
    BQ_ARG(world >= 1 && rank >= 0 && rank < world, "rank/world");
    BQ_ARG_WORLD(world);
    bq_ctx *c = nullptr;
    BQ_TRY(ctx_new(device, &c));
    c->rank = rank;
    c->world = world;
    c->comm_kind = BQ_COMM_SHARE;
    *out = c;
    return BQ_OK;
}

extern "C" int bq_ctx_destroy(bq_ctx *c) {
    if (c == nullptr) return BQ_OK;
    if (c->refs > 0) {   // problems still hold this context (and its stream): it goes with the last of them
        c->zombie = true;
        return BQ_OK;
    }
    hipSetDevice(c->device);
    bq_ctx_register(c, false);
    // the bounded wait first, the watchdog's end after it: a context closed behind a collective whose peer has gone must not sit
    // here for ever either; after an abort the stream holds nothing worth waiting for
    if (c->stream && !c->comm_aborted) (void)bq_ctx_sync(c);
    bq_watchdog_stop(c);
    bq_comm_destroy(c);
    for (auto &slot : c->prof)
        for (auto &pr : slot.pending) {
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
    if (c->prof_skip) hipFree(c->prof_skip);
    for (auto e : c->event_pool) hipEventDestroy(e);
    if (c->pinned) hipHostFree(c->pinned);
    bq_ctx_drop_cache(c);
    bq_ctx_release_held(c, nullptr);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return BQ_OK;
}

extern "C" int bq_ctx_info(const bq_ctx *c, int *device, int *rank, int *world, char *name, size_t cap) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    if (device) *device = c->device;
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    if (name && cap) snprintf(name, cap, "%s", c->name);
    return BQ_OK;
}

extern "C" int bq_ctx_comm_info(const bq_ctx *c, int *kind, int *comm_ranks, int *sym_allreduce) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    if (kind) *kind = c->comm_kind;
    if (comm_ranks) *comm_ranks = bq_comm_size(c);
    if (sym_allreduce) *sym_allreduce = c->sym_allreduce ? 1 : 0;
    return BQ_OK;
}

extern "C" int bq_ctx_set_sym_allreduce(bq_ctx *c, int on) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    c->sym_allreduce = on != 0;
    return BQ_OK;
}

extern "C" int bq_ctx_profile(bq_ctx *c, int enable) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    c->profiling = enable != 0;
    return BQ_OK;
}

// bracket == true: the pair brackets a region of the stream (e0 is recorded here, e1 by bq_prof_end).  bracket == false: the pair is
// handed to ONE kernel launch (hipExtLaunchKernelGGL(..., e0, e1, ...)), whose own dispatch carries the two timestamps — the
// kernel's duration as the tracer sees it, and no event packets on the stream; bq_prof_end is then called with recorded == true.
int bq_prof_begin(bq_ctx *c, int which, hipEvent_t *e0, hipEvent_t *e1, bool bracket) {
    *e0 = *e1 = nullptr;
    if (!c->profiling) return BQ_OK;
    hipError_t err = hipSuccess;
    for (hipEvent_t *e : {e0, e1}) {
        if (!c->event_pool.empty()) {
            *e = c->event_pool.back();
            c->event_pool.pop_back();
        } else if ((err = hipEventCreate(e)) != hipSuccess) {
            *e = nullptr;
            break;
        }
    }
    if (err == hipSuccess && bracket) err = hipEventRecord(*e0, c->stream);
    if (err != hipSuccess) {   // nothing leaks on the error path: what was taken goes back to the pool
        for (hipEvent_t *e : {e0, e1}) {
            if (*e) c->event_pool.push_back(*e);
            *e = nullptr;
        }
        bq_set_error("profiling events: %s", hipGetErrorString(err));
        return BQ_ERR_HIP;
    }
    (void)which;
    return BQ_OK;
}

void bq_prof_drop(bq_ctx *c, hipEvent_t e0, hipEvent_t e1) {
    if (e0) c->event_pool.push_back(e0);
    if (e1) c->event_pool.push_back(e1);
    c->prof_cur_idx = -1;
}

void bq_prof_skip_arg(bq_ctx *c, hipEvent_t e0, int **slot, int *seq) {
    *slot = nullptr;
    *seq = 0;
    c->prof_cur_idx = -1;
    if (e0 == nullptr) return;   // not profiling
    if (c->prof_skip == nullptr) {
        if (hipMalloc(&c->prof_skip, sizeof(int) * BQ_PROF_SKIP_CAP) != hipSuccess ||
            hipMemsetAsync(c->prof_skip, 0, sizeof(int) * BQ_PROF_SKIP_CAP, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            c->prof_skip = nullptr;
            return;
        }
    }
    if ((int64_t)c->prof[BQ_PROF_MATVEC].pending.size() >= BQ_PROF_SKIP_CAP - 1) return;   // ring full until the next read
    c->prof_seq += 1;
    c->prof_cur_idx = (int)(c->prof_seq % BQ_PROF_SKIP_CAP);
    c->prof_cur_seq = (int)(c->prof_seq & 0x7fffffff) | 1;   // never 0 (the ring starts zeroed)
    *slot = c->prof_skip + c->prof_cur_idx;
    *seq = c->prof_cur_seq;
}

int bq_prof_end(bq_ctx *c, int which, hipEvent_t e0, hipEvent_t e1, bool recorded) {
    if (e0 == nullptr) return BQ_OK;
    if (!recorded) BQ_HIP(hipEventRecord(e1, c->stream));
    bq_prof_pending pe;
    pe.first = e0;
    pe.second = e1;
    if (which == BQ_PROF_MATVEC && c->prof_cur_idx >= 0) {
        pe.skip_idx = c->prof_cur_idx;
        pe.skip_seq = c->prof_cur_seq;
    }
    c->prof_cur_idx = -1;
    c->prof[which].pending.push_back(pe);
    return BQ_OK;
}

extern "C" int bq_ctx_profile_read(bq_ctx *c, int which, double *total_ms, int64_t *launches, int reset) {
    BQ_ARG(c != nullptr && which >= 0 && which < BQ_PROF_COUNT, "ctx/which");
    BQ_SYNC(c);
    bq_prof_slot &s = c->prof[which];
    std::vector<int> ring;
    bool any_tag = false;
    for (const bq_prof_pending &pe : s.pending) any_tag = any_tag || pe.skip_idx >= 0;
    if (any_tag && c->prof_skip != nullptr) {
        ring.resize(BQ_PROF_SKIP_CAP);
        BQ_HIP(hipMemcpy(ring.data(), c->prof_skip, sizeof(int) * BQ_PROF_SKIP_CAP, hipMemcpyDeviceToHost));
    }
    for (const bq_prof_pending &pe : s.pending) {
        float ms = 0.f;
        BQ_HIP(hipEventElapsedTime(&ms, pe.first, pe.second));
        c->event_pool.push_back(pe.first);
        c->event_pool.push_back(pe.second);
        // a launch that returned at once on its `done` flag said so itself (bq_prof_skip_arg): it is no product and stays out of
        // the mean — exactly those launches, whatever their duration
        if (pe.skip_idx >= 0 && !ring.empty() && ring[(size_t)pe.skip_idx] == pe.skip_seq) {
            s.skipped += 1;
            continue;
        }
        s.total_ms += ms;
        s.launches += 1;
    }
    s.pending.clear();
    if (total_ms) *total_ms = s.total_ms;
    if (launches) *launches = s.launches;
    if (reset) {
        s.total_ms = 0.0;
        s.launches = 0;
        s.skipped = 0;
    }
    return BQ_OK;
}

static int64_t row_block_size(int64_t n, int world) {
    const int64_t per = (n + world - 1) / world;
    return bq_round_up(per > 0 ? per : 1, 128);  // tile-aligned for the Gram kernel
}

extern "C" int bq_row_block(int64_t n, int rank, int world, int64_t *begin, int64_t *end) {
    BQ_ARG(n >= 0 && world >= 1 && rank >= 0 && rank < world, "n/rank/world");
    const int64_t blk = row_block_size(n, world);
    int64_t b = (int64_t)rank * blk;
    if (b > n) b = n;
    int64_t e = b + blk;
    if (e > n) e = n;
    if (begin) *begin = b;
    if (end) *end = e;
    return BQ_OK;
}

// Balanced triangular partition of nb tile rows into S canonical segments: segment s starts at round(nb * sqrt(s / S)), so
// every segment holds about nb^2 / (2 S) tiles of the lower triangle.  Rank k of G owns the segments
// [floor(k S / G), floor((k+1) S / G)) — for G dividing S that is I_k = round(nb * sqrt(k / G)), equal tile counts per rank.
int64_t bq_sym_seg_cut(int64_t nb, int s, int S) {
    if (s <= 0) return 0;
    if (s >= S) return nb;
    int64_t v = (int64_t)std::llround((double)nb * std::sqrt((double)s / (double)S));
    return v < 0 ? 0 : (v > nb ? nb : v);
}

static void sym_tile_rows(int64_t nb, int rank, int world, int64_t *I0, int64_t *I1) {
    const int S = bq_sym_segments(world);
    *I0 = bq_sym_seg_cut(nb, bq_sym_seg_first(rank, world, S), S);
    *I1 = bq_sym_seg_cut(nb, bq_sym_seg_first(rank + 1, world, S), S);
}

void bq_sym_seg_table(const bq_problem *p, bq_seg_table *tab) {
    const int world = p->ctx->world;   // <= 64: checked where a multi-rank context is created (BQ_ARG_WORLD)
    tab->count = p->seg_count;
    tab->lo = p->seg_lo;
    tab->hi = p->seg_hi;
    for (int s = 0; s <= p->seg_count; ++s) tab->cut[s] = bq_sym_seg_cut(p->nb, s, p->seg_count);
    for (int k = 0; k < world; ++k) {
        const int lo = bq_sym_seg_first(k, world, p->seg_count), hi = bq_sym_seg_first(k + 1, world, p->seg_count);
        for (int s = lo; s < hi; ++s) tab->slot[s] = k * p->seg_cmax + (s - lo);
    }
}

extern "C" int bq_sym_row_block(int64_t n, int rank, int world, int64_t *begin, int64_t *end) {
    BQ_ARG(n >= 0 && world >= 1 && rank >= 0 && rank < world, "n/rank/world");
    const int64_t nb = (n + BQ_SYM_TILE - 1) / BQ_SYM_TILE;
    int64_t I0, I1;
    sym_tile_rows(nb, rank, world, &I0, &I1);
    if (begin) *begin = std::min(n, I0 * BQ_SYM_TILE);
    if (end) *end = std::min(n, I1 * BQ_SYM_TILE);
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------
// the quadratic
// ---------------------------------------------------------------------------------------------
static int problem_alloc_common(bq_problem *p, const double *q_host) {
    bq_ctx *c = p->ctx;
    const int64_t nblk = p->ldN / BQ_VEC_TILE;
    hipError_t e = bq_dev_zeroed(hipSuccess, p->mem, &p->q, p->ldN, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->q, q_host, sizeof(double) * p->N, hipMemcpyHostToDevice, c->stream);
    e = bq_dev_zeroed(e, p->mem, &p->w, p->ld, c->stream);
    const int64_t slen = bq_round_up(std::max(p->blk * c->world, p->nb * BQ_SYM_TILE), BQ_PAD);
    if (p->symmetric) {
        if (e == hipSuccess && !p->streamed) e = p->mem.dev(&p->slab, p->nb * p->nb * BQ_SYM_TILE);   // streamed: its own scratch
        // the gathered segment vectors of every rank (also a one-rank communicator)
        if (c->comm_kind != BQ_COMM_NONE) e = bq_dev_zeroed(e, p->mem, &p->gath, (size_t)c->world * p->seg_cmax * p->nb * BQ_SYM_TILE, c->stream);
    }
    e = bq_dev_zeroed(e, p->mem, &p->s, slen, c->stream);
    e = bq_dev_zeroed(e, p->mem, &p->va, p->ldN, c->stream);
    e = bq_dev_zeroed(e, p->mem, &p->vb, p->ldN, c->stream);
    if (e == hipSuccess) e = p->mem.dev(&p->partials, BQ_MAX_PARTIAL_Q * nblk);
    if (e == hipSuccess) e = p->mem.dev(&p->scal, 16);
    BQ_HIP_CHAIN(e, "problem setup");
    return BQ_OK;
}

static int problem_layout(bq_problem *p, int64_t n, int64_t N) {
    bq_ctx *c = p->ctx;
    p->n = n;
    p->N = N;
    p->ld = bq_round_up(n, BQ_PAD);
    p->ldN = bq_round_up(N, BQ_PAD);
    p->blk = row_block_size(n, c->world);
    int64_t rows;
    if (p->symmetric) {
        p->nb = (n + BQ_SYM_TILE - 1) / BQ_SYM_TILE;
        sym_tile_rows(p->nb, c->rank, c->world, &p->I0, &p->I1);
        p->seg_count = bq_sym_segments(c->world);
        p->seg_lo = bq_sym_seg_first(c->rank, c->world, p->seg_count);
        p->seg_hi = bq_sym_seg_first(c->rank + 1, c->world, p->seg_count);
        p->seg_cmax = (p->seg_count + c->world - 1) / c->world;
        p->r0 = std::min(n, p->I0 * BQ_SYM_TILE);
        p->r1 = std::min(n, p->I1 * BQ_SYM_TILE);
        rows = (p->I1 - p->I0) * BQ_SYM_TILE;  // whole tiles, zero rows past n
    } else {
        BQ_TRY(bq_row_block(n, c->rank, c->world, &p->r0, &p->r1));
        rows = p->r1 - p->r0;
    }
    if (p->streamed) return BQ_OK;   // no resident panel
    // compact fp64 panels (bq_c7.h, packed layout only) take 7 bytes per element
    const size_t esz = p->compact ? 7 : p->storage == BQ_F64 ? 8 : 4;
    // symmetric panels are stored packed: tile row I keeps (I+1)*256 columns
    const size_t elems = p->symmetric ? (size_t)(bq_sym_off(p->I1) - bq_sym_off(p->I0))
                                      : (size_t)(rows > 0 ? rows : 1) * (size_t)p->ld;
    p->panel_elems = (int64_t)elems;
    size_t bytes = (elems > 0 ? elems : 1) * esz;
    const size_t data_bytes = bytes;
    hipError_t e = hipSuccess;
    size_t cached = 0;
    if (void *kept = bq_ctx_cache_take(c, bytes, &cached)) {
        p->panel = kept;   // the panel a destroyed problem left behind
        p->panel_bytes = cached;
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        e = hipMalloc(&p->panel, bytes);   // bq_device_malloc: drops the cached panel and retries on failure
        p->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        p->panel_bytes = bytes;
    }
    p->panel_alloc = p->panel;
    (void)data_bytes;
    if (e != hipSuccess) {
        p->panel = nullptr;
        p->panel_alloc = nullptr;
        bq_set_error("cannot allocate the %lld x %lld panel (%.1f GB): %s", (long long)rows, (long long)p->ld,
                     bytes / 1e9, hipGetErrorString(e));
        return BQ_ERR_NOMEM;
    }
    BQ_HIP(hipMemsetAsync(p->panel, 0, bytes, c->stream));
    return BQ_OK;
}

void bq_problem_unref(bq_problem *p) {
    if (p == nullptr) return;
    if (--p->refs <= 0 && p->zombie) {
        p->refs = 0;
        p->zombie = false;
        bq_problem_destroy(p);
    }
}

extern "C" int bq_problem_destroy(bq_problem *p) {
    if (p == nullptr) return BQ_OK;
    if (p->refs > 0) {   // solvers still run on this problem: it goes with the last of them
        p->zombie = true;
        return BQ_OK;
    }
    hipSetDevice(p->ctx->device);
    (void)bq_ctx_sync(p->ctx);   // may sit behind a collective: bounded when a collective timeout is set
    if (p->panel_alloc && p->panel_bytes >= ((size_t)1 << 30)) {   // keep one large panel for the next problem (see bq_ctx)
        bq_ctx_cache_put(p->ctx, p->panel_alloc, p->panel_bytes);
        p->panel_alloc = nullptr;
    }
    p->panel = nullptr;
    bq_ctx_release_held(p->ctx, p);
    bq_image_register(p, false);   // (after this no failing allocation touches p->himg)
    if (p->himg) hipFree(p->himg);   // the panel family is not the owner's (bq_problem::mem)
    if (p->panel_alloc) hipFree(p->panel_alloc);
    bq_stream_free(p->stream_img);
    bq_ctx *c = p->ctx;
    delete p;
    if (--c->refs <= 0 && c->zombie) {
        c->refs = 0;
        c->zombie = false;
        bq_ctx_destroy(c);
    }
    return BQ_OK;
}

static int place_panel(bq_problem *p, double first_alloc_ms);

static int dense_new(bq_ctx *c, int64_t n, const double *q, int storage, bool symmetric, bool place, bq_problem **out) {
    bq_problem *p = new bq_problem();
    p->ctx = c;
    c->refs += 1;
    p->structure = BQ_PLAIN;
    p->storage = storage;
    p->symmetric = symmetric;
    int rc = problem_layout(p, n, n);
    if (rc == BQ_OK) rc = problem_alloc_common(p, q);
    if (rc == BQ_OK && place && symmetric) rc = place_panel(p, p->alloc_ms);
    if (rc != BQ_OK) {
        bq_problem_destroy(p);
        return rc;
    }
    *out = p;
    return BQ_OK;
}

// Quadratic(Q, q) (optiml/opti/_base.py:228-256).  A Q that equals its transpose exactly goes into the packed lower tile rows of
// the kernel-built panels (half the HBM, half the bytes per product: symv_tiles_kernel); any other Q keeps whole row blocks and
// NumPy's `Q @ x` (gemv_rows_kernel).  bq_dense.hip has the upload and the check.
extern "C" int bq_problem_create_dense(bq_ctx *c, int64_t n, const double *Q, const double *q, int storage,
                                       bq_problem **out) {
    BQ_ARG(c && Q && q && out, "NULL argument");
    BQ_ARG(n >= 2, "Q is too small");  // optiml/opti/_base.py:249-250
    const bool force_rows = (storage & BQ_DENSE_ROWS) != 0, trust_lower = (storage & BQ_DENSE_LOWER) != 0;
    const bool place = (storage & BQ_PLACE_PANEL) != 0;
    storage &= ~(BQ_DENSE_ROWS | BQ_DENSE_LOWER | BQ_PLACE_PANEL);
    BQ_ARG(storage == BQ_F64 || storage == BQ_F32, "storage");
    BQ_ARG(!(force_rows && trust_lower), "BQ_DENSE_ROWS and BQ_DENSE_LOWER exclude each other");
    BQ_HIP(hipSetDevice(c->device));
    bq_problem *p = nullptr;
    // every rank is handed the same Q, so the look at the host matrix sends them all the same way
    bool try_sym = !force_rows && (trust_lower || bq_dense_host_spot_symmetric(Q, n));
    if (try_sym) {
        // rank-local steps (the packed panel's allocation, the upload, the comparison), then ONE agreement on a multi-rank context:
        // "some rank failed" ends the call with an error on EVERY rank, "some rank saw a difference" sends every rank to row blocks
        int rc = dense_new(c, n, q, storage, true, place, &p);
        int is_sym = 1;
        if (rc == BQ_OK) rc = bq_dense_upload_sym(p, Q, !trust_lower, &is_sym);
        if (rc == BQ_OK) rc = bq_ctx_sync(c);
        bool any_failed = rc != BQ_OK, any_asym = !is_sym;
        if (!trust_lower || c->world > 1) {
            int arc = bq_dense_agree(c, rc != BQ_OK, &any_failed);
            if (arc == BQ_OK && !any_failed && !trust_lower) arc = bq_dense_agree(c, !is_sym, &any_asym);
            if (rc == BQ_OK && arc != BQ_OK) rc = arc;
        }
        if (rc != BQ_OK || any_failed) {
            if (p) bq_problem_destroy(p);
            if (rc == BQ_OK) {
                bq_set_error("the dense Hessian could not be set up on another rank");
                rc = BQ_ERR_HIP;
            }
            return rc;
        }
        if (!any_asym) {
            *out = p;
            return BQ_OK;
        }
        bq_problem_destroy(p);   // not symmetric after all: row blocks
        bq_ctx_drop_cache(c);    // (the packed panel is half the size the row blocks need: nothing to keep it for)
        p = nullptr;
    }
    BQ_TRY(dense_new(c, n, q, storage, false, false, &p));
    int rc = bq_dense_upload_rows(p, Q);
    if (rc == BQ_OK) rc = bq_ctx_sync(c);
    if (rc != BQ_OK) {
        bq_problem_destroy(p);
        return rc;
    }
    *out = p;
    return BQ_OK;
}

// BQ_PLACE_PANEL (bcqp.h): time the product kernel on the freshly allocated, zeroed panel; while it streams below the "good" rate,
// the device can hold one more panel and the TIME BUDGET allows it, allocate another candidate and time it; keep the fastest,
// HOLD the rest until the first solver on the problem is destroyed (or the problem, or an allocation fails: released earlier, the allocator would hand the same memory
// back as the next candidate; released at the end — rounds 4-5 — the release itself slowed the solve that followed: bq_ctx::held).
//
// What a slow placement is (round 4, profiles/r04/placement_*.txt): a property of the physical region the driver handed out, stable
// for the life of the allocation (6.04 ... 6.50 ms in clusters) — NOT of the base address (the same allocation at 8 - 20 byte
// offsets up to 1 GiB: flat to 0.5 %), not of the page-table contiguity the API can ask for (hipDeviceMallocContiguous: same
// spread), not of the translation caches (UTCL1 misses equal); on a slow panel the fabric sees FEWER requests in flight and LOWER
// latency (TCC_EA0_RDREQ_LEVEL -10 %, DRAM credit stalls -30 %) while the vector L1 waits longer (TCP_PENDING_STALL +8 %).  Nothing
// on the allocation side changes it, so the remedy stays a choice among allocations — bounded in time so that it can be ON by
// default (SVC / SVR.fit and bench.py alike): BQ_PLACE_BUDGET_MS (200) covers the timing of the first panel (5 products) and
// as many further candidates as fit, each priced at what the FIRST allocation of this size cost (freshly released device memory
// is cleared by the driver before it is handed out: seconds, not milliseconds — then no candidate fits the budget).
// Per rank and before the first collective of a multi-rank job: the other ranks wait at most the budget.
// The choice itself, for any allocation a one-column product streams (the panel; the Hessian image): `launch(alloc)` enqueues one product
// on `alloc`, `*alloc` comes in as the first allocation (already zeroed on the stream) and goes out as the fastest; the others are held
// for `owner`.  tried / ms: the placements timed and the launch time on each.
namespace {
struct place_timer {   // events and the profiling switch go back on every exit path
    bq_ctx *c;
    bool prof;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit place_timer(bq_ctx *ctx) : c(ctx), prof(ctx->profiling) { c->profiling = false; }
    ~place_timer() {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        c->profiling = prof;
    }
    int init() {
        BQ_HIP(hipEventCreate(&e0));
        BQ_HIP(hipEventCreate(&e1));
        return BQ_OK;
    }
    // five products: one to warm, the mean of four
    int time_on(const std::function<int(void *)> &launch, void *alloc, double *ms_out) {
        int rc = launch(alloc);   // warm
        hipEventRecord(e0, c->stream);
        for (int i = 0; rc == BQ_OK && i < 4; ++i) rc = launch(alloc);
        hipEventRecord(e1, c->stream);
        hipError_t he = hipEventSynchronize(e1);
        float ms = 0.f;
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
        if (rc == BQ_OK && he != hipSuccess) {
            bq_set_error("timing a panel placement failed: %s", hipGetErrorString(he));
            rc = BQ_ERR_HIP;
        }
        *ms_out = (double)ms / 4.0;
        return rc;
    }
};
}  // namespace

static int place_candidates(bq_ctx *c, const void *owner, size_t bytes, double first_alloc_ms, const std::function<int(void *)> &launch,
                            void **alloc, int *tried, double *ms, int max_tried) {
    const int want = std::min(3, max_tried);   // allocations tried at most (a 4th never won in round 4's sweeps: profiles/r04/placement_*.txt)
    const double good_gbs = bq_hook_value("panel_good_gbs", 6500.0);
    const char *e = getenv("BQ_PLACE_BUDGET_MS");
    const double budget_min = c->place_min_ms >= 0.0 ? c->place_min_ms : (e ? atof(e) : 200.0);
    double budget_ms = budget_min;   // grows with the work the caller expects once the product's time is known (below)
    const auto t_start = std::chrono::steady_clock::now();
    auto elapsed_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    place_timer timer(c);
    BQ_TRY(timer.init());
    std::vector<void *> losers;
    double best = 0.0;
    int rc = timer.time_on(launch, *alloc, &best);
    *tried = 1;
    ms[0] = best;
    // a panel that came from the context's cache (a destroyed problem of the same size left it: fit loops) was chosen when IT was
    // allocated, and a fresh allocation right after that release is the slow kind: it is kept as it is
    if (first_alloc_ms <= 0.0) return rc;
    // bq_ctx_set_placement_budget: a slow placement costs ~5 % of every product, so up to 2 % of the products the caller expects to
    // run may be spent on finding a better one (within [min, max]): SVC.fit passes its max_iter, a steady-state measurement "many"
    if (c->place_products > 0.0 && c->place_max_ms > budget_min)
        budget_ms = std::min(c->place_max_ms, std::max(budget_min, 0.02 * c->place_products * best));
    // what one more candidate costs: an allocation like the first one + clearing it + five products on it
    const double cand_ms = first_alloc_ms + (double)bytes / 4.0e9 + 6.0 * best;
    while (rc == BQ_OK && *tried < want && (double)bytes / (best * 1e-3) / 1e9 < good_gbs && elapsed_ms() + cand_ms <= budget_ms) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + bytes / 16) break;
        // the losers are held while the problem lives (bq_ctx::held): a second copy only if a tenth of the device stays free beside
        // the two (config 5's 125 GB panel on 288 GB: yes, once; a failing allocation later gives the held one back: bq_alloc.cpp)
        if (2 * bytes + total_b / 10 > total_b || free_b < bytes + total_b / 10) break;
        void *cand = nullptr;
        if (hipMalloc(&cand, bytes) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        hipError_t he = hipMemsetAsync(cand, 0, bytes, c->stream);
        double t = 0.0;
        if (he == hipSuccess) rc = timer.time_on(launch, cand, &t);
        if (he != hipSuccess || rc != BQ_OK) {
            hipFree(cand);
            if (he != hipSuccess) (void)hipGetLastError();
            break;
        }
        ms[(*tried)++] = t;
        if (t < best) {
            losers.push_back(*alloc);
            *alloc = cand;
            best = t;
        } else {
            losers.push_back(cand);
        }
    }
    // not released here: a large hipFree is followed by a transient in which the whole process streams slower (bq_ctx::held)
    for (void *l : losers) bq_ctx_hold(c, l, bytes, owner);
    return rc;
}

static int place_panel(bq_problem *p, double first_alloc_ms) {
    bq_ctx *c = p->ctx;
    if (!p->symmetric || p->streamed || p->panel == nullptr || p->panel_bytes < ((size_t)1 << 30) || p->I1 <= p->I0) return BQ_OK;
    bq_seg_table tab;
    bq_sym_seg_table(p, &tab);
    auto launch = [&](void *panel) {
        return bq_launch_symv(c, bq_problem_panel(p, panel), p->add_one, p->nb, tab, p->w, p->slab, p->s, nullptr);
    };
    void *chosen = p->panel;
    const int rc = place_candidates(c, p, p->panel_bytes, first_alloc_ms, launch, &chosen, &p->place_tried, p->place_ms, 32);
    p->panel = chosen;
    p->panel_alloc = chosen;
    return rc;
}

// The Hessian image (bq_h52.h; the rules: bq_problem_hessian_image in bcqp.h).  "Not built" is a state, never an error: the product
// reads the panel then, with the same bits.  The image is placed like the panel — the streaming time belongs to the physical region
// that is streamed, and that is now the image: a zero-filled image decodes to 1.0 everywhere, so it is timed empty as the panel is.
int bq_hessian_image_ensure(bq_problem *p) {
    bq_ctx *c = p->ctx;
    if (p->himg_state != BQ_HIMG_NONE) return BQ_OK;   // decided once per problem
    auto decided = [&](int state) {
        p->himg_state = state;
        return BQ_OK;
    };
    if (!p->add_one || !p->compact || !p->symmetric || p->streamed || p->panel == nullptr || p->I1 <= p->I0) return decided(BQ_HIMG_NOT_ELIGIBLE);
    if (!bq_hook_on("hessian_image")) return decided(BQ_HIMG_SWITCHED_OFF);
    const size_t bytes = (size_t)bq_h52_bytes(p->panel_elems);
    size_t free_b = 0, total_b = 0;
    BQ_HIP(hipMemGetInfo(&free_b, &total_b));
    if (free_b < bytes + total_b / 10) return decided(BQ_HIMG_NO_ROOM);   // place_panel's rule for a second panel
    if (!(p->expected_products > 0.0)) return decided(BQ_HIMG_NO_REPAY);   // unknown counts as 0
    bq_seg_table tab;
    bq_sym_seg_table(p, &tab);
    double t_prod = 0.0;   // the product as place_panel measured it on the panel kept; else five products now
    for (int i = 0; i < p->place_tried; ++i) t_prod = (i == 0 || p->place_ms[i] < t_prod) ? p->place_ms[i] : t_prod;
    if (p->place_tried == 0) {
        place_timer timer(c);
        BQ_TRY(timer.init());
        BQ_TRY(timer.time_on([&](void *panel) {
            return bq_launch_symv(c, bq_problem_panel(p, panel), true, p->nb, tab, p->w, p->slab, p->s, nullptr);
        }, p->panel, &t_prod));
    }
    const size_t panel_data = (size_t)p->panel_elems * 7;
    const double good_gbs = bq_hook_value("panel_good_gbs", 6500.0);
    const double cost_ms = p->alloc_ms * (double)bytes / (double)std::max<size_t>(p->panel_bytes, 1) + (double)(panel_data + bytes) / (good_gbs * 1e6);
    if (cost_ms > p->expected_products * (1.0 - 6.5 / 7.0) * t_prod) return decided(BQ_HIMG_NO_REPAY);
    // hook alloc_fail_above: a request above the threshold is refused here (the allocator's own simulation only fails a request that
    // giving something back could serve)
    const long long fail_above = (long long)bq_hook_value("alloc_fail_above", -1.0);
    void *img = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if ((fail_above >= 0 && (long long)bytes > fail_above) || hipMalloc(&img, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return decided(BQ_HIMG_ALLOC_FAILED);
    }
    const double alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bq_scratch mem;   // the conversion's flag; the image itself is the allocator's to take back (bq_problem::mem)
    int *bad_dev = nullptr;
    int rc = BQ_OK;
    auto give_up = [&](int err) {
        if (img) hipFree(img);
        return err;
    };
    if (hipMemsetAsync(img, 0, bytes, c->stream) != hipSuccess || mem.dev(&bad_dev, 1) != hipSuccess) {
        bq_set_error("Hessian image setup failed: %s", hipGetErrorString(hipGetLastError()));
        return give_up(BQ_ERR_HIP);
    }
    {   // timed on every image; further candidates as for the panel: from 1 GiB on
        auto launch = [&](void *image) {
            return bq_launch_symv(c, bq_problem_image(p, image), false, p->nb, tab, p->w, p->slab, p->s, nullptr);
        };
        rc = place_candidates(c, p, bytes, alloc_ms, launch, &img, &p->himg_tried, p->himg_ms, bytes >= ((size_t)1 << 30) ? 3 : 1);
        if (rc != BQ_OK) return give_up(rc);
    }
    // The bytes are not the whole story: a grid of one round of workgroups or less lasts as long as one strip takes, and there the
    // image's product was measured SLOWER than the panel's (C2, 435 strips: profiles/hessian_image/c2_ab_duplicate_load.json: with the 16-byte load issued twice).  So the panel's
    // product is timed again NOW, with the same five launches as the image's a moment ago (the time place_panel took at problem
    // creation is another moment of the device), and the image stays only if the MEASURED saving per product is positive and repays
    // what the allocation did cost and the conversion will (hook hessian_image_gain=G: the image's product must be G times faster;
    // 0 keeps it regardless, for the tests' small sizes).
    double t_img = p->himg_ms[0], t_now = 0.0;
    for (int i = 1; i < p->himg_tried; ++i) t_img = std::min(t_img, p->himg_ms[i]);
    {
        place_timer timer(c);
        rc = timer.init();
        if (rc == BQ_OK)
            rc = timer.time_on([&](void *panel) {
                return bq_launch_symv(c, bq_problem_panel(p, panel), true, p->nb, tab, p->w, p->slab, p->s, nullptr);
            }, p->panel, &t_now);
        if (rc != BQ_OK) return give_up(rc);
    }
    const double gain = bq_hook_value("hessian_image_gain", 1.0);
    const double spent_ms = alloc_ms + (double)(panel_data + bytes) / (good_gbs * 1e6);
    if (gain > 0.0 && (t_img * gain >= t_now || p->expected_products * (t_now - t_img) < spent_ms)) {
        // held like a candidate that lost, until the first solver of the problem goes (bq_solver_destroy): a large release slows
        // the solve that follows (bq_ctx::held)
        bq_ctx_hold(c, img, bytes, p);
        img = nullptr;
        give_up(BQ_OK);
        return decided(BQ_HIMG_NOT_FASTER);
    }
    const auto t1 = std::chrono::steady_clock::now();
    rc = bq_launch_h52_convert(c, p, img, bad_dev, bq_hook_value("hessian_image_bad", 0.0) != 0.0);
    int bad = 0;
    if (rc == BQ_OK && hipMemcpyAsync(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        bq_set_error("Hessian image conversion failed: %s", hipGetErrorString(hipGetLastError()));
        rc = BQ_ERR_HIP;
    }
    if (rc == BQ_OK) rc = bq_ctx_sync(c);
    if (rc != BQ_OK) return give_up(rc);
    p->himg_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (bad) {   // never reached from a compact panel (K in {0} u [2^-15, 1]): the safety net, as for the compact panel itself
        give_up(BQ_OK);
        return decided(BQ_HIMG_OUT_OF_DOMAIN);
    }
    p->himg = img;
    p->himg_bytes = bytes;
    bq_image_register(p, true);
    return decided(BQ_HIMG_BUILT);
}

extern "C" int bq_problem_hessian_image(const bq_problem *p, int *state, int64_t *bytes, double *build_ms, int *tried, double *ms, int cap) {
    BQ_ARG(p != nullptr && state != nullptr, "NULL argument");
    *state = p->himg_state;
    if (bytes) *bytes = p->himg ? (int64_t)p->himg_bytes : 0;
    if (build_ms) *build_ms = p->himg_build_ms;
    if (tried) *tried = p->himg_tried;
    for (int i = 0; ms != nullptr && i < cap && i < p->himg_tried; ++i) ms[i] = p->himg_ms[i];
    return BQ_OK;
}

extern "C" int bq_ctx_set_placement_budget(bq_ctx *c, double min_ms, double max_ms, double expected_products) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    BQ_ARG(expected_products >= 0.0, "expected_products must be >= 0");
    c->place_min_ms = min_ms;      // < 0: BQ_PLACE_BUDGET_MS / 200 ms
    c->place_max_ms = max_ms;
    c->place_products = expected_products;
    return BQ_OK;
}

extern "C" int bq_problem_placement(const bq_problem *p, int *tried, double *ms, int cap) {
    BQ_ARG(p != nullptr && tried != nullptr, "NULL argument");
    *tried = p->place_tried;
    for (int i = 0; ms != nullptr && i < cap && i < p->place_tried; ++i) ms[i] = p->place_ms[i];
    return BQ_OK;
}

extern "C" int bq_problem_create_kernel(bq_ctx *c, int structure, int64_t n, int64_t d, const double *X,
                                        const double *y, int kernel, double gamma, double coef0, int degree,
                                        double diag_add, const double *q, int storage, bq_problem **out) {
    BQ_ARG(c && X && q && out, "NULL argument");
    const bool no_rank_one = (structure & BQ_NO_RANK_ONE) != 0, full_panel = (structure & BQ_FULL_PANEL) != 0;
    const bool place = (structure & BQ_PLACE_PANEL) != 0, plain_panel = (structure & BQ_PLAIN_PANEL) != 0;
    structure &= ~(BQ_NO_RANK_ONE | BQ_FULL_PANEL | BQ_PLACE_PANEL | BQ_PLAIN_PANEL);
    BQ_ARG(structure == BQ_PLAIN || structure == BQ_SVC || structure == BQ_SVR, "structure");
    BQ_ARG(structure != BQ_SVC || y != nullptr, "labels required for BQ_SVC");
    BQ_ARG(kernel >= BQ_KERNEL_LINEAR && kernel <= BQ_KERNEL_LAPLACIAN, "kernel");
    BQ_ARG(n >= 2 && d >= 1, "n/d");
    BQ_ARG(storage == BQ_F64 || storage == BQ_F32 || storage == BQ_STREAM, "storage");
    BQ_ARG(storage != BQ_STREAM || kernel != BQ_KERNEL_LAPLACIAN, "the streamed mode is built for the inner-product kernels");
    BQ_ARG(kernel != BQ_KERNEL_POLY || degree > 0, "degree must be > 0");
    BQ_HIP(hipSetDevice(c->device));
    bq_problem *p = new bq_problem();
    p->ctx = c;
    c->refs += 1;
    p->structure = structure;
    p->storage = storage;
    p->kernel = kernel;
    p->add_one = structure != BQ_PLAIN && !no_rank_one;
    p->gamma = gamma;
    p->coef0 = coef0;
    p->degree = degree;
    p->diag_add = diag_add;
    p->d = d;
    p->streamed = storage == BQ_STREAM;
    p->expected_products = c->place_products;
    // Gram panels are symmetric: store and stream only the tiles on/below the diagonal, unless the caller asked for whole rows
    // (BQ_FULL_PANEL).  Streamed problems take the same segment partition of the tile rows and form each lower-triangle tile once.
    p->symmetric = p->streamed || !full_panel;
    auto fail = [&](hipError_t e) {
        bq_set_error("kernel problem setup failed: %s", hipGetErrorString(e));
        bq_problem_destroy(p);
        return BQ_ERR_HIP;
    };
    hipError_t e;
    if ((e = p->mem.dev(&p->X, n * d)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(p->X, X, sizeof(double) * n * d, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e);
    int rc = BQ_OK;
    // An RBF panel in fp64 whose every element lies in [2^-14, 1] (bq_c7_eligible: a function of X and gamma only, so every rank
    // decides alike) is stored in the compact 7-byte layout; BQ_PLAIN_PANEL (SMO) and hook compact_panel=0 keep the plain one
    if (kernel == BQ_KERNEL_RBF && storage == BQ_F64 && p->symmetric && !p->streamed && !plain_panel && bq_compact_allowed()) {
        double m2 = 0.0;
        rc = bq_max_sq_norm(c, p->X, n, d, &m2);
        p->compact = rc == BQ_OK && bq_c7_eligible(gamma, m2);
    }
    if (rc == BQ_OK) rc = problem_layout(p, n, structure == BQ_SVR ? 2 * n : n);
    if (rc == BQ_OK) rc = problem_alloc_common(p, q);
    if (rc == BQ_OK && place) rc = place_panel(p, p->alloc_ms);
    if (rc != BQ_OK) {
        bq_problem_destroy(p);
        return rc;
    }
    if (structure == BQ_SVC) {
        if ((e = bq_dev_zeroed(hipSuccess, p->mem, &p->sgn, p->ld, c->stream)) != hipSuccess) return fail(e);
        if ((e = hipMemcpyAsync(p->sgn, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e);
    }
    int bad = 0;
    if (p->streamed)
        rc = bq_stream_prepare(c, p->X, n, d, p->I0 * BQ_SYM_TILE, p->I1 * BQ_SYM_TILE, &p->stream_img);
    else
        rc = bq_launch_gram(c, p->X, n, d, p->r0, p->r1, kernel, gamma, coef0, degree, p->panel, p->compact ? BQ_F64C : storage, p->ld,
                            p->symmetric, p->panel_elems, &bad);
    if (rc == BQ_OK && p->compact) {
        // the safety net of the compact layout: an element the build could not store (the eligibility bound makes this
        // unreachable) on ANY rank sends every rank back to the plain layout — a wrong panel is never streamed
        bool any = bad != 0;
        rc = bq_dense_agree(c, bad != 0, &any);
        if (rc == BQ_OK && any) {
            hipFree(p->panel_alloc);
            p->panel = p->panel_alloc = nullptr;
            p->compact = false;
            rc = problem_layout(p, n, structure == BQ_SVR ? 2 * n : n);
            if (rc == BQ_OK)
                rc = bq_launch_gram(c, p->X, n, d, p->r0, p->r1, kernel, gamma, coef0, degree, p->panel, storage, p->ld, p->symmetric);
        }
    }
    if (rc != BQ_OK) {
        bq_problem_destroy(p);
        return rc;
    }
    if (const int src = bq_ctx_sync(c)) {   // (bounded on a multi-rank context)
        bq_problem_destroy(p);
        return src;
    }
    *out = p;
    return BQ_OK;
}

extern "C" int bq_problem_dims(const bq_problem *p, int64_t *n_dual, int64_t *n_rows, int64_t *rb, int64_t *re) {
    BQ_ARG(p != nullptr, "problem is NULL");
    if (n_dual) *n_dual = p->N;
    if (n_rows) *n_rows = p->n;
    if (rb) *rb = p->r0;
    if (re) *re = p->r1;
    return BQ_OK;
}

extern "C" int bq_problem_layout(const bq_problem *p, int *packed, int *streamed, int64_t *panel_bytes) {
    BQ_ARG(p != nullptr, "problem is NULL");
    if (packed) *packed = p->symmetric ? 1 : 0;
    if (streamed) *streamed = p->streamed ? 1 : 0;
    if (panel_bytes) *panel_bytes = (int64_t)p->panel_bytes;
    return BQ_OK;
}

static int upload_padded(bq_problem *p, const double *host, double *dev, int64_t len, int64_t padded) {
    BQ_HIP(hipMemsetAsync(dev, 0, sizeof(double) * padded, p->ctx->stream));
    BQ_HIP(hipMemcpyAsync(dev, host, sizeof(double) * len, hipMemcpyHostToDevice, p->ctx->stream));
    return BQ_OK;
}

extern "C" int bq_problem_matvec(bq_problem *p, const double *v, double *out) {
    BQ_ARG(p && v && out, "NULL argument");
    BQ_HIP(hipSetDevice(p->ctx->device));
    BQ_TRY(upload_padded(p, v, p->va, p->N, p->ldN));
    BQ_TRY(bq_problem_apply(p, p->va, p->vb, nullptr));
    BQ_HIP(hipMemcpyAsync(out, p->vb, sizeof(double) * p->N, hipMemcpyDeviceToHost, p->ctx->stream));
    BQ_SYNC(p->ctx);
    return BQ_OK;
}

extern "C" int bq_problem_eval(bq_problem *p, const double *x, double *f, double *g) {
    BQ_ARG(p && x && f, "NULL argument");
    BQ_HIP(hipSetDevice(p->ctx->device));
    BQ_TRY(upload_padded(p, x, p->va, p->N, p->ldN));
    BQ_TRY(bq_problem_apply(p, p->va, p->vb, nullptr));
    BQ_TRY(bq_vec_eval_f(p, p->va, p->vb, g ? p->vb : nullptr, p->scal));
    BQ_HIP(hipMemcpyAsync(f, p->scal, sizeof(double), hipMemcpyDeviceToHost, p->ctx->stream));
    if (g) BQ_HIP(hipMemcpyAsync(g, p->vb, sizeof(double) * p->N, hipMemcpyDeviceToHost, p->ctx->stream));
    BQ_SYNC(p->ctx);
    return BQ_OK;
}

extern "C" int bq_problem_gram_matvec(bq_problem *p, const double *w, double *out) {
    BQ_ARG(p && w && out, "NULL argument");
    BQ_ARG(p->kernel >= 0, "not a kernel-structured problem");
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    BQ_HIP(hipMemsetAsync(p->w, 0, sizeof(double) * p->ld, c->stream));
    BQ_HIP(hipMemcpyAsync(p->w, w, sizeof(double) * p->n, hipMemcpyHostToDevice, c->stream));
    BQ_TRY(bq_panel_product(p, false, p->w, nullptr));
    BQ_HIP(hipMemcpyAsync(out, p->s, sizeof(double) * p->n, hipMemcpyDeviceToHost, c->stream));
    BQ_SYNC(c);
    return BQ_OK;
}

// test-only (hook product_rows=1): the output vector of the last panel product as the device holds it, pad rows included
extern "C" int bq_problem_last_product(bq_problem *p, double *out, int64_t cap, int64_t *len) {
    BQ_ARG(p && len, "NULL argument");
    BQ_ARG(bq_hook_value("product_rows", 0.0) != 0.0, "bq_problem_last_product is a test entry: BQ_TEST_HOOKS product_rows=1");
    const int64_t rows = p->symmetric ? p->nb * BQ_SYM_TILE : p->n;
    *len = rows;
    if (out == nullptr) return BQ_OK;
    BQ_ARG(cap >= rows, "out is too short");
    BQ_HIP(hipSetDevice(p->ctx->device));
    BQ_HIP(hipMemcpyAsync(out, p->s, sizeof(double) * rows, hipMemcpyDeviceToHost, p->ctx->stream));
    BQ_SYNC(p->ctx);
    return BQ_OK;
}

extern "C" int bq_problem_panel_rows(bq_problem *p, int64_t row0, int64_t nrows, double *out) {
    BQ_ARG(p && out, "NULL argument");
    BQ_ARG(row0 >= p->r0 && row0 + nrows <= p->r1 && nrows >= 0, "rows outside this rank's block");
    BQ_ARG(!p->streamed, "a streamed problem keeps no panel");
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    if (nrows == 0) return BQ_OK;
    if (p->symmetric) {
        // packed layout: row i holds its (I+1)*256 leading columns, strip by strip (bq_sym_addr); the rest of the output row
        // (strictly-upper tiles) is 0.  The requested rows are taken tile row by tile row: within one, a strip's stretch of these rows
        // is ONE 2-D copy per plane (source pitch: the strip's; destination: a staging block of whole rows), decoded / widened here.
        const int64_t n = p->n;
        const size_t esz = p->compact ? 4 : p->storage == BQ_F64 ? 8 : 4;   // compact: the lo plane; mid and top beside it
        const int64_t cap = std::min<int64_t>(nrows, BQ_SYM_TILE);
        std::vector<unsigned char> lo((size_t)cap * n * esz);
        std::vector<uint16_t> mid(p->compact ? (size_t)cap * n : 0);
        std::vector<uint8_t> top(p->compact ? (size_t)cap * n : 0);
        const bq_c7p pv = p->compact ? bq_c7_view(p->panel, p->panel_elems) : bq_c7p{nullptr, nullptr, nullptr};
        for (int64_t r = 0; r < nrows;) {
            const int64_t i0 = row0 + r, I = i0 / BQ_SYM_TILE;
            const int64_t rb = std::min(nrows - r, (I + 1) * BQ_SYM_TILE - i0);   // rows of this tile row
            const int64_t len = std::min(n, bq_sym_cols(I));
            for (int64_t j0 = 0; j0 < len; j0 += BQ_SYM_STRIP_COLS) {
                const int64_t a = bq_sym_addr(i0, j0, p->I0), m = std::min(len - j0, BQ_SYM_STRIP_COLS);
                const int64_t w = bq_sym_strip_w(I, j0 / BQ_SYM_STRIP_COLS);
                const unsigned char *src = p->compact ? (const unsigned char *)(pv.lo + a) : (const unsigned char *)p->panel + (size_t)a * esz;
                BQ_HIP(hipMemcpy2DAsync(lo.data() + (size_t)j0 * esz, (size_t)n * esz, src, (size_t)w * esz, (size_t)m * esz, (size_t)rb,
                                        hipMemcpyDeviceToHost, c->stream));
                if (p->compact) {
                    BQ_HIP(hipMemcpy2DAsync(mid.data() + j0, (size_t)n * 2, pv.mid + a, (size_t)w * 2, (size_t)m * 2, (size_t)rb,
                                            hipMemcpyDeviceToHost, c->stream));
                    BQ_HIP(hipMemcpy2DAsync(top.data() + j0, (size_t)n, pv.top + a, (size_t)w, (size_t)m, (size_t)rb,
                                            hipMemcpyDeviceToHost, c->stream));
                }
            }
            BQ_SYNC(c);
            for (int64_t k = 0; k < rb; ++k) {
                double *o = out + (r + k) * n;
                if (p->compact) {
                    const uint32_t *l = (const uint32_t *)lo.data() + k * n;
                    for (int64_t j = 0; j < len; ++j) {
                        const uint64_t b = bq_c7_bits(l[j], mid[(size_t)(k * n + j)], top[(size_t)(k * n + j)]);
                        std::memcpy(&o[j], &b, sizeof(double));
                    }
                } else if (p->storage == BQ_F64) {
                    std::memcpy(o, (const double *)lo.data() + k * n, (size_t)len * 8);
                } else {
                    const float *f = (const float *)lo.data() + k * n;
                    for (int64_t j = 0; j < len; ++j) o[j] = (double)f[j];
                }
                for (int64_t j = len; j < n; ++j) o[j] = 0.0;
            }
            r += rb;
        }
        return BQ_OK;
    }
    const int64_t lr = row0 - p->r0;
    if (p->storage == BQ_F64) {
        BQ_HIP(hipMemcpy2DAsync(out, p->n * 8, (const double *)p->panel + lr * p->ld, p->ld * 8, p->n * 8, nrows,
                                hipMemcpyDeviceToHost, c->stream));
        BQ_SYNC(c);
    } else {
        std::vector<float> tmp((size_t)nrows * p->n);
        BQ_HIP(hipMemcpy2DAsync(tmp.data(), p->n * 4, (const float *)p->panel + lr * p->ld, p->ld * 4, p->n * 4, nrows,
                                hipMemcpyDeviceToHost, c->stream));
        BQ_SYNC(c);
        for (size_t i = 0; i < tmp.size(); ++i) out[i] = (double)tmp[i];
    }
    return BQ_OK;
}

extern "C" int bq_decision_function(bq_ctx *c, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                                    const double *SV, const double *coef, double intercept, int64_t t,
                                    const double *Xt, double *out) {
    BQ_ARG(c && SV && coef && Xt && out, "NULL argument");
    BQ_ARG(m >= 1 && d >= 1 && t >= 1, "m/d/t");
    BQ_HIP(hipSetDevice(c->device));
    return bq_launch_decision(c, kernel, gamma, coef0, degree, m, d, SV, coef, intercept, t, Xt, out);
}

extern "C" int bq_decision_function_multi(bq_ctx *c, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                                          const double *SV, int k, const double *W, const double *b, int64_t t,
                                          const double *Xt, double *out) {
    BQ_ARG(c && SV && W && Xt && out, "NULL argument");
    BQ_ARG(m >= 1 && d >= 1 && t >= 1 && k >= 1, "m/d/t/k");
    BQ_ARG(kernel != BQ_KERNEL_LAPLACIAN, "the Laplacian kernel has no GEMM form: use bq_decision_function per column");
    BQ_ARG(kernel == BQ_KERNEL_LINEAR || kernel == BQ_KERNEL_POLY || kernel == BQ_KERNEL_RBF || kernel == BQ_KERNEL_SIGMOID,
           "unknown kernel");
    BQ_HIP(hipSetDevice(c->device));
    return bq_launch_decision_multi(c, kernel, gamma, coef0, degree, m, d, SV, k, W, b, t, Xt, out);
}

extern "C" int bq_gram_matrix(bq_ctx *c, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                              const double *A, int64_t t, const double *B, double *out) {
    BQ_ARG(c && A && out, "NULL argument");
    BQ_ARG(m >= 1 && d >= 1 && (B == nullptr || t >= 1), "m/d/t");
    BQ_HIP(hipSetDevice(c->device));
    return bq_launch_gram_matrix(c, kernel, gamma, coef0, degree, m, d, A, t, B, out);
}

int bq_chol_solve_dense_impl(bq_ctx *ctx, int64_t n, const double *A, const double *b, double *x, double *factor_ms);

extern "C" int bq_cholesky_solve(bq_ctx *c, int64_t n, const double *A, const double *b, double *x, double *factor_ms) {
    BQ_ARG(c && A && b && x, "NULL argument");
    BQ_ARG(n >= 1, "n");
    BQ_HIP(hipSetDevice(c->device));
    return bq_chol_solve_dense_impl(c, n, A, b, x, factor_ms);
}

int bq_chol_probe_impl(bq_ctx *ctx, int64_t n, const double *A, int nrhs, const double *B, const int64_t *first_nonzero, int sweeps,
                       double *X, double *L, int *info);

extern "C" int bq_cholesky_probe(bq_ctx *c, int64_t n, const double *A, int nrhs, const double *B, const int64_t *first_nonzero,
                                 int sweeps, double *X, double *L, int *info) {
    BQ_ARG(c && A && info && nrhs >= 0 && (nrhs == 0 || (B && X)), "NULL argument");
    BQ_ARG(n >= 1, "n");
    for (int j = 0; j < nrhs; ++j) {
        const int64_t f = first_nonzero ? first_nonzero[j] : 0;
        BQ_ARG(f >= 0 && f < n, "first_nonzero outside [0, n)");
        for (int64_t i = 0; i < f; ++i) BQ_ARG(B[(int64_t)j * n + i] == 0.0, "a right-hand side has a non-zero before its first_nonzero");
    }
    BQ_HIP(hipSetDevice(c->device));
    return bq_chol_probe_impl(c, n, A, nrhs, B, first_nonzero, sweeps, X, L, info);
}

extern "C" int bq_ctx_mem_info(bq_ctx *c, int64_t *free_bytes, int64_t *total_bytes) {
    BQ_ARG(c && free_bytes && total_bytes, "NULL argument");
    BQ_HIP(hipSetDevice(c->device));
    size_t f = 0, t = 0;
    BQ_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f;
    *total_bytes = (int64_t)t;
    return BQ_OK;
}
