// bq_score_pass (optiml_amd/csrc/bq_score_pass.h), what a held-out scoring entry point repeats around its launches, against counting
// stubs of the allocator and of the copy and set calls: no HIP runtime is linked, the "device" is the heap, and the stubs really
// copy, so AddressSanitizer checks every byte count against the buffers' sizes.  A pass of m = 0..8 mixed requests (copied input,
// set input, plain buffer, output, device-only output, output in a buffer of the solver's, the column count) runs with request f
// refused (out of memory, and another error), with copy f refused (in the set-up, and in finish()), with a pending launch error
// and with a launcher's own code.  Checked: what follows a failure reaches neither the allocator nor a copy; the code is
// BQ_ERR_NOMEM only for an out-of-memory failure before ready() and BQ_ERR_HIP otherwise, under the message of its stage; finish()
// copies every ledger entry exactly once, in order, with its byte count, and nothing after a failure; a null-host output is never
// copied; every buffer is freed once, when the pass goes.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bcqp.h"

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct stream_stub *hipStream_t;

struct copy_rec {
    void *dst;
    const void *src;   // null: a set
    size_t bytes;
    int kind;          // a set: the byte
};
static int g_allocs = 0, g_fail_alloc = -1, g_moves = 0, g_fail_move = -1;
static hipError_t g_alloc_code = hipErrorOutOfMemory, g_move_code = hipErrorInvalidValue, g_pending = hipSuccess;
static std::vector<void *> g_live, g_freed;
static std::vector<copy_rec> g_done;
static std::string g_message;
static hipStream_t const STREAM = (hipStream_t)0x51;

hipError_t bq_device_malloc(void **ptr, size_t bytes) {
    if (g_allocs++ == g_fail_alloc) return g_alloc_code;
    *ptr = malloc(bytes ? bytes : 1);
    g_live.push_back(*ptr);
    return hipSuccess;
}
hipError_t bq_device_free(void *ptr) {
    g_freed.push_back(ptr);
    free(ptr);   // a double free or a pointer never handed out is AddressSanitizer's to report
    return hipSuccess;
}
static hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    if (st != STREAM) return hipErrorInvalidValue;
    if (g_moves++ == g_fail_move) return g_move_code;
    memcpy(dst, src, bytes);
    g_done.push_back({dst, src, bytes, (int)kind});
    return hipSuccess;
}
static hipError_t hipMemsetAsync(void *dst, int byte, size_t bytes, hipStream_t st) {
    if (st != STREAM) return hipErrorInvalidValue;
    if (g_moves++ == g_fail_move) return g_move_code;
    memset(dst, byte, bytes);
    g_done.push_back({dst, nullptr, bytes, byte});
    return hipSuccess;
}
static hipError_t hipGetLastError() {
    const hipError_t e = g_pending;
    g_pending = hipSuccess;
    return e;
}
static const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipSuccess ? "no error" : "invalid value"; }
void bq_set_error(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_message = buf;
}

#include "bq_score_pass.h"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static int times(const std::vector<void *> &v, void *p) {
    int n = 0;
    for (void *q : v) n += q == p;
    return n;
}

// One pass of m requests, request r of kind r % 7.  fail_alloc / fail_move: the allocator call / the copy-or-set call (set-up and
// finish() counted together) that is refused, or -1; pending: the launch error hipGetLastError() holds at finish(); launcher: the
// code a bq_launch_* returned.  The expectations are worked out beside the calls, from the requests alone.
static void run(int m, int fail_alloc, hipError_t alloc_code, int fail_move, hipError_t move_code, hipError_t pending, int launcher) {
    g_allocs = g_moves = 0;
    g_fail_alloc = fail_alloc;
    g_alloc_code = alloc_code;
    g_fail_move = fail_move;
    g_move_code = move_code;
    g_pending = hipSuccess;
    g_live.clear();
    g_freed.clear();
    g_done.clear();
    g_message.clear();
    // host arrays of exactly the requests' sizes: a wrong byte count overruns one of them
    std::vector<std::vector<double>> hin;
    std::vector<std::vector<int64_t>> hout;
    std::vector<std::vector<double>> theirs;   // "the solver's" device buffers
    std::vector<copy_rec> ledger;              // the device-to-host copies finish() owes, in order
    int allocs = 0, moves = 0, launches = 0;
    bool alive = true;                         // no failure so far
    int want_rc = BQ_OK;
    std::string want_msg;
    auto alloc = [&]() {   // one request reaches the allocator when nothing has failed
        if (!alive) return false;
        if (allocs++ == fail_alloc) {
            alive = false;
            want_rc = alloc_code == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
            want_msg = std::string("held-out check setup failed: ") + hipGetErrorString(alloc_code);
        }
        return alive;
    };
    auto move = [&](bool setup) {
        if (!alive) return false;
        if (moves++ == fail_move) {
            alive = false;
            want_rc = setup && move_code == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
            want_msg = std::string(setup ? "held-out check setup failed: " : "held-out check: ") + hipGetErrorString(move_code);
        }
        return alive;
    };
    int rc;
    {
        bq_score_pass pass("held-out check", STREAM);
        CHECK(pass.ok());
        for (int r = 0; r < m; ++r) {
            const size_t count = (size_t)r + 2;
            const size_t before = g_done.size();
            void *p = nullptr;
            switch (r % 7) {
            case 0: {   // a copied input
                hin.emplace_back(count, 1.5 + r);
                p = pass.in(hin.back().data(), count);
                if (alloc() && move(true)) {
                    CHECK(g_done.size() == before + 1 && g_done.back().dst == p && g_done.back().src == hin.back().data());
                    CHECK(g_done.back().bytes == sizeof(double) * count && g_done.back().kind == hipMemcpyHostToDevice);
                    CHECK(((double *)p)[count - 1] == 1.5 + r);
                }
                break;
            }
            case 1:   // a set input
                p = pass.fill<int>(0xff, count);
                if (alloc() && move(true)) {
                    CHECK(g_done.size() == before + 1 && g_done.back().dst == p && g_done.back().src == nullptr);
                    CHECK(g_done.back().bytes == sizeof(int) * count && g_done.back().kind == 0xff && ((int *)p)[count - 1] == -1);
                }
                break;
            case 2:   // a plain buffer
                p = pass.dev<long long>(count);
                alloc();
                break;
            case 3:   // an output
                hout.emplace_back(count, -1);
                p = pass.out<long long>(hout.back().data(), count);
                if (alloc()) ledger.push_back({hout.back().data(), p, sizeof(long long) * count, hipMemcpyDeviceToHost});
                break;
            case 4:   // a device-only output: never copied
                p = pass.out<int>((int *)nullptr, count);
                alloc();
                break;
            case 5:   // an output in a buffer of the solver's: no request
                theirs.emplace_back(count, 2.5 + r);
                hin.emplace_back(count, 0.0);
                pass.out_of(hin.back().data(), theirs.back().data(), count);
                if (alive) ledger.push_back({hin.back().data(), theirs.back().data(), sizeof(double) * count, hipMemcpyDeviceToHost});
                CHECK(g_done.size() == before);
                p = alive ? (void *)theirs.back().data() : nullptr;
                break;
            default:   // the column count
                p = pass.columns(40 + r);
                if (alloc() && move(true)) {
                    CHECK(g_done.size() == before + 1 && g_done.back().bytes == sizeof(int) && *(int *)p == 40 + r);
                }
                break;
            }
            CHECK(pass.ok() == alive);
            CHECK((p != nullptr) == alive);                   // null once anything has failed
            CHECK(g_allocs == allocs && g_moves == moves);    // and nothing after the failure reaches the allocator or a copy
        }
        const size_t setup_done = g_done.size();
        const bool setup_ok = alive;
        CHECK(pass.ready() == alive);
        if (pass.ok()) {   // the launches
            ++launches;
            if (launcher != BQ_OK) {
                CHECK(!pass.step(launcher));
                alive = false;
                want_rc = launcher;   // (the launcher's own message stands)
            } else {
                CHECK(pass.step(BQ_OK));
                g_pending = pending;
                if (pending != hipSuccess) {
                    alive = false;
                    want_rc = BQ_ERR_HIP;   // also for an out-of-memory error: the set-up is over
                    want_msg = std::string("held-out check: ") + hipGetErrorString(pending);
                }
            }
        }
        CHECK(launches == (setup_ok ? 1 : 0));                // the caller launches only after a clean set-up
        rc = pass.finish();
        size_t copied = 0;
        while (copied < ledger.size() && move(false)) ++copied;
        CHECK(g_moves == moves);
        CHECK(g_done.size() == setup_done + copied);          // every ledger entry once, none after a failure
        for (size_t i = 0; i < copied; ++i) {
            const copy_rec &got = g_done[setup_done + i], &w = ledger[i];
            CHECK(got.dst == w.dst && got.src == w.src && got.bytes == w.bytes && got.kind == hipMemcpyDeviceToHost);
        }
        CHECK(rc == want_rc);
        CHECK(g_message == want_msg);
        CHECK(g_freed.empty());                               // nothing is freed before the pass goes (the closing sync comes first)
    }
    CHECK(g_freed.size() == g_live.size());                   // exactly the buffers handed out, once each
    for (void *p : g_live) CHECK(times(g_freed, p) == 1);
}

int main() {
    int runs = 0;
    for (int m = 0; m <= 8; ++m) {
        run(m, -1, hipSuccess, -1, hipSuccess, hipSuccess, BQ_OK), ++runs;
        run(m, -1, hipSuccess, -1, hipSuccess, hipErrorInvalidValue, BQ_OK), ++runs;
        run(m, -1, hipSuccess, -1, hipSuccess, hipErrorOutOfMemory, BQ_OK), ++runs;
        run(m, -1, hipSuccess, -1, hipSuccess, hipSuccess, BQ_ERR_BADARG), ++runs;
        for (int f = 0; f < m; ++f) {   // (m requests make at most m allocator calls and at most m copies in all)
            run(m, f, hipErrorOutOfMemory, -1, hipSuccess, hipSuccess, BQ_OK), ++runs;
            run(m, f, hipErrorInvalidValue, -1, hipSuccess, hipSuccess, BQ_OK), ++runs;
            run(m, -1, hipSuccess, f, hipErrorInvalidValue, hipSuccess, BQ_OK), ++runs;
            run(m, -1, hipSuccess, f, hipErrorOutOfMemory, hipSuccess, BQ_OK), ++runs;
        }
    }
    printf("score_pass_check ok (%d passes)\n", runs);
    return 0;
}
