// One scoring pass of a held-out entry point (bq_mscore.hip): what every such call repeats around its launches.  The pass owns the
// call's bq_scratch, takes its inputs (allocate and copy in, or allocate and set bytes), its device-only buffers and its outputs
// (allocate now, copy out in finish()), keeps the FIRST error and turns it into the call's code and message:
//   before ready()   "<what> setup failed: ..."   BQ_ERR_NOMEM for hipErrorOutOfMemory, else BQ_ERR_HIP
//   after it         "<what>: ..."                BQ_ERR_HIP
// After a failure nothing more reaches the allocator or a copy, and the caller launches only while ok().  A call reads: argument
// checks, requests, `if (pass.ready()) { launches }`, `return bq_ctx_sync_after(ctx, pass.finish())` — the pass goes out of scope
// after that closing sync, which is what frees.  One allocation per request, as bq_scratch has it.
// Needs from the includer: hipError_t, hipSuccess, hipErrorOutOfMemory, hipStream_t, hipMemcpyAsync, hipMemsetAsync,
// hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipGetLastError, hipGetErrorString and BQ_OK, BQ_ERR_HIP, BQ_ERR_NOMEM
// (tests/c/score_pass_check.cpp compiles it against stubs).
#pragma once
#include "bq_scratch.h"

void bq_set_error(const char *fmt, ...);

struct bq_score_pass {
    static constexpr int OUTS = 12;   // the ledger: the largest user (held-out calibration) registers 10

    bq_score_pass(const char *what, hipStream_t stream) : what_(what), st_(stream) {}

    bool ok() const { return rc_ == BQ_OK; }

    // `count` elements of T on the device; null once anything has failed
    template <class T>
    T *dev(size_t count) {
        if (!ok()) return nullptr;
        T *p = mem_.dev<T>(count);
        note(mem_.error());
        return p;
    }
    // the same, filled from `count` elements at host (which must stay valid until the call's closing sync)
    template <class T>
    T *in(const T *host, size_t count) {
        T *p = dev<T>(count);
        if (ok()) note(hipMemcpyAsync(p, host, sizeof(T) * count, hipMemcpyHostToDevice, st_));
        return ok() ? p : nullptr;
    }
    // the same, every byte set to `byte`
    template <class T>
    T *fill(int byte, size_t count) {
        T *p = dev<T>(count);
        if (ok()) note(hipMemsetAsync(p, byte, sizeof(T) * count, st_));
        return ok() ? p : nullptr;
    }
    // the product's column count as a device integer of this call's own (the solver's nlive is 0 once every column has stopped)
    int *columns(int k) {
        k_ = k;
        return in(&k_, 1);
    }
    // an output: `count` elements of T on the device that finish() copies to host; a null host: a device-only result, not copied
    template <class T, class H>
    T *out(H *host, size_t count) {
        T *p = dev<T>(count);
        out_of(host, p, count);
        return p;
    }
    // an output that lives in a buffer of the solver's: finish() copies `count` elements from device to host
    template <class T, class H>
    void out_of(H *host, const T *device, size_t count) {
        static_assert(sizeof(T) == sizeof(H), "an output is copied byte for byte");
        if (!ok() || host == nullptr) return;
        if (nout_ == OUTS) return note(hipErrorOutOfMemory);
        outs_[nout_++] = {host, device, sizeof(T) * count};
    }

    // closes the set-up: true when every request and copy so far succeeded; a later failure is a failure of the pass itself
    bool ready() {
        launched_ = true;
        return ok();
    }
    void check(hipError_t e) { note(e); }   // of a kernel launch: hipGetLastError()
    // the code of a launcher that has set its own message (bq_launch_*); returns ok()
    bool step(int rc) {
        if (ok()) rc_ = rc;
        return ok();
    }

    // after the last launch: the pending launch error, then every output's copy, once; the code for bq_ctx_sync_after
    int finish() {
        if (ok()) note(hipGetLastError());
        for (int i = 0; i < nout_ && ok(); ++i)
            note(hipMemcpyAsync(outs_[i].host, outs_[i].device, outs_[i].bytes, hipMemcpyDeviceToHost, st_));
        return rc_;
    }

  private:
    struct output {
        void *host;
        const void *device;
        size_t bytes;
    };

    void note(hipError_t e) {
        if (e == hipSuccess || !ok()) return;
        if (launched_) {
            bq_set_error("%s: %s", what_, hipGetErrorString(e));
            rc_ = BQ_ERR_HIP;
        } else {
            bq_set_error("%s setup failed: %s", what_, hipGetErrorString(e));
            rc_ = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
        }
    }

    const char *what_;
    hipStream_t st_;
    bq_scratch mem_;
    output outs_[OUTS];
    int nout_ = 0, k_ = 0, rc_ = BQ_OK;
    bool launched_ = false;
};
