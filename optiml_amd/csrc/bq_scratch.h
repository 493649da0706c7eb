// The owner of device buffers: every buffer a one-shot entry point allocates (bq_scratch), and every buffer a long-lived object —
// a problem, a solver, a workspace — keeps (bq_owner, a member of that object), is handed out by, and freed with, one owner.
// A call declares its bq_scratch before the first buffer and lets it go out of scope after the call's closing bq_ctx_sync; an object's
// destroy function synchronises, tears down what is not device memory, and deletes the object.  The destructor (and release, for a
// buffer that regrows or serves the set-up only) is the only place that frees.  Copies, launches and the NOMEM-versus-HIP decision
// stay with the caller, which continues its hipError_t chain from error().  One allocation per request (no arena): bq_device_malloc
// retries, and its test hook compares, per request.
// Needs hipError_t / hipSuccess from the includer and nothing else of HIP (tests/c/scratch_check.cpp compiles it against stubs).
#pragma once
#include <cstddef>

hipError_t bq_device_malloc(void **ptr, size_t bytes);
hipError_t bq_device_free(void *ptr);

template <int N>
struct bq_buffers {
    static constexpr int CAP = N;

    bq_buffers() = default;
    bq_buffers(const bq_buffers &) = delete;
    bq_buffers &operator=(const bq_buffers &) = delete;
    ~bq_buffers() {
        for (int i = 0; i < n_; ++i) (void)bq_device_free(ptrs_[i]);
    }

    // `count` elements of T, or null once a request (this one included) has failed; after a failure the allocator is not called
    // again.  count = 0 is hipMalloc(0): the allocator is asked, answers success with a null pointer, and there is nothing to free.
    template <class T>
    T *dev(size_t count) {
        if (err_ != hipSuccess) return nullptr;
        if (n_ == CAP) {
            err_ = hipErrorOutOfMemory;
            return nullptr;
        }
        void *p = nullptr;
        err_ = bq_device_malloc(&p, sizeof(T) * count);
        if (err_ != hipSuccess) return nullptr;
        if (p != nullptr) ptrs_[n_++] = p;
        return (T *)p;
    }
    // the same into a field of the owning object: *field = dev<T>(count), null on failure
    template <class T>
    hipError_t dev(T **field, size_t count) {
        *field = dev<T>(count);
        return err_;
    }

    // frees one buffer now and forgets it (its slot is free for the next request); null or a pointer this owner did not hand
    // out: nothing happens.  The caller clears its own copy of the pointer.
    void release(const void *ptr) {
        for (int i = 0; ptr != nullptr && i < n_; ++i)
            if (ptrs_[i] == ptr) {
                (void)bq_device_free(ptrs_[i]);
                ptrs_[i] = ptrs_[--n_];
                return;
            }
    }

    hipError_t error() const { return err_; }   // the first failure

  private:
    void *ptrs_[CAP];
    int n_ = 0;
    hipError_t err_ = hipSuccess;
};

using bq_scratch = bq_buffers<16>;   // one call: the largest user (held-out calibration of SMO columns) takes 15
using bq_owner = bq_buffers<64>;     // one object: the largest (the active-set workspace with its CG vectors) takes about 30
