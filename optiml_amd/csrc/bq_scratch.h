// The device scratch of one call: every buffer a one-shot entry point allocates is handed out by, and freed with, one bq_scratch.
// Declare it before the first buffer and let it go out of scope after the call's closing bq_ctx_sync: the destructor is the only
// place that frees.  Copies, launches and the NOMEM-versus-HIP decision stay with the caller, which continues its hipError_t chain
// from error().  One allocation per request (no arena): bq_device_malloc retries, and its test hook compares, per request.
// Needs hipError_t / hipSuccess from the includer and nothing else of HIP (tests/c/scratch_check.cpp compiles it against stubs).
#pragma once
#include <cstddef>

hipError_t bq_device_malloc(void **ptr, size_t bytes);
hipError_t bq_device_free(void *ptr);

struct bq_scratch {
    static constexpr int CAP = 16;   // the largest user (held-out calibration) takes 14

    bq_scratch() = default;
    bq_scratch(const bq_scratch &) = delete;
    bq_scratch &operator=(const bq_scratch &) = delete;
    ~bq_scratch() {
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

    hipError_t error() const { return err_; }   // the first failure

  private:
    void *ptrs_[CAP];
    int n_ = 0;
    hipError_t err_ = hipSuccess;
};
