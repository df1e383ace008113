// DevBuf: one device allocation and its size in bytes, freed by its destructor.  Every device pointer a Handle owns is one of
// these (nempc_internal.h), so that nothing keeps a list of what to free.  Nothing of HIP and nothing of the library is
// included: a host program that defines the raw functions below with malloc / free runs the type as it is
// (tests/dev_buf_check.cpp).
#pragma once

#include <cstddef>
#include <utility>

namespace nempc {

// The raw functions (nempc_api.hip: hipMalloc / hipFree, and hipDeviceSynchronize for ensure).  dev_raw_alloc: `bytes` > 0
// of device memory into *p, 0 on success; on failure *p is null, the error text is "hipMalloc (<what>): <hip error string>"
// and the code is NEMPC_ENOMEM.  dev_raw_sync: 0, or the library's code of a failed device synchronisation (error text set).
int dev_raw_alloc(void** p, std::size_t bytes, const char* what);
void dev_raw_free(void* p);
int dev_raw_sync();

template <class T = void>
class DevBuf {
    T* p_ = nullptr;
    std::size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    template <class U>
    U* as() const { return static_cast<U*>(static_cast<void*>(p_)); }
    std::size_t bytes() const { return bytes_; }     // as asked for (0 for an empty array, which still has an address)
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_) dev_raw_free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // a fresh allocation of `bytes` (what it held is freed first); on failure the buffer is empty
    int alloc(std::size_t bytes, const char* what) {
        reset();
        void* p = nullptr;
        // (an empty array still has an address of its own)
        if (const int rc = dev_raw_alloc(&p, bytes ? bytes : 16, what)) return rc;
        p_ = static_cast<T*>(p);
        bytes_ = bytes;
        return 0;
    }
    // grow-only: nothing when it holds `bytes` already; else a device synchronisation -- an earlier launch may still run out of
    // the old allocation on some stream; the first allocation synchronises too -- and then alloc.  A failed synchronisation
    // leaves the buffer as it was.
    int ensure(std::size_t bytes, const char* what) {
        if (bytes_ >= bytes) return 0;
        if (const int rc = dev_raw_sync()) return rc;
        return alloc(bytes, what);
    }
};

}  // namespace nempc
