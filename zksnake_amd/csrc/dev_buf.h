// dev_buf.h -- DevBuf: the scoped owner of one block of the caching device allocator (host.hip).  Plain C++, no HIP include.
// Lifetime rule: dev_free_cached() does NOT wait for the device, and the next dev_alloc_cached() of the same size hands the
// block out again.  So an owner must outlive the work that uses its block: every function with a local DevBuf synchronises
// (its stream or the device) before any return that follows a launch on its success path, and a long-lived owner (MsmPlan)
// synchronises in its destructor body, before its members go.  A failing HIP call after a launch returns at once, and the
// block goes back while that work may still be in flight: that was so before this type existed and it does not change it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zkmi {
int dev_alloc_cached(void** p, size_t bytes);  // host.hip; ZK_OK or ZK_ERR_HIP with the last error set
void dev_free_cached(void* p);                 // nullptr is fine

// In a namespace of its own, named where it is used (`using mem::DevBuf;`): the kernel headers reach this one through msm_plan.h,
// and a unit that includes them for their kernels and says `using namespace zkmi` keeps the short name for its own helpers.
namespace mem {
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    // gives back what it held, then asks for `bytes`; the allocator's status, and empty when that is not ZK_OK
    int alloc(size_t bytes) {
        reset();
        int rc = dev_alloc_cached(&p_, bytes);
        if (rc) p_ = nullptr;
        return rc;
    }
    void reset() { dev_free_cached(p_); p_ = nullptr; }
    template <class T = uint32_t>
    T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr;
};
}  // namespace mem
}  // namespace zkmi
