// rope_buffers.h — the owning buffer types of the context (rope_ctx.h): a pointer and the number of elements allocated behind
// it, kept together.  No runtime header: the four functions below are defined by whoever links this — rope_abi.hip over
// hipMalloc / hipFree / hipHostMalloc / hipHostFree, tests/buffers_main.cpp over malloc.  A buffer knows nothing of streams or of
// the context: it never waits, and whoever may have work in flight on a block waits before growing it.
#pragma once

#include <cstddef>
#include <utility>

// 0 or the runtime's error code.  dev_alias non-null: mapped memory, and where the device sees it.
int rope_dev_alloc(void **p, size_t bytes);
int rope_dev_free(void *p);
int rope_pinned_alloc(void **p, size_t bytes, void **dev_alias);
int rope_pinned_free(void *p);

namespace rope {

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~DevBuf() { release(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }              // reads like the pointer it owns
    size_t cap() const { return cap_; }              // elements

    // at least n elements: keeps the block when it is large enough, else a new one — contents are not carried over
    int grow(size_t n) { return n <= cap_ ? 0 : reset(n); }
    // a new block of n elements whatever there was; after a failure the buffer is empty
    int reset(size_t n)
    {
        int e = p_ ? rope_dev_free(p_) : 0;
        p_ = nullptr; cap_ = 0;
        if (e == 0) e = rope_dev_alloc(reinterpret_cast<void **>(&p_), n * sizeof(T));
        if (e != 0) { p_ = nullptr; return e; }
        cap_ = n;
        return 0;
    }
    void release() { if (p_) (void)rope_dev_free(p_); p_ = nullptr; cap_ = 0; }
    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// page-locked host memory; `mapped`: the device reads and writes it in place, through dev()
template <typename T>
class PinnedBuf {
public:
    explicit PinnedBuf(bool mapped = false) : mapped_(mapped) {}
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : mapped_(o.mapped_) { swap(o); }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~PinnedBuf() { release(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }                  // null unless mapped
    size_t cap() const { return cap_; }

    int grow(size_t n) { return n <= cap_ ? 0 : reset(n); }
    int reset(size_t n)
    {
        int e = p_ ? rope_pinned_free(p_) : 0;
        p_ = dev_ = nullptr; cap_ = 0;
        if (e == 0) e = rope_pinned_alloc(reinterpret_cast<void **>(&p_), n * sizeof(T), mapped_ ? reinterpret_cast<void **>(&dev_) : nullptr);
        if (e != 0) { p_ = dev_ = nullptr; return e; }
        cap_ = n;
        return 0;
    }
    void release() { if (p_) (void)rope_pinned_free(p_); p_ = dev_ = nullptr; cap_ = 0; }
    void swap(PinnedBuf &o) noexcept { std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(cap_, o.cap_); std::swap(mapped_, o.mapped_); }

private:
    T *p_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0;
    bool mapped_;
};

}  // namespace rope
