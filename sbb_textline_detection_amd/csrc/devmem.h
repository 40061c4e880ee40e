// devmem.h -- private, host only, no HIP header (a plain host compiler builds it; tests/test_devmem_cpu.py does): who owns the memory a handle
// allocates.  A DeviceMem is a registry of blocks behind one allocator (two function pointers: api.hip gives hipMalloc / hipFree for the handle's
// `mem` and hipHostMalloc / hipHostFree for its `pinned`).  Whatever is allocated through it is freed by release_all() (sbbseg_destroy) at the
// latest, so a pointer stored in a plan struct or in the handle merely points at a block the registry owns.  A DevBuf is the grow-only scratch
// buffer of the run-time paths; ensure() is the one place that grows one.
#pragma once

#include <stddef.h>

#include <vector>

namespace sbbseg {

class DeviceMem {
public:
    typedef int (*AllocFn)(void** p, size_t bytes);     // 0 = success (the backend reports its own error)
    typedef int (*FreeFn)(void* p);
    struct Block { void* p; size_t bytes; size_t serial; bool user; };

    DeviceMem(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;

    // a new block of `bytes` -> *p (left as it was on failure).  `user`: handed to the caller of the C ABI (sbbseg_device_alloc)
    int alloc(void** p, size_t bytes, bool user = false)
    {
        blocks_.reserve(blocks_.size() + 1);             // (may throw: before the backend is asked, so nothing is lost)
        void* q = nullptr;
        if (!alloc_ || alloc_(&q, bytes)) return 1;
        *p = q;
        if (!q) return 0;                                // (a zero-byte request: nothing to own)
        blocks_.push_back({q, bytes, next_serial_++, user});
        total_ += bytes;
        return 0;
    }
    // the block that starts at p, or nullptr when the registry has none
    const Block* find(const void* p) const
    {
        for (size_t i = blocks_.size(); i-- > 0;)
            if (blocks_[i].p == p) return &blocks_[i];
        return nullptr;
    }
    // frees and forgets one block; nullptr is a no-op, a pointer the registry does not own an error (1) that frees nothing.  2 = the backend's
    // free failed (the block is forgotten all the same: there is nothing else to do with it)
    int release(void* p)
    {
        if (!p) return 0;
        const Block* b = find(p);
        if (!b) return 1;
        total_ -= b->bytes;
        blocks_.erase(blocks_.begin() + (b - blocks_.data()));
        return free_(p) ? 2 : 0;
    }
    size_t mark() const { return next_serial_; }
    // frees every block registered since mark() returned `m`
    int release_since(size_t m)
    {
        int rc = 0;
        while (!blocks_.empty() && blocks_.back().serial >= m) rc |= release(blocks_.back().p);      // (serials ascend along the list)
        return rc;
    }
    int release_all() { return release_since(0); }
    size_t bytes() const { return total_; }
    const std::vector<Block>& blocks() const { return blocks_; }

private:
    AllocFn alloc_;
    FreeFn free_;
    std::vector<Block> blocks_;
    size_t total_ = 0, next_serial_ = 0;
};

// Frees what a function allocated from a registry unless the function reaches commit(): the plan-building calls, whose op is only pushed at the end.
struct AllocScope {
    DeviceMem& mem;
    size_t from;
    bool committed = false;
    explicit AllocScope(DeviceMem& m) : mem(m), from(m.mark()) {}
    AllocScope(const AllocScope&) = delete;
    ~AllocScope() { if (!committed) (void)mem.release_since(from); }
    void commit() { committed = true; }
};

// A temporary of n elements that lives as long as the holder (the debug entry points' read-back buffers).
template <typename T>
struct ScopedBlock {
    DeviceMem& mem;
    T* p = nullptr;
    explicit ScopedBlock(DeviceMem& m) : mem(m) {}
    ScopedBlock(const ScopedBlock&) = delete;
    ~ScopedBlock() { (void)mem.release(p); }
    int alloc(size_t n) { return mem.alloc((void**)&p, n * sizeof(T)); }
};

// A grow-only buffer: cap bytes at p, in a block a DeviceMem owns.
template <typename T>
struct DevBuf { T* p = nullptr; size_t cap = 0; };

// b holds at least `bytes` afterwards.  Enough already: no allocator call.  Else the old block is released and b is {nullptr, 0} BEFORE the new
// one is requested, so a failed request leaves "nothing allocated", never a stale capacity.  (Contents are not carried over.)
template <typename T>
int ensure(DeviceMem& mem, DevBuf<T>& b, size_t bytes)
{
    if (b.cap >= bytes) return 0;
    void* old = b.p;
    b.p = nullptr; b.cap = 0;
    if (mem.release(old)) return 1;
    void* q = nullptr;
    if (mem.alloc(&q, bytes)) return 1;
    b.p = (T*)q; b.cap = bytes;
    return 0;
}

}  // namespace sbbseg
