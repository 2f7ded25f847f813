// nxg_devbuf.h -- the one owner of a grow-on-demand GPU buffer (device or pinned host memory) and
// the one routine that grows it.
//
// Invariant: a buffer is empty (null pointer, capacity 0) or it holds a live allocation of
// exactly `cap` elements. Growing never leaves a null pointer under a non-zero capacity, nor a
// capacity over freed memory, whichever step fails; so a call that follows a failed one grows
// again instead of handing a null pointer to a copy or a kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

enum class DevMem { Device, Pinned };

// How large a grown buffer becomes, in elements:
//   max(need + (slack ? need / 4 : 0), doubling ? 2 * cap : 0, floor)
// and whether the whole new allocation is zeroed (on the stream) before it is used.
struct GrowPolicy {
    size_t floor;
    bool doubling;
    bool slack;
    bool zero;
};

// One constant per row of the table in DESIGN.md ("Grow-on-demand buffers").
constexpr GrowPolicy kGrowDouble{0, true, false, false};           // d/pscratch, aw_*, aix_*, stage
constexpr GrowPolicy kGrowDouble64K{1 << 16, true, false, false};  // rdesc, glws
constexpr GrowPolicy kGrowTileStatus{4096, true, false, true};     // tstat (words)
constexpr GrowPolicy kGrowEncScratch{1024, false, false, false};   // escratch (words)
constexpr GrowPolicy kGrowFrame{1 << 20, false, false, false};     // dframe, dheap
constexpr GrowPolicy kGrowWriteCols{1024, false, false, false};    // dwflags + dwid (rows)
constexpr GrowPolicy kGrowZstdRecs{1 << 16, false, false, false};  // zrecs
constexpr GrowPolicy kGrowZstdEnc{1 << 16, false, true, false};    // zc_recs, _out, _pack, _hpin
constexpr GrowPolicy kGrowFirstTable{4096, false, false, true};    // rw_first, rr_first_* (words)

inline size_t grow_size(size_t need, size_t cap, GrowPolicy pol) {
    size_t n = pol.slack ? need + need / 4 : need;
    if (pol.doubling) n = std::max(n, cap * 2);
    return std::max(n, pol.floor);
}

// What a buffer is made of; DevBuf below owns one of these.
struct DevBufState {
    void* p = nullptr;
    size_t cap = 0;  // elements
};

// A failed step of growing: the name of the operation and its error code (no step: success).
struct GrowFail {
    const char* step = nullptr;
    int code = 0;
};

// The steps of growing, over the four operations they need. Ops has
//   int sync();  int free(void* p, DevMem m);  int alloc(void** p, size_t bytes, DevMem m);
//   int zero(void* p, size_t bytes);
// each returning 0 on success (HipOps below in production; a scripted fake in the CPU test).
// A failed sync leaves the buffer as it was; any later failure leaves it empty.
template <class Ops>
GrowFail devbuf_grow_steps(DevBufState& s, size_t elem, DevMem mem, size_t need, GrowPolicy pol,
                           Ops& ops) {
    if (need <= s.cap) return {};
    const size_t n = grow_size(need, s.cap, pol);
    int e;
    if ((e = ops.sync())) return {"stream synchronize", e};
    void* old = s.p;
    s.p = nullptr;
    s.cap = 0;
    if (old && (e = ops.free(old, mem))) return {"free", e};
    void* p = nullptr;
    if ((e = ops.alloc(&p, n * elem, mem))) return {"allocation", e};
    s.p = p;  // (owned from here on: a failed memset below frees it again)
    if (pol.zero && (e = ops.zero(p, n * elem))) {
        s.p = nullptr;
        (void)ops.free(p, mem);
        return {"memset", e};
    }
    s.cap = n;
    return {};
}

struct HipOps {
    hipStream_t stream;
    int sync() { return (int)hipStreamSynchronize(stream); }
    int free(void* p, DevMem m) { return (int)(m == DevMem::Device ? hipFree(p) : hipHostFree(p)); }
    int alloc(void** p, size_t bytes, DevMem m) {
        return (int)(m == DevMem::Device ? hipMalloc(p, bytes)
                                         : hipHostMalloc(p, bytes, hipHostMallocDefault));
    }
    int zero(void* p, size_t bytes) { return (int)hipMemsetAsync(p, 0, bytes, stream); }
    static const char* errstr(int e) { return hipGetErrorString((hipError_t)e); }
};

// Move-only owner of `cap()` elements of T in device or pinned host memory. Reads as a T*.
template <class T, DevMem M = DevMem::Device>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : s_(std::exchange(o.s_, DevBufState{})) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            s_ = std::exchange(o.s_, DevBufState{});
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    // Frees the allocation, if any (the caller has set the device and drained the stream).
    void release() {
        if (s_.p) (void)HipOps{nullptr}.free(s_.p, M);
        s_ = DevBufState{};
    }

    T* get() const { return static_cast<T*>(s_.p); }
    operator T*() const { return get(); }
    size_t cap() const { return s_.cap; }

    template <class Ops>
    GrowFail grow(size_t need, GrowPolicy pol, Ops& ops) {
        return devbuf_grow_steps(s_, sizeof(T), M, need, pol, ops);
    }

private:
    DevBufState s_;
};
