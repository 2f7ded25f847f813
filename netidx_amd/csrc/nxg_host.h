// nxg_host.h -- what the host translation units of the C ABI share: the context, the error
// convention, the status-ring call helpers, buffer growth and the column helpers. Host only and
// not ABI: no .hip file and no header a .hip file includes may include it.
//
//   nxg_ctx.cpp          contexts, columns, the status ring, host staging, debug entries, framing
//   nxg_api.cpp          update decode / encode, the async backlog, nxg_ctx_sync, To batches
//   nxg_api_archive.cpp  archive batches, zstd, windows and images, recording, the RecordIndex,
//                        replay
//   nxg_api_oneshot.cpp  a oneshot reply: the pathmap and deltas sections, the shard's and the
//                        reply's framing
//   nxg_api_fanout.cpp   partition, dispatch, publish, per-client frames, the value table
//   nxg_api_route.cpp    write / Subscribe / reply routing, the path table
//   nxg_api_range.cpp    byte-range and share decode (multi-GPU)
//
// Error convention follows netidx-ffi (netidx-ffi/src/error.rs:19-29): fallible calls return
// bool and fill NetidxError.msg with a heap string released by nxg_error_free.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/nxg_codec.h"
#include "nxg_devbuf.h"
#include "nxg_internal.h"

constexpr int kStatusRing = 1024;  // at most kStatusRing/2 async calls in flight

// The ctx's own stream, destroyed after every other member (it is declared first).
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};

struct NxgCtx {
    // Releases everything the context holds, on its device: the raw allocations below in the
    // destructor's body, then the DevBuf members (they need the device set, and no stream), the
    // stream last. The caller has drained the stream.
    ~NxgCtx();
    OwnedStream own;
    int device = 0;
    hipStream_t stream = nullptr;
    int ncu = 0;
    int grid_enc_f64 = 0, grid_enc_gen = 0;
    // status ring: one DevStatus per call, the whole ring re-zeroed once per lap
    DevStatus* dst = nullptr;
    DevStatus* hst = nullptr;  // pinned mirror
    DevStatus* hst_dev = nullptr;  // ... as the device addresses it (the status gather's target)
    uint32_t calls = 0;
    // Calls numbered below gathered_to (call sequence numbers: `calls` at their begin_call,
    // compared modulo 2^32) have a status gather enqueued behind them (nxg_status.hip), so
    // nxg_ctx_sync gathers only the pending calls from there on. At most kStatusRing/2 calls are
    // pending and a gather covers pending calls only, so it never overwrites an hst slot the
    // host has not consumed: the host took its copy of every older slot at the sync before.
    // Every error return of a function that enqueues gathers clears the record (gather_forget).
    uint32_t gathered_to = 0;
    uint32_t epoch = 0;
    // (every DevBuf frees itself with the ctx; the fixed-size allocations are freed by ~NxgCtx)
    DevBuf<uint64_t> tstat;
    DevBuf<uint8_t> glws;          // general decode: lane words, 256 B per tile
    uint64_t* gruns = nullptr;     // general decode: run summaries + bases
    bool no_fa = false;            // NXG_ARCH_PATH=exact: archive batches on the exact decoder only
    DevBuf<uint8_t> dscratch;      // dispatch: counters, offsets, block sums, unmatched count
    int wgs_dec_gen = 0;
    // f64 decoder choice: the length-run decoder (nxg_decode_f64_run.hip) unless the frames of
    // this connection have record lengths that vary record to record; then the single-pass
    // decoder of any f64 frame (nxg_decode_f64_x.hip) for the next kIrregularCalls calls
    // (NXG_F64_PATH=x forces it)
    DevBuf<uint8_t> rdesc;  // length-run decoder: 16-byte tile descriptors
    uint32_t irregular_left = 0;
    bool force_x = false;
    // before both: the one-launch decoder of frames whose ids count up by one
    // (nxg_decode_f64_seq.hip), unless it rejected a recent frame of this connection: then it is
    // skipped for the next kSeqSkipCalls calls (NXG_F64_PATH=run skips it always)
    uint32_t seq_left = 0;
    bool no_seq = false;
    // a backlog of such frames (nxg_decode_frames_async): grouped into launches of the backlog
    // kernel on a grid of seq_group_wgs resident workgroups (NXG_F64S_GROUP=0: one launch per
    // frame; NXG_F64S_GROUP_WGS=n caps the grid, tests)
    bool seq_group = true;
    int seq_group_wgs = 0;
    uint32_t bl_launches = 0, bl_frames = 0;  // decode launches / frames of the last backlog call
    // the sequential-id f64 encoder (nxg_encode_f64_seq.hip): after it declines a batch (ids not
    // counting up by one) it is skipped for the next kSeqSkipCalls f64 encodes; NXG_F64_ENC=tile
    // skips it always
    DevBuf<uint8_t> pscratch;  // the type-partitioned view's counts and offsets
    uint32_t enc_seq_left = 0;
    uint32_t last_enc_kernel = 0;  // the last f64 encode: 1 sequential-id kernel, 2 tiled (debug)
    bool no_enc_seq = false;
    // mixed decode: the fast decoder (nxg_decode_mixed.hip) unless it rejected a recent frame of
    // this connection; then the general decoder for the next kMixFailCalls calls
    // (NXG_MIXED_PATH=general: always the general decoder)
    uint32_t mix_left = 0;
    bool no_fmx = false;
    uint32_t last_route = 0;  // the decoder of the last finish_decode: a FAST_* code (debug)
    // the fast mixed decoder's count pass: lean (one-byte-prefix Update candidates only, then the
    // tiles where that found no chain recounted from every kind) while this connection's last
    // decoded frame had at most 1 tile in 32 holding a Heartbeat or a two-byte prefix
    // (DevStatus.diag[0], from the resolve pass), else every candidate kind (NXG_FMX_COUNT=full
    // always, =lean always)
    bool fmx_full = false;
    int fmx_count_mode = 0;  // 0 adaptive, 1 full, 2 lean
    int wgs_fmx[2] = {0, 0};
    uint32_t f64r_flags = 0;  // NXG_F64R_FLAGS (tests): 1 every tile exact, 2 never hand over
    uint32_t patience = 128;  // NXG_LOOKBACK_PATIENCE: look-back polls before self-help
    DevBuf<uint8_t> dframe;
    DevBuf<uint64_t> escratch;
    NxgColumns dcols{};  // device staging columns for host-resident outputs/inputs
    bool dcols_valid = false;
    DevBuf<uint8_t> dheap;
    // device staging of a host-resident NxgWriteCols (nxg_decode_writes / nxg_encode_writes)
    DevBuf<uint8_t> dwflags;
    DevBuf<uint64_t> dwid;
    // write routing (nxg_route_writes.hip): the first Unsubscribe row per Id, tagged with the
    // call's epoch (24 bits; the table is cleared when it is grown and when the epoch wraps)
    DevBuf<uint64_t> rw_first;
    uint32_t rw_epoch = 0;
    // reply routing (nxg_route_replies.hip): the first span per Id and per pending request, tagged
    // likewise with one epoch for both
    DevBuf<uint64_t> rr_first_id, rr_first_q;
    uint32_t rr_epoch = 0;
    // in-flight async operations (completed in order by nxg_ctx_sync)
    struct Pending {
        int kind;  // 1 decode, 2 encode
        int fast;
        const uint8_t* frame;
        uint64_t len;
        NxgColumns* cols;
        uint64_t* len_out;
        uint64_t cap;  // encode: the output capacity
        DevStatus* st;
        uint32_t slot;
        uint32_t flags = 0;            // decode: the caller's NXG_DECODE_* flags
        const uint8_t* heap = nullptr;  // encode: the heap and the output buffer
        uint8_t* out = nullptr;
        uint32_t seq = 0;  // the call's sequence number (NxgCtx::calls at its begin_call)
    };
    std::vector<Pending> pending;
    // zstd (compressed archive records): predefined tables, literal buffers, descriptors
    void* zdefs = nullptr;
    uint8_t* zlit = nullptr;
    int zgrid = 0;
    DevBuf<uint8_t> zrecs;
    // zstd compression (nxg_archive_compress): the predefined distributions' encoding tables, the
    // waves' literal / sequence slabs, descriptors, the frames' slots and their packed copy
    void* zc_tables = nullptr;
    uint8_t* zc_slab = nullptr;
    int zc_grid = 0;
    DevBuf<uint8_t> zc_recs, zc_out, zc_pack;
    DevBuf<uint8_t, DevMem::Pinned> zc_hpin;  // pinned host staging of the packed frames
    hipEvent_t zc_ev[2] = {nullptr, nullptr};  // around the compressor kernel (diagnostics)
    float zc_kernel_ms = 0.f;
    DevStatus last{};  // last completed decode's device status (diagnostics)
    uint64_t fa_last[8] = {};  // the last fast archive attempt's FaHead (diagnostics)
    // a window of archive records / its image (nxg_archive_window.hip): the head and the records
    // or the image's table, and the pinned host mirror of head + records
    DevBuf<uint8_t> aw_dev;
    DevBuf<uint8_t, DevMem::Pinned> aw_host;
    // the RecordIndex calls (nxg_archive_index.hip): the writer's (record, Id) table, cleared by a
    // memset per call; the scan's offsets / result words and their pinned host mirror
    DevBuf<uint8_t> aix_table;
    DevBuf<uint8_t> aix_dev;
    DevBuf<uint8_t, DevMem::Pinned> aix_host;
    // nxg_oneshot_assemble_shard: pinned staging of the shard's two small heads
    DevBuf<uint8_t, DevMem::Pinned> os_host;
    uint64_t last_split = 0;  // last completed encode's DevStatus.split_start
};

namespace nxg_host {

void set_err(NetidxError* err, const char* fmt, ...);
// `return refuse(err, "...")`: the message (taken as it is, no format) as the error, and false.
bool refuse(NetidxError* err, const char* msg);

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            ::nxg_host::set_err(err, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                       \
            return false;                                                                  \
        }                                                                                  \
    } while (0)

// A launch's result under the wording of its site: "<what>: <the HIP error>".
bool launch_ok(hipError_t e, const char* what, NetidxError* err);
bool set_device(NxgCtx* c, NetidxError* err);
// An entry point that would overtake the async calls in flight refuses.
bool no_pending(NxgCtx* c, NetidxError* err);
bool is_device_ptr(const void* p);
// Every non-null pointer of the list is device memory.
bool all_device(std::initializer_list<const void*> ps);

// ---- the status ring (nxg_ctx.cpp) -------------------------------------------------------------
// Next status slot + epoch for one call. Slot k is zeroed by the call that used slot
// k - kStatusRing/2 (nxg_zero_slot: block 0 of its kernel, or end_call when it launched none), so
// at most kStatusRing/2 calls may be in flight. Every begin_call is paired with an end_call:
// with_call below does that, and everything but the two backlog paths named there goes through it.
bool begin_call(NxgCtx* c, DevStatus** st, uint32_t* slot, NetidxError* err);
// After a call's launches (or a failure to launch): if no kernel took the zero-ahead slot (an
// empty frame or batch launches nothing), clear it here, so that the call kStatusRing/2 later
// does not inherit this ring lap's status bits.
bool end_call(NxgCtx* c, NetidxError* err);

// A status slot for one device call and the launches `enqueue(st)` makes in it. The zero-ahead
// slot is settled whatever enqueue returned (a failed grow or launch included), and an end_call
// failure is reported in preference to enqueue's.
// Exceptions, which call begin_call themselves: decode_seq_backlog and the length-run stream path
// of decode_frames_async_impl (nxg_api.cpp). Each of their frames hands nxg_take_zero_slot() to its
// launch or clears it at once when the frame is empty, so no end_call is owed, and the frames
// become pending only after their launch.
template <class F>
bool with_call(NxgCtx* c, DevStatus** st, uint32_t* slot, NetidxError* err, F&& enqueue) {
    if (!begin_call(c, st, slot, err)) return false;
    const bool ok = enqueue(*st);
    return end_call(c, err) && ok;
}

// The slot's DevStatus in host memory after the stream has drained: one copy, whatever further
// small copies `also()` enqueues, one synchronize.
template <class F>
bool fetch_status(NxgCtx* c, DevStatus* st, uint32_t slot, DevStatus* h, NetidxError* err,
                  F&& also) {
    HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
    if (!also()) return false;
    HIPCHK(hipStreamSynchronize(c->stream));
    *h = c->hst[slot];
    return true;
}
inline bool fetch_status(NxgCtx* c, DevStatus* st, uint32_t slot, DevStatus* h, NetidxError* err) {
    return fetch_status(c, st, slot, h, err, [] { return true; });
}

// Enqueues a status gather for the pending calls that none covers yet (the pending calls used
// consecutive ring slots and sequence numbers). Nothing to do: no launch.
bool gather_pending(NxgCtx* c, NetidxError* err);
// After a failure: whatever gather was enqueued may cover calls that never became pending, or
// may not have been launched at all; the next nxg_ctx_sync gathers every pending call again.
void gather_forget(NxgCtx* c);

// ---- buffers -----------------------------------------------------------------------------------
// Grows `b` to hold `need` elements (nxg_devbuf.h: the steps, and what a failure leaves behind).
template <class Buf, class Ops>
bool grow_with(Buf& b, size_t need, GrowPolicy pol, Ops& ops, NetidxError* err) {
    const GrowFail f = b.grow(need, pol, ops);
    if (!f.step) return true;
    set_err(err, "growing a buffer to %zu elements: %s failed: %s", need, f.step,
            Ops::errstr(f.code));
    return false;
}

template <class Buf>
bool grow(NxgCtx* c, Buf& b, size_t need, GrowPolicy pol, NetidxError* err) {
    HipOps ops{c->stream};
    return grow_with(b, need, pol, ops, err);
}

bool ensure_dscratch(NxgCtx* c, size_t need, NetidxError* err);  // whichever entry point runs (bytes)
bool ensure_tstat(NxgCtx* c, size_t words, NetidxError* err);
bool ensure_escratch(NxgCtx* c, size_t words, NetidxError* err);
bool ensure_rdesc(NxgCtx* c, size_t bytes, NetidxError* err);
bool ensure_glws(NxgCtx* c, size_t bytes, NetidxError* err);

// ---- columns and host staging (nxg_ctx.cpp) ----------------------------------------------------
// w: the companion columns of a To frame's Write rows (null for From)
ColsDesc desc_of(const NxgColumns* c, const NxgWriteCols* w = nullptr);
void cols_free_impl(NxgColumns* c);
// On failure nothing stays allocated and *o is all zero.
bool cols_alloc_impl(uint32_t layout, uint64_t cr, uint64_t cc, uint64_t ck, uint32_t mem,
                     NxgColumns* o, NetidxError* err);
bool mixed_capable(const NxgColumns* c);
// device staging columns shaped like `like` (grown on demand)
bool ensure_dcols(NxgCtx* c, const NxgColumns* like, NetidxError* err);
// view of the device staging columns restricted to `like`'s layout and capacities
NxgColumns staged_view(NxgCtx* c, const NxgColumns* like);
bool copy_cols_d2h(NxgCtx* c, const NxgColumns* d, NxgColumns* h, NetidxError* err);
bool copy_cols_h2d(NxgCtx* c, const NxgColumns* h, NxgColumns* d, NetidxError* err);
bool frame_to_device(NxgCtx* c, const uint8_t* frame, uint64_t len, const uint8_t** df,
                     NetidxError* err);

// ---- archive calls (nxg_api_archive.cpp) -------------------------------------------------------
// The records of a decoded window as row ranges: hbeg[i] / hend[i] for record i and hbeg[n_recs] =
// the end of the last record (0 without records). false: an info whose rows leave the window,
// whose row_off decreases or whose rows overlap the record before (the message says which).
bool window_records(const NxgColumns* window, const NxgArchiveBatchInfo* info, uint32_t n_recs,
                    std::vector<uint64_t>* hbeg, std::vector<uint64_t>* hend, NetidxError* err);
// the words for a kRec* cause (nxg_record.h) of a refused entry or window row
const char* rec_cause(uint32_t cause);

// ---- update decode / encode (nxg_api.cpp) ------------------------------------------------------
// path codes of a fast attempt (Pending::fast): homogeneous f64 (SEQ, RUN, X) or mixed (MIX)
enum { FAST_NONE = 0, FAST_RUN = 1, FAST_X = 2, FAST_MIX = 3, FAST_SEQ = 4 };

// Homogeneous-f64 attempt; *path receives the FAST_* code of the decoder that was enqueued.
// try_seq: the sequential-id decoder may be tried first (not on a rerun after it declined).
bool enqueue_dec_fast(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, DevStatus* st,
                      int* path, NetidxError* err, bool try_seq = true);
// finish a device decode: read status, fall back to the general kernel if the f64 kernel
// rejected the frame, fill the user-visible status
// `fetched`: the caller has already copied the status ring to c->hst after the stream drained.
// `redone` (optional) is set when a fallback decoder rewrote the columns here, i.e. after every
// call enqueued behind this one had already run.
bool finish_decode(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, int tried_fast,
                   DevStatus* st, uint32_t slot, NxgStatus* ust, NetidxError* err,
                   bool fetched = false, bool* redone = nullptr);
bool finish_encode(NxgCtx* c, const NxgColumns* in, DevStatus* st, uint32_t slot,
                   uint64_t* len_out, uint64_t cap, bool wrote, NetidxError* err,
                   bool fetched = false, int fast = 0, const uint8_t* heap = nullptr,
                   uint8_t* out = nullptr, bool* redone = nullptr);
// An encoder's status as an error: the watchdog, then err_kind (false: err is set).
bool encode_status_ok(const DevStatus& h, NetidxError* err);
// "output buffer too small" unless `total` bytes fit `cap` and no kernel ran out of room.
bool encode_fits(bool capacity, uint64_t total, uint64_t cap, NetidxError* err);

// memory touched by a call (nxg_ctx_sync's ordering of late fallbacks, the value table's checks)
struct Span {
    uintptr_t lo, hi;
};
Span span_of(const void* p, uint64_t bytes);
// every column array of `c`, sized by its capacity (or its count, if larger)
void cols_spans(const NxgColumns* c, std::vector<Span>* v);
bool overlaps(const std::vector<Span>& a, const std::vector<Span>& b);

}  // namespace nxg_host
