// nxg_api.cpp -- the C ABI (include/nxg_codec.h): contexts, column allocation, dispatch of the
// gfx950 kernels, host staging for host-resident frames/columns, and host framing.
//
// Error convention follows netidx-ffi (netidx-ffi/src/error.rs:19-29): fallible calls return
// bool and fill NetidxError.msg with a heap string released by nxg_error_free.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nxg_codec.h"
#include "nxg_devbuf.h"
#include "nxg_internal.h"
#include "nxg_path_hash.h"
#include "nxg_record.h"
#include "nxg_replay.h"

namespace {

void set_err(NetidxError* err, const char* fmt, ...) {
    if (!err) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    free(err->msg);
    err->msg = strdup(buf);
}

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_err(err, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                    __LINE__);                                                             \
            return false;                                                                  \
        }                                                                                  \
    } while (0)

constexpr int kStatusRing = 1024;  // at most kStatusRing/2 async calls in flight

}  // namespace

thread_local uint32_t nxg_patience = 128;  // the calling ctx's, set by begin_call
thread_local DevStatus* nxg_zero_slot = nullptr;
thread_local bool nxg_zero_used = false;

struct NxgCtx {
    int device = 0;
    hipStream_t own = nullptr;
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
    // (every DevBuf frees itself with the ctx: a new one needs no line in nxg_ctx_destroy)
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
    uint64_t last_split = 0;  // last completed encode's DevStatus.split_start
};

namespace {

bool set_device(NxgCtx* c, NetidxError* err) {
    HIPCHK(hipSetDevice(c->device));
    return true;
}

// Next status slot + epoch for one call. Slot k is zeroed by the call that used slot
// k - kStatusRing/2 (nxg_zero_slot: block 0 of its kernel, or end_call when it launched none), so
// at most kStatusRing/2 calls may be in flight. Every begin_call is paired with an end_call.
bool begin_call(NxgCtx* c, DevStatus** st, uint32_t* slot, NetidxError* err) {
    *slot = c->calls % kStatusRing;
    *st = c->dst + *slot;
    nxg_patience = c->patience;
    nxg_zero_slot = c->dst + (c->calls + kStatusRing / 2) % kStatusRing;
    nxg_zero_used = false;
    c->calls++;
    c->epoch++;
    if (c->epoch > kEpochMax) {  // wrap: stale words could alias epoch 1 again
        c->epoch = 1;
        if (c->tstat) HIPCHK(hipMemsetAsync(c->tstat, 0, c->tstat.cap() * 8, c->stream));
    }
    return true;
}

// After a call's launches (or a failure to launch): if no kernel took the zero-ahead slot (an
// empty frame or batch launches nothing), clear it here, so that the call kStatusRing/2 later
// does not inherit this ring lap's status bits.
bool end_call(NxgCtx* c, NetidxError* err) {
    if (nxg_zero_used) return true;
    nxg_zero_used = true;
    HIPCHK(hipMemsetAsync(nxg_zero_slot, 0, sizeof(DevStatus), c->stream));
    return true;
}

// Enqueues a status gather for the pending calls that none covers yet (the pending calls used
// consecutive ring slots and sequence numbers). Nothing to do: no launch.
bool gather_pending(NxgCtx* c, NetidxError* err) {
    if (c->pending.empty()) return true;
    const uint32_t first = c->pending.front().seq;
    const uint32_t span = c->pending.back().seq - first + 1;  // (modulo 2^32, like `done`)
    uint32_t done = c->gathered_to - first;  // leading calls already covered
    if (done > span) done = 0;               // the record is older than this backlog
    if (done == span) return true;
    HIPCHK(nxg_launch_status_gather(c->dst, c->hst_dev, (first + done) % kStatusRing,
                                    std::min<uint32_t>(span - done, kStatusRing), kStatusRing,
                                    c->stream));
    c->gathered_to = first + span;
    return true;
}

// After a failure: whatever gather was enqueued may cover calls that never became pending, or
// may not have been launched at all; the next nxg_ctx_sync gathers every pending call again.
void gather_forget(NxgCtx* c) {
    c->gathered_to = c->pending.empty() ? c->calls : c->pending.front().seq;
}

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

// the scratch of whichever entry point runs (bytes)
bool ensure_dscratch(NxgCtx* c, size_t need, NetidxError* err) {
    return grow(c, c->dscratch, need, kGrowDouble, err);
}

bool ensure_tstat(NxgCtx* c, size_t words, NetidxError* err) {
    return grow(c, c->tstat, words, kGrowTileStatus, err);
}

bool ensure_escratch(NxgCtx* c, size_t words, NetidxError* err) {
    return grow(c, c->escratch, words, kGrowEncScratch, err);
}

bool ensure_rdesc(NxgCtx* c, size_t bytes, NetidxError* err) {
    return grow(c, c->rdesc, bytes, kGrowDouble64K, err);
}

bool ensure_glws(NxgCtx* c, size_t bytes, NetidxError* err) {
    return grow(c, c->glws, bytes, kGrowDouble64K, err);
}

// An entry point that would overtake the async calls in flight refuses.
bool no_pending(NxgCtx* c, NetidxError* err) {
    if (c->pending.empty()) return true;
    set_err(err, "an async operation is pending on this ctx; call nxg_ctx_sync first");
    return false;
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

// w: the companion columns of a To frame's Write rows (null for From)
ColsDesc desc_of(const NxgColumns* c, const NxgWriteCols* w = nullptr) {
    ColsDesc d{};
    d.wflags = w ? w->wflags : nullptr;
    d.wid = w ? w->wid : nullptr;
    d.cap_rows = c->cap_rows;
    d.cap_children = c->cap_children;
    d.cap_ctl = c->cap_ctl;
    d.n_rows = c->n_rows;
    d.n_children = c->n_children;
    d.n_ctl = c->n_ctl;
    d.id = c->id;
    d.tag = c->tag;
    d.fixed = c->fixed;
    d.aux = c->aux;
    d.ctag = c->ctag;
    d.cfixed = c->cfixed;
    d.caux = c->caux;
    d.ctl_row = c->ctl_row;
    d.ctl_off = c->ctl_off;
    d.ctl_len = c->ctl_len;
    d.ctl_variant = c->ctl_variant;
    return d;
}

void cols_free_impl(NxgColumns* c) {
    void* ps[] = {c->id, c->tag, c->fixed, c->aux, c->ctag, c->cfixed, c->caux,
                  c->ctl_row, c->ctl_off, c->ctl_len, c->ctl_variant};
    for (void* p : ps) {
        if (!p) continue;
        if (c->mem == NXG_MEM_DEVICE) (void)hipFree(p);
        else (void)hipHostFree(p);
    }
    memset(c, 0, sizeof *c);
}

// On failure nothing stays allocated and *o is all zero.
bool cols_alloc_impl(uint32_t layout, uint64_t cr, uint64_t cc, uint64_t ck, uint32_t mem,
                     NxgColumns* o, NetidxError* err) {
    memset(o, 0, sizeof *o);
    o->layout = layout;
    o->mem = mem;
    o->cap_rows = cr;
    o->cap_children = cc;
    o->cap_ctl = ck;
    auto alloc = [&](void** p, size_t bytes) -> bool {
        bytes = std::max<size_t>(bytes, 16);
        hipError_t e = mem == NXG_MEM_DEVICE ? hipMalloc(p, bytes)
                                             : hipHostMalloc(p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            set_err(err, "column allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
            return false;
        }
        return true;
    };
    bool ok = alloc((void**)&o->id, cr * 8) && alloc((void**)&o->fixed, cr * 8);
    if (ok && layout == NXG_LAYOUT_MIXED) {
        ok = alloc((void**)&o->tag, cr) && alloc((void**)&o->aux, cr * 4) &&
             alloc((void**)&o->ctag, cc) && alloc((void**)&o->cfixed, cc * 8) &&
             alloc((void**)&o->caux, cc * 4) && alloc((void**)&o->ctl_row, ck * 8) &&
             alloc((void**)&o->ctl_off, ck * 8) && alloc((void**)&o->ctl_len, ck * 4) &&
             alloc((void**)&o->ctl_variant, ck);
    }
    if (!ok) cols_free_impl(o);
    return ok;
}

// device staging columns shaped like `like` (grown on demand)
bool mixed_capable(const NxgColumns* c) {
    return c->tag && c->aux && c->ctag && c->cfixed && c->caux && c->ctl_row && c->ctl_off &&
           c->ctl_len && c->ctl_variant;
}

bool ensure_dcols(NxgCtx* c, const NxgColumns* like, NetidxError* err) {
    const bool mixed = mixed_capable(like);
    if (c->dcols_valid && c->dcols.cap_rows >= like->cap_rows &&
        c->dcols.cap_children >= like->cap_children && c->dcols.cap_ctl >= like->cap_ctl &&
        (c->dcols.layout == NXG_LAYOUT_MIXED || !mixed))
        return true;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->dcols_valid) cols_free_impl(&c->dcols);
    c->dcols_valid = false;
    if (!cols_alloc_impl(mixed ? NXG_LAYOUT_MIXED : NXG_LAYOUT_F64, like->cap_rows,
                         like->cap_children, like->cap_ctl, NXG_MEM_DEVICE, &c->dcols, err))
        return false;
    c->dcols_valid = true;
    return true;
}

// view of the device staging columns restricted to `like`'s layout and capacities
NxgColumns staged_view(NxgCtx* c, const NxgColumns* like) {
    NxgColumns v = c->dcols;
    v.layout = like->layout;
    v.cap_rows = like->cap_rows;
    v.cap_children = like->cap_children;
    v.cap_ctl = like->cap_ctl;
    if (!mixed_capable(like)) {
        v.tag = nullptr;
        v.aux = nullptr;
        v.ctag = nullptr;
        v.cfixed = nullptr;
        v.caux = nullptr;
        v.ctl_row = nullptr;
        v.ctl_off = nullptr;
        v.ctl_len = nullptr;
        v.ctl_variant = nullptr;
    }
    return v;
}

constexpr uint32_t kIrregularCalls = 64;
constexpr uint32_t kMixFailCalls = 16;
constexpr uint32_t kSeqSkipCalls = 64;

// path codes of a fast attempt (Pending::fast): homogeneous f64 (SEQ, RUN, X) or mixed (MIX)
enum { FAST_NONE = 0, FAST_RUN = 1, FAST_X = 2, FAST_MIX = 3, FAST_SEQ = 4 };

bool seq_active(const NxgCtx* c) {
    return !c->no_seq && !c->force_x && c->seq_left == 0 && c->irregular_left == 0;
}

// the single-pass decoder of any f64 frame
bool enqueue_dec_x(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, DevStatus* st,
                   NetidxError* err) {
    if (!ensure_tstat(c, nxg_dec_f64x_groups(len), err)) return false;
    HIPCHK(nxg_launch_dec_f64x(f, len, out->id, out->fixed, out->cap_rows, c->tstat, c->epoch, st,
                               c->stream));
    return true;
}

// Homogeneous-f64 attempt; *path receives the FAST_* code of the decoder that was enqueued.
// try_seq: the sequential-id decoder may be tried first (not on a rerun after it declined).
bool enqueue_dec_fast(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, DevStatus* st,
                      int* path, NetidxError* err, bool try_seq = true) {
    if (try_seq && len > 0 && seq_active(c)) {
        *path = FAST_SEQ;
        HIPCHK(nxg_launch_dec_f64s(f, len, out->id, out->fixed, out->cap_rows, st,
                                   nxg_take_zero_slot(), c->stream));
        return true;
    }
    // (a rerun right after the sequential-id decoder declined does not count: the skip lasts
    // kSeqSkipCalls calls after the one that declined)
    if (try_seq && c->seq_left) c->seq_left--;
    if (!c->force_x && c->irregular_left == 0) {
        *path = FAST_RUN;
        if (!ensure_tstat(c, nxg_dec_f64r_groups(len), err)) return false;
        if (!ensure_rdesc(c, 16 * nxg_dec_f64r_tiles(len), err)) return false;
        HIPCHK(nxg_launch_dec_f64r(f, len, 0, len, out->id, out->fixed, out->cap_rows, c->rdesc,
                                   c->tstat, c->epoch, c->f64r_flags, st, c->stream));
        return true;
    }
    if (c->irregular_left) c->irregular_left--;
    *path = FAST_X;
    return enqueue_dec_x(c, f, len, out, st, err);
}

bool enqueue_dec_general(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out,
                         DevStatus* st, NetidxError* err) {
    if (!ensure_glws(c, nxg_dec_gen_scratch_bytes(len), err)) return false;
    const ColsDesc d = desc_of(out);
    HIPCHK(nxg_launch_dec_gen(f, len, d, reinterpret_cast<uint32_t*>(c->glws.get()), c->gruns,
                              c->gruns + (size_t)gdec2::MAX_RUNS * gdec2::RUN_WORDS,
                              c->wgs_dec_gen, st, c->stream));
    return true;
}

// Mixed decode: the fast decoder for frames of short Update messages (it raises fast_fail on
// anything else and finish_decode reruns the frame on the general decoder).
bool enqueue_dec_mixed(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, DevStatus* st,
                       int* path, NetidxError* err) {
    const ColsDesc d = desc_of(out);
    // (frames of 4 GiB or more: the general decoder; the fast path keeps per-tile counts in 32 bits)
    if (len > 0 && len < (1ull << 32) && d.tag && d.ctag && !c->no_fmx && c->mix_left == 0) {
        *path = FAST_MIX;
        // one buffer for both, so that a fallback does not reallocate
        const uint64_t need = std::max(nxg_fmx_scratch_bytes(len), nxg_dec_gen_scratch_bytes(len));
        if (!ensure_glws(c, need, err)) return false;
        const bool lean = c->fmx_count_mode == 2 || (c->fmx_count_mode == 0 && !c->fmx_full);
        HIPCHK(nxg_launch_dec_fmx(f, len, d, c->glws, c->wgs_fmx, st,
                                  c->stream, lean));
        return true;
    }
    if (c->mix_left) c->mix_left--;
    *path = FAST_NONE;
    return enqueue_dec_general(c, f, len, out, st, err);
}

// finish a device decode: read status, fall back to the general kernel if the f64 kernel
// rejected the frame, fill the user-visible status
// `fetched`: the caller has already copied the status ring to c->hst after the stream drained.
// `redone` (optional) is set when a fallback decoder rewrote the columns here, i.e. after every
// call enqueued behind this one had already run.
bool finish_decode(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, int tried_fast,
                   DevStatus* st, uint32_t slot, NxgStatus* ust, NetidxError* err,
                   bool fetched = false, bool* redone = nullptr) {
    if (redone) *redone = false;
    if (!fetched) {
        HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    DevStatus h = c->hst[slot];
    if (tried_fast == FAST_SEQ && len > 0 && h.fast_fail) {
        if (h.irregular & 2u) {
            // not an f64 frame at all: on to the mixed decoders (as after the length-run probe)
            tried_fast = FAST_RUN;
        } else {
            // an f64 frame whose ids do not count up by one: the length-run (or single-pass)
            // decoder, and this one skipped for the next kSeqSkipCalls calls
            c->seq_left = kSeqSkipCalls;
            DevStatus* st2;
            uint32_t slot2;
            if (!begin_call(c, &st2, &slot2, err)) return false;
            const bool ok = enqueue_dec_fast(c, f, len, out, st2, &tried_fast, err, false);
            if (!end_call(c, err) || !ok) return false;
            if (redone) *redone = true;
            HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                                  c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            h = c->hst[slot2];
        }
    }
    // (irregular bit 1: not an f64 frame at all -- straight on to the mixed decoders)
    if (tried_fast == FAST_RUN && len > 0 && h.fast_fail && (h.irregular & 3u) == 1u) {
        // record lengths vary record to record: the single-pass decoder of any f64 frame, for
        // this frame and the next kIrregularCalls ones
        c->irregular_left = kIrregularCalls;
        DevStatus* st2;
        uint32_t slot2;
        if (!begin_call(c, &st2, &slot2, err)) return false;
        const bool ok = enqueue_dec_x(c, f, len, out, st2, err);
        if (!end_call(c, err) || !ok) return false;
        if (redone) *redone = true;
        tried_fast = FAST_X;
        HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        h = c->hst[slot2];
    }
    // a rejected frame: after the f64 decoders the mixed fast path (mixed columns), after that
    // the general decoder
    while (tried_fast && len > 0 && h.fast_fail) {
        if (tried_fast == FAST_MIX) {
            c->mix_left = kMixFailCalls;
            c->fmx_full = true;  // its next attempt with every candidate kind
        }
        DevStatus* st2;
        uint32_t slot2;
        if (!begin_call(c, &st2, &slot2, err)) return false;
        int next = FAST_NONE;
        const bool ok = tried_fast == FAST_MIX
                            ? enqueue_dec_general(c, f, len, out, st2, err)
                            : enqueue_dec_mixed(c, f, len, out, st2, &next, err);
        if (!end_call(c, err) || !ok) return false;
        if (redone) *redone = true;
        HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        h = c->hst[slot2];
        tried_fast = next;
    }
    c->last_route = (uint32_t)tried_fast;
    // the next fast mixed decode's count pass from this frame's mix of tiles
    if (h.path == 4 && len > 0) c->fmx_full = h.diag[0] * 32 > (len + 4095) / 4096;
    if (h.err_key) {  // general decode: the earliest (offset, kind) on the true chain
        h.err_kind = (uint32_t)(~h.err_key & 0xffu);
        h.err_offset = ~h.err_key >> 8;
    }
    c->last = h;
    if (h.timeout || h.err_kind == NXG_TIMEOUT) {
        set_err(err, "device look-back watchdog expired");
        return false;
    }
    NxgStatus s{};
    s.n_rows = h.n_rows;
    s.n_children = h.n_children;
    s.n_ctl = h.n_ctl;
    s.n_heartbeat = h.n_heartbeat;
    s.err_kind = (int32_t)h.err_kind;
    s.err_offset = h.err_offset;
    s.path = len == 0 ? 1 : h.path;
    if (!s.err_kind && h.capacity) s.err_kind = NXG_CAPACITY;
    if (!s.err_kind && !mixed_capable(out) && (h.nonf64 || s.n_ctl || s.n_children))
        s.err_kind = NXG_NOT_F64;
    if (ust) *ust = s;
    out->n_rows = s.n_rows;
    out->n_children = s.n_children;
    out->n_ctl = s.n_ctl;
    out->n_heartbeat = s.n_heartbeat;
    return true;
}

bool copy_cols_d2h(NxgCtx* c, const NxgColumns* d, NxgColumns* h, NetidxError* err) {
    const uint64_t nr = std::min(d->n_rows, h->cap_rows);
    HIPCHK(hipMemcpyAsync(h->id, d->id, nr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h->fixed, d->fixed, nr * 8, hipMemcpyDeviceToHost, c->stream));
    if (mixed_capable(h) && d->tag) {
        const uint64_t nc = std::min(d->n_children, h->cap_children);
        const uint64_t nk = std::min(d->n_ctl, h->cap_ctl);
        HIPCHK(hipMemcpyAsync(h->tag, d->tag, nr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->aux, d->aux, nr * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->ctag, d->ctag, nc, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->cfixed, d->cfixed, nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->caux, d->caux, nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->ctl_row, d->ctl_row, nk * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->ctl_off, d->ctl_off, nk * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->ctl_len, d->ctl_len, nk * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h->ctl_variant, d->ctl_variant, nk, hipMemcpyDeviceToHost,
                              c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return true;
}

bool copy_cols_h2d(NxgCtx* c, const NxgColumns* h, NxgColumns* d, NetidxError* err) {
    const uint64_t nr = h->n_rows, nc = h->n_children, nk = h->n_ctl;
    HIPCHK(hipMemcpyAsync(d->id, h->id, nr * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d->fixed, h->fixed, nr * 8, hipMemcpyHostToDevice, c->stream));
    if (h->layout == NXG_LAYOUT_MIXED) {
        HIPCHK(hipMemcpyAsync(d->tag, h->tag, nr, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->aux, h->aux, nr * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->ctag, h->ctag, nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->cfixed, h->cfixed, nc * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->caux, h->caux, nc * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->ctl_row, h->ctl_row, nk * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->ctl_off, h->ctl_off, nk * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->ctl_len, h->ctl_len, nk * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d->ctl_variant, h->ctl_variant, nk, hipMemcpyHostToDevice,
                              c->stream));
    }
    d->n_rows = nr;
    d->n_children = nc;
    d->n_ctl = nk;
    return true;
}

bool frame_to_device(NxgCtx* c, const uint8_t* frame, uint64_t len, const uint8_t** df,
                     NetidxError* err) {
    const bool dev = is_device_ptr(frame);
    if (dev && ((uintptr_t)frame & 15) == 0) {
        *df = frame;
        return true;
    }
    if (!grow(c, c->dframe, len + 16, kGrowFrame, err)) return false;
    if (len)
        HIPCHK(hipMemcpyAsync(c->dframe, frame, len,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    *df = c->dframe;
    return true;
}

// *fast = 1 when the sequential-id f64 encoder was launched (finish_encode then reruns a batch it
// declines on the tiled encoder); allow_seq = false forces the tiled encoder.
// win: Write mode (To::Write rows; MIXED layout, device NxgWriteCols)
bool enqueue_encode(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                    uint64_t cap, DevStatus* st, NetidxError* err, int* fast = nullptr,
                    bool allow_seq = true, const NxgWriteCols* win = nullptr) {
    if (fast) *fast = 0;
    if (in->layout == NXG_LAYOUT_F64 && !win) {
        const bool try_seq = allow_seq && !c->no_enc_seq && in->n_rows > 0;
        if (try_seq && c->enc_seq_left == 0) {
            HIPCHK(nxg_launch_enc_f64s(in->id, in->fixed, in->n_rows, out, cap, st, c->stream));
            if (fast) *fast = 1;
            return true;
        }
        if (try_seq) c->enc_seq_left--;
        const uint64_t nt = nxg_enc_f64_tiles(in->n_rows);
        if (!ensure_tstat(c, nt, err)) return false;
        HIPCHK(nxg_launch_enc_f64(in->id, in->fixed, in->n_rows, out, cap, c->tstat, c->epoch, st,
                                  c->grid_enc_f64, c->stream));
        return true;
    }
    const uint64_t nt = nxg_enc_general_tiles(in->n_rows);
    if (!ensure_tstat(c, nt, err)) return false;
    if (!ensure_escratch(c, in->n_ctl ? in->n_ctl + 1 + in->n_rows : 1, err)) return false;
    const ColsDesc d = desc_of(in, win);
    HIPCHK(nxg_launch_enc_general(d, heap, out, cap, c->escratch, c->tstat, c->epoch, st,
                                  c->grid_enc_gen, c->stream, 0, win != nullptr));
    return true;
}

bool finish_encode(NxgCtx* c, const NxgColumns* in, DevStatus* st, uint32_t slot,
                   uint64_t* len_out, uint64_t cap, bool wrote, NetidxError* err,
                   bool fetched = false, int fast = 0, const uint8_t* heap = nullptr,
                   uint8_t* out = nullptr, bool* redone = nullptr) {
    if (redone) *redone = false;
    if (!fetched)
        HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
    uint64_t ctl_total = 0;
    if (in->layout == NXG_LAYOUT_MIXED && in->n_ctl)
        HIPCHK(hipMemcpyAsync(&ctl_total, c->escratch + in->n_ctl, 8, hipMemcpyDeviceToHost,
                              c->stream));
    if (!fetched || (in->layout == NXG_LAYOUT_MIXED && in->n_ctl))
        HIPCHK(hipStreamSynchronize(c->stream));
    DevStatus h = c->hst[slot];
    if (fast && h.fast_fail) {
        // the sequential-id encoder declined (ids that do not count up by one, or past 35 bits):
        // the tiled encoder, and the sequential one skipped for the next kSeqSkipCalls encodes
        c->enc_seq_left = kSeqSkipCalls;
        DevStatus* st2;
        uint32_t slot2;
        if (!begin_call(c, &st2, &slot2, err)) return false;
        const bool ok = enqueue_encode(c, in, heap, out, cap, st2, err, nullptr, false);
        if (!end_call(c, err) || !ok) return false;
        if (redone) *redone = true;
        HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        h = c->hst[slot2];
        fast = 0;  // (the tiled encoder's status from here on: last_enc_kernel reports it)
    }
    c->last_split = h.split_start;
    if (in->layout == NXG_LAYOUT_F64) c->last_enc_kernel = fast && !h.fast_fail ? 1u : 2u;
    if (h.timeout) {
        set_err(err, "device look-back watchdog expired");
        return false;
    }
    if (h.err_kind) {
        if (h.err_kind == NXG_TOO_BIG)
            set_err(err, "encode failed: a message exceeds MAX_BATCH (%llu bytes) or a size "
                         "guard (PackError::TooBig)", (unsigned long long)kMaxBatch);
        else
            set_err(err, "encode failed: PackError kind %u", h.err_kind);
        return false;
    }
    const uint64_t total = h.total_bytes + ctl_total;
    if (len_out) *len_out = total;
    if (wrote && (h.capacity || total > cap)) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)total, (unsigned long long)cap);
        return false;
    }
    return true;
}


// ---- memory touched by a call (nxg_ctx_sync's ordering of late fallbacks) ---------------------
struct Span {
    uintptr_t lo, hi;
};

Span span_of(const void* p, uint64_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    return Span{a, p ? a + bytes : a};
}

// every column array of `c`, sized by its capacity (or its count, if larger)
void cols_spans(const NxgColumns* c, std::vector<Span>* v) {
    const uint64_t r = std::max(c->cap_rows, c->n_rows);
    const uint64_t k = std::max(c->cap_children, c->n_children);
    const uint64_t q = std::max(c->cap_ctl, c->n_ctl);
    const std::pair<const void*, uint64_t> a[] = {
        {c->id, r * 8},      {c->fixed, r * 8},   {c->tag, r},         {c->aux, r * 4},
        {c->ctag, k},        {c->cfixed, k * 8},  {c->caux, k * 4},    {c->ctl_row, q * 8},
        {c->ctl_off, q * 8}, {c->ctl_len, q * 4}, {c->ctl_variant, q}};
    for (const auto& x : a)
        if (x.first && x.second) v->push_back(span_of(x.first, x.second));
}

bool overlaps(const std::vector<Span>& a, const std::vector<Span>& b) {
    for (const Span& x : a)
        for (const Span& y : b)
            if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}

// every span of `a` lies inside one span of `by`
bool covered(const std::vector<Span>& by, const std::vector<Span>& a) {
    for (const Span& x : a) {
        bool in = x.lo == x.hi;
        for (const Span& y : by) in = in || (y.lo <= x.lo && x.hi <= y.hi);
        if (!in) return false;
    }
    return true;
}

// ---- a backlog of sequential-id frames, grouped into launches (nxg_f64s_backlog_kernel) ---------
struct SeqPlan {
    uint8_t start;   // a launch starts in front of this frame
    uint8_t reuse;   // it writes the columns of an earlier frame of its launch (kF64sReuse)
    uint32_t tiles;  // its tiles per wave on `waves` waves (0: not a frame for the backlog kernel)
};

// Which frames of a backlog share a launch; returns the number of launches. Pure: addresses and
// lengths only. The waves of one launch run the frames in backlog order, but no wave waits for
// another, so inside a launch no frame may read or write memory that another one writes. One case
// is exempt: frames with the same id and fixed arrays, the same cap_rows and the same length.
// There every row is written by the same wave for both frames (the wave of a row follows from
// the grid, and the rounds a wave makes from the length), and that wave takes them in order
// (kF64sReuse). A launch is cut in front of
// frame j when
//   - frame j is empty, or too long for the backlog kernel (it goes alone, and so ends its launch);
//   - the launch holds kF64sBacklogMax frames;
//   - frame j's bytes overlap the columns of an earlier frame of the launch, or its columns the
//     bytes of one (per-frame launches would run the one wholly before the other);
//   - its columns overlap an earlier frame's otherwise than in the exempt case.
uint32_t plan_seq_backlog(uint32_t n, const uint8_t* const* frames, const uint64_t* lens,
                          const NxgColumns* const* cols, uint32_t waves, SeqPlan* out) {
    std::vector<Span> sp;         // the column spans of the launch's frames, frame after frame
    std::vector<size_t> first;    // frame g0 + i of the launch: sp[first[i], first[i + 1])
    std::vector<Span> mine;
    uint32_t g0 = 0, launches = 0;
    bool open = false;  // the launch takes more frames
    auto hit = [](const Span* a, const Span* ae, const Span* b, const Span* be) {
        for (; a != ae; a++)
            for (const Span* y = b; y != be; y++)
                if (a->lo < y->hi && y->lo < a->hi) return true;
        return false;
    };
    for (uint32_t j = 0; j < n; j++) {
        const bool takes = nxg_f64s_backlog_takes(lens[j]);
        out[j].tiles = takes ? nxg_f64s_tiles_per_wave(lens[j], waves) : 0u;
        mine.clear();
        cols_spans(cols[j], &mine);
        const Span wj = span_of(frames[j], lens[j]);
        bool cut = !open || !takes || j - g0 >= kF64sBacklogMax, reuse = false;
        for (uint32_t i = g0; i < j && !cut; i++) {
            const Span *si = sp.data() + first[i - g0], *se = sp.data() + first[i - g0 + 1];
            const Span wi = span_of(frames[i], lens[i]);
            const Span *mb = mine.data(), *me = mb + mine.size();
            if (hit(&wj, &wj + 1, si, se) || hit(mb, me, &wi, &wi + 1)) {
                cut = true;
            } else if (cols[i]->id == cols[j]->id && cols[i]->fixed == cols[j]->fixed &&
                       cols[i]->cap_rows == cols[j]->cap_rows && lens[i] == lens[j]) {
                reuse = true;
            } else if (hit(mb, me, si, se)) {
                cut = true;
            }
        }
        if (cut) {
            sp.clear();
            first.assign(1, 0);
            g0 = j;
            open = takes;
            if (lens[j] > 0) launches++;
        }
        out[j].start = cut;
        out[j].reuse = !cut && reuse;
        sp.insert(sp.end(), mine.begin(), mine.end());
        first.push_back(sp.size());
    }
    return launches;
}

// a pending decode done again from the start, synchronously (its first attempt's columns were
// overwritten by an earlier frame's late fallback)
bool redo_decode(NxgCtx* c, const NxgCtx::Pending& p, NxgStatus* s, NetidxError* err) {
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    int fast = FAST_NONE;
    const bool ok = !(p.flags & NXG_DECODE_HINT_MIXED)
                        ? enqueue_dec_fast(c, p.frame, p.len, p.cols, st, &fast, err)
                        : enqueue_dec_mixed(c, p.frame, p.len, p.cols, st, &fast, err);
    if (!end_call(c, err) || !ok) return false;
    return finish_decode(c, p.frame, p.len, p.cols, fast, st, slot, s, err);
}

// a pending encode done again, synchronously (its input columns or its output buffer were
// rewritten after it ran)
bool redo_encode(NxgCtx* c, const NxgCtx::Pending& p, const NxgColumns* in, NetidxError* err) {
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    int fast = 0;
    const bool ok = enqueue_encode(c, in, p.heap, p.out, p.cap, st, err, &fast);
    if (!end_call(c, err) || !ok) return false;
    return finish_encode(c, in, st, slot, p.len_out, p.cap, true, err, false, fast, p.heap, p.out);
}

}  // namespace

extern "C" {

const char* nxg_version(void) { return "nxg 0.1.0 gfx950"; }

// Not part of the ABI: the last decode's kernel diagnostics (DevStatus::diag), for profiling.
void nxg_debug_status(NxgCtx* c, unsigned long long out[6]) {
    const DevStatus z{};
    const DevStatus& h = c ? c->last : z;
    out[0] = h.fast_fail;
    out[1] = h.irregular;
    out[2] = h.path;
    out[3] = h.n_rows;
    out[4] = h.err_kind;
    out[5] = h.timeout;
}
// Not part of the ABI: which f64 encoder wrote the last f64 encode (1 sequential-id, 2 tiled).
unsigned nxg_debug_enc_kernel(NxgCtx* c) { return c ? c->last_enc_kernel : 0u; }
// Not part of the ABI: the decoder that produced the last completed decode (the FAST_* code of
// the final attempt: 1 length-run, 2 single-pass, 3 fast mixed, 4 sequential-id, 0 general) and
// the connection's countdowns seq_left, irregular_left, mix_left.
void nxg_debug_route(NxgCtx* c, unsigned out[4]) {
    out[0] = c ? c->last_route : 0u;
    out[1] = c ? c->seq_left : 0u;
    out[2] = c ? c->irregular_left : 0u;
    out[3] = c ? c->mix_left : 0u;
}
void nxg_debug_diag(NxgCtx* c, unsigned long long out[8]) {
    for (int i = 0; i < 8; i++) out[i] = c ? c->last.diag[i] : 0;
}
// Not part of the ABI: the last nxg_decode_frames_async call that the sequential-id decoder took:
// its decode launches, its frames, the backlog kernel's grid (workgroups), grouping on (1) or off.
void nxg_debug_backlog(NxgCtx* c, unsigned long long out[4]) {
    out[0] = c ? c->bl_launches : 0;
    out[1] = c ? c->bl_frames : 0;
    out[2] = c ? (unsigned long long)c->seq_group_wgs : 0;
    out[3] = c ? c->seq_group : 0;
}
// Not part of the ABI, and needs no GPU: the grouping plan of a backlog of n frames at addresses
// wire[j], lens[j] bytes long, into F64 columns id[j], fixed[j] of cap_rows[j] rows, for a grid of
// `waves` waves. start[j]: a launch starts in front of frame j; reuse[j]: the frame writes the
// columns of an earlier frame of its launch; tiles[j]: its tiles per wave (0: it goes alone, on
// the per-frame kernel, or is empty). Returns the number of launches.
uint32_t nxg_debug_f64s_plan(uint32_t n, const uint64_t* wire, const uint64_t* lens,
                             const uint64_t* id, const uint64_t* fixed, const uint64_t* cap_rows,
                             uint32_t waves, uint8_t* start, uint8_t* reuse, uint32_t* tiles) {
    std::vector<NxgColumns> cs(n);
    std::vector<const NxgColumns*> cp(n);
    std::vector<const uint8_t*> fp(n);
    std::vector<SeqPlan> plan(n);
    for (uint32_t j = 0; j < n; j++) {
        memset(&cs[j], 0, sizeof(NxgColumns));
        cs[j].layout = NXG_LAYOUT_F64;
        cs[j].mem = NXG_MEM_DEVICE;
        cs[j].id = (uint64_t*)(uintptr_t)id[j];
        cs[j].fixed = (uint64_t*)(uintptr_t)fixed[j];
        cs[j].cap_rows = cap_rows[j];
        cp[j] = &cs[j];
        fp[j] = (const uint8_t*)(uintptr_t)wire[j];
    }
    const uint32_t launches =
        plan_seq_backlog(n, fp.data(), lens, cp.data(), waves ? waves : 1u, plan.data());
    for (uint32_t j = 0; j < n; j++) {
        start[j] = plan[j].start;
        reuse[j] = plan[j].reuse;
        tiles[j] = plan[j].tiles;
    }
    return launches;
}

// Not part of the ABI, and needs no GPU: one call of the grow routine every DevBuf uses
// (nxg_devbuf.h, through the grow_with that reports production failures) against a scripted fake
// of its four operations. The buffer comes in and goes out as *ptr / *cap (elements of `elem`
// bytes, pinned: host memory); `policy` is the row of the policy table, 0 kGrowDouble to 8
// kGrowFirstTable; fail_op is the operation that fails (0 none, 1 sync, 2 free, 3 alloc,
// 4 memset). ops[i], args[i]: the operations issued, in order, at most 8 (1 sync; 2 free, the
// pointer; 3 alloc, the bytes; 4 memset, the bytes; + 16 on pinned memory); *n_ops their count.
bool nxg_debug_devbuf_grow(uint64_t* ptr, uint64_t* cap, uint32_t elem, bool pinned,
                           uint32_t policy, uint64_t need, uint32_t fail_op, uint32_t* ops,
                           uint64_t* args, uint32_t* n_ops, NetidxError* err) {
    static const GrowPolicy rows[] = {kGrowDouble,     kGrowDouble64K, kGrowTileStatus,
                                      kGrowEncScratch, kGrowFrame,     kGrowWriteCols,
                                      kGrowZstdRecs,   kGrowZstdEnc,   kGrowFirstTable};
    struct Fake {
        uint32_t fail_op, *ops, n;
        uint64_t* args;
        int op(uint32_t code, DevMem m, uint64_t arg) {
            if (n < 8) {
                ops[n] = code + (m == DevMem::Pinned ? 16u : 0u);
                args[n] = arg;
            }
            n++;
            return code == fail_op ? 2 : 0;
        }
        int sync() { return op(1, DevMem::Device, 0); }
        int free(void* p, DevMem m) { return op(2, m, (uintptr_t)p); }
        int alloc(void** p, size_t bytes, DevMem m) {
            const int e = op(3, m, bytes);
            if (!e) *p = (void*)(uintptr_t)(0x7000000000ull + bytes);
            return e;
        }
        int zero(void* p, size_t bytes) { return op(4, DevMem::Device, bytes); }
        static const char* errstr(int) { return "scripted failure"; }
    } fake{fail_op, ops, 0, args};
    struct Raw {
        DevBufState s;
        size_t elem;
        DevMem mem;
        GrowFail grow(size_t need, GrowPolicy pol, Fake& f) {
            return devbuf_grow_steps(s, elem, mem, need, pol, f);
        }
    } raw{{(void*)(uintptr_t)*ptr, (size_t)*cap}, elem, pinned ? DevMem::Pinned : DevMem::Device};
    if (policy >= sizeof rows / sizeof rows[0]) {
        set_err(err, "policy: no such row");
        return false;
    }
    const bool ok = grow_with(raw, need, rows[policy], fake, err);
    *ptr = (uintptr_t)raw.s.p;
    *cap = raw.s.cap;
    *n_ops = fake.n;
    return ok;
}

// Not part of the ABI: the last fast archive attempt's FaHead (fast_fail | arrived << 32, end,
// end_children, items, kids, recounts, decline reasons, 1 + the last declining tile).
void nxg_debug_fa(NxgCtx* c, unsigned long long out[8]) {
    for (int i = 0; i < 8; i++) out[i] = c ? c->fa_last[i] : 0;
}

void nxg_error_free(NetidxError* err) {
    if (!err) return;
    free(err->msg);
    err->msg = nullptr;
}

NxgCtx* nxg_ctx_new(int device, NetidxError* err) {
    NxgCtx* c = new NxgCtx();
    c->device = device;
    auto fail = [&](const char* what, hipError_t e) -> NxgCtx* {
        set_err(err, "%s: %s", what, hipGetErrorString(e));
        delete c;
        return nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return fail("hipGetDeviceProperties", e);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(err, "nxg codec is built for gfx950 (MI355X); device %d is %s", device,
                prop.gcnArchName);
        delete c;
        return nullptr;
    }
    c->ncu = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking)) != hipSuccess)
        return fail("hipStreamCreate", e);
    c->stream = c->own;
    // Default schedule for the look-back (encode) kernels: one workgroup per tile in blockIdx
    // order (grid 0), so the look-back always finds recent inclusive prefixes. NXG_PERSISTENT=1
    // selects a persistent grid instead: every workgroup co-resident, with one block of margin
    // under the occupancy answer (MI355X_MICROARCH.md residency notes).
    auto grid = [&](int occ) { return c->ncu * std::max(1, occ > 2 ? occ - 1 : occ); };
    const char* pe = getenv("NXG_PERSISTENT");
    const bool persist = pe && pe[0] == '1';
    c->grid_enc_f64 = persist ? grid(nxg_occupancy_enc_f64()) : 0;
    c->grid_enc_gen = persist ? grid(nxg_occupancy_enc_general()) : 0;
    if ((e = hipMalloc(&c->dst, sizeof(DevStatus) * kStatusRing)) != hipSuccess)
        return fail("hipMalloc(status)", e);
    if ((e = hipMemset(c->dst, 0, sizeof(DevStatus) * kStatusRing)) != hipSuccess)
        return fail("hipMemset(status)", e);
    // (one slot more: the fast archive decoder's FaHead)
    if ((e = hipHostMalloc(&c->hst, sizeof(DevStatus) * (kStatusRing + 1), hipHostMallocDefault)) !=
        hipSuccess)
        return fail("hipHostMalloc(status)", e);
    if ((e = hipHostGetDevicePointer((void**)&c->hst_dev, c->hst, 0)) != hipSuccess)
        return fail("hipHostGetDevicePointer(status)", e);
    // general decode: run summaries + bases (no initialisation needed)
    const size_t gw = (size_t)gdec2::MAX_RUNS * (gdec2::RUN_WORDS + 4);
    if ((e = hipMalloc(&c->gruns, gw * 8)) != hipSuccess) return fail("hipMalloc(gruns)", e);
    c->wgs_dec_gen = nxg_dec_gen_wgs(c->ncu);
    nxg_fmx_wgs(c->ncu, c->wgs_fmx);
    const char* fp = getenv("NXG_F64_PATH");
    c->force_x = fp && strcmp(fp, "x") == 0;
    c->no_seq = fp && (strcmp(fp, "run") == 0 || strcmp(fp, "x") == 0);
    const char* sg = getenv("NXG_F64S_GROUP");
    c->seq_group = !(sg && sg[0] == '0');
    c->seq_group_wgs = nxg_f64s_backlog_wgs(c->ncu);
    const char* sw = getenv("NXG_F64S_GROUP_WGS");
    if (sw && strtol(sw, nullptr, 0) > 0)
        c->seq_group_wgs = (int)std::min<long>(c->seq_group_wgs, strtol(sw, nullptr, 0));
    const char* fe = getenv("NXG_F64_ENC");
    c->no_enc_seq = fe && strcmp(fe, "tile") == 0;
    const char* mp = getenv("NXG_MIXED_PATH");
    c->no_fmx = mp && strcmp(mp, "general") == 0;
    const char* fc = getenv("NXG_FMX_COUNT");
    c->fmx_count_mode = fc && strcmp(fc, "full") == 0 ? 1 : (fc && strcmp(fc, "lean") == 0 ? 2 : 0);
    const char* ap = getenv("NXG_ARCH_PATH");
    c->no_fa = ap && strcmp(ap, "exact") == 0;
    // (per context: a test context with patience 0 leaves every other context's alone)
    const char* lp = getenv("NXG_LOOKBACK_PATIENCE");
    c->patience = lp ? (uint32_t)strtoul(lp, nullptr, 0) : 128u;
    const char* ff = getenv("NXG_F64R_FLAGS");
    c->f64r_flags = ff ? (uint32_t)strtoul(ff, nullptr, 0) : 0u;
    return c;
}

void nxg_ctx_destroy(NxgCtx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->dcols_valid) cols_free_impl(&c->dcols);
    if (c->gruns) (void)hipFree(c->gruns);
    if (c->zdefs) (void)hipFree(c->zdefs);
    if (c->zlit) (void)hipFree(c->zlit);
    if (c->zc_tables) (void)hipFree(c->zc_tables);
    if (c->zc_slab) (void)hipFree(c->zc_slab);
    for (hipEvent_t e : c->zc_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->dst) (void)hipFree(c->dst);
    if (c->hst) (void)hipHostFree(c->hst);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;  // (every grow-on-demand buffer: the DevBuf members free themselves)
}

bool nxg_ctx_set_stream(NxgCtx* c, void* s, NetidxError* err) {
    if (!c) {
        set_err(err, "null ctx");
        return false;
    }
    if (!set_device(c, err)) return false;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own;
    return true;
}

void* nxg_ctx_stream(NxgCtx* c) { return c ? (void*)c->stream : nullptr; }

bool nxg_columns_alloc(NxgCtx* c, uint32_t layout, uint64_t cap_rows, uint64_t cap_children,
                       uint64_t cap_ctl, uint32_t mem, NxgColumns* out, NetidxError* err) {
    if (!c || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (layout != NXG_LAYOUT_F64 && layout != NXG_LAYOUT_MIXED) {
        set_err(err, "unknown layout %u", layout);
        return false;
    }
    if (mem != NXG_MEM_DEVICE && mem != NXG_MEM_HOST) {
        set_err(err, "unknown memory kind %u", mem);
        return false;
    }
    if (!set_device(c, err)) return false;
    return cols_alloc_impl(layout, cap_rows, cap_children, cap_ctl, mem, out, err);
}

void nxg_columns_free(NxgCtx* c, NxgColumns* cols) {
    if (!cols) return;
    if (c) (void)hipSetDevice(c->device);
    cols_free_impl(cols);
}

bool nxg_decode_updates(NxgCtx* c, const uint8_t* frame, uint64_t len, NxgColumns* out,
                        uint32_t flags, NxgStatus* ust, NetidxError* err) {
    if (!c || !out || (!frame && len)) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (len >= (1ull << 40)) {
        set_err(err, "frame too large (%llu bytes)", (unsigned long long)len);
        return false;
    }
    if (!set_device(c, err)) return false;
    const uint8_t* df;
    if (!frame_to_device(c, frame, len, &df, err)) return false;
    NxgColumns* target = out;
    NxgColumns view;
    const bool host_out = out->mem == NXG_MEM_HOST;
    if (host_out) {
        if (!ensure_dcols(c, out, err)) return false;
        view = staged_view(c, out);
        target = &view;
    }
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    int fast = FAST_NONE;
    const bool ok = !(flags & NXG_DECODE_HINT_MIXED)
                        ? enqueue_dec_fast(c, df, len, target, st, &fast, err)
                        : enqueue_dec_mixed(c, df, len, target, st, &fast, err);
    if (!end_call(c, err) || !ok) return false;
    NxgStatus s;
    if (!finish_decode(c, df, len, target, fast, st, slot, &s, err)) return false;
    // result layout: F64 when the homogeneous kernel produced it (tag/aux not written)
    out->layout = (!mixed_capable(out) || s.path == 1) ? NXG_LAYOUT_F64 : NXG_LAYOUT_MIXED;
    if (host_out) {
        target->n_rows = s.n_rows;
        target->n_children = s.n_children;
        target->n_ctl = s.n_ctl;
        if (s.err_kind == 0) {
            NxgColumns hv = *out;
            if (s.path == 1) hv.tag = nullptr;  // only id/fixed were produced
            if (!copy_cols_d2h(c, target, &hv, err)) return false;
        }
    }
    out->n_rows = s.n_rows;
    out->n_children = s.n_children;
    out->n_ctl = s.n_ctl;
    out->n_heartbeat = s.n_heartbeat;
    if (ust) *ust = s;
    return true;
}

bool nxg_decode_updates_async(NxgCtx* c, const uint8_t* dframe, uint64_t len, NxgColumns* dout,
                              uint32_t flags, NetidxError* err) {
    if (!c || !dout || (!dframe && len)) {
        set_err(err, "null argument");
        return false;
    }
    if (c->pending.size() >= kStatusRing / 2) {
        set_err(err, "too many in-flight async calls (max %d); call nxg_ctx_sync", kStatusRing / 2);
        return false;
    }
    if (dout->mem != NXG_MEM_DEVICE || ((uintptr_t)dframe & 15)) {
        set_err(err, "async decode needs device columns and a 16-byte aligned device frame");
        return false;
    }
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    const uint32_t seq = c->calls - 1;
    int fast = FAST_NONE;
    const bool ok = !(flags & NXG_DECODE_HINT_MIXED)
                        ? enqueue_dec_fast(c, dframe, len, dout, st, &fast, err)
                        : enqueue_dec_mixed(c, dframe, len, dout, st, &fast, err);
    if (!end_call(c, err) || !ok) return false;
    c->pending.push_back({1, fast, dframe, len, dout, nullptr, 0, st, slot, flags});
    c->pending.back().seq = seq;
    return true;
}

}  // extern "C"

namespace {

// A backlog the sequential-id decoder takes, in as few launches as plan_seq_backlog allows.
// Bookkeeping as on the length-run path below: one call per frame, with its own status slot and
// zero-ahead slot; the frames of a launch become pending only once it is enqueued. A frame that
// makes a launch of its own takes the per-frame kernel.
bool decode_seq_backlog(NxgCtx* c, uint32_t n, const uint8_t* const* dframes, const uint64_t* lens,
                        NxgColumns* const* douts, uint32_t flags, NetidxError* err) {
    if (!set_device(c, err)) return false;
    std::vector<SeqPlan> plan(n);
    plan_seq_backlog(n, dframes, lens, douts, 4u * (uint32_t)c->seq_group_wgs, plan.data());
    NxgF64sBacklog b;
    b.n = 0;
    b.pad = 0;
    std::vector<NxgCtx::Pending> pend;
    pend.reserve(std::min<uint32_t>(n, kF64sBacklogMax));
    for (uint32_t j = 0; j < n; j++) {
        const bool last = j + 1 == n || plan[j + 1].start;
        DevStatus* st;
        uint32_t slot;
        if (!begin_call(c, &st, &slot, err)) return false;
        DevStatus* zst = nxg_take_zero_slot();
        pend.push_back({1, FAST_SEQ, dframes[j], lens[j], douts[j], nullptr, 0, st, slot, flags});
        pend.back().seq = c->calls - 1;
        if (lens[j] == 0) {
            // an empty frame launches nothing: its zero-ahead slot is cleared here
            HIPCHK(hipMemsetAsync(zst, 0, sizeof(DevStatus), c->stream));
        } else if (plan[j].start && last) {
            HIPCHK(nxg_launch_dec_f64s(dframes[j], lens[j], douts[j]->id, douts[j]->fixed,
                                       douts[j]->cap_rows, st, zst, c->stream));
            c->bl_launches++;
        } else {
            NxgF64sFrame& f = b.f[b.n++];
            f.wire = dframes[j];
            f.W = lens[j];
            f.oid = douts[j]->id;
            f.oval = douts[j]->fixed;
            f.cap = douts[j]->cap_rows;
            f.st = st;
            f.zst = zst;
            f.tiles_per_wave = plan[j].tiles;
            f.flags = plan[j].reuse ? kF64sReuse : 0u;
            if (last) {
                HIPCHK(nxg_launch_dec_f64s_backlog(b, c->seq_group_wgs, c->stream));
                c->bl_launches++;
                b.n = 0;
            }
        }
        if (last) {
            c->pending.insert(c->pending.end(), pend.begin(), pend.end());
            pend.clear();
        }
    }
    return gather_pending(c, err);
}

bool decode_frames_async_impl(NxgCtx* c, uint32_t n, const uint8_t* const* dframes,
                              const uint64_t* lens, NxgColumns* const* douts, uint32_t flags,
                              NetidxError* err) {
    if (c->pending.size() + n > kStatusRing / 2) {
        set_err(err, "too many in-flight async calls (max %d); call nxg_ctx_sync", kStatusRing / 2);
        return false;
    }
    uint64_t max_len = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (!douts[j] || (!dframes[j] && lens[j])) {
            set_err(err, "null frame or columns at %u", j);
            return false;
        }
        if (douts[j]->mem != NXG_MEM_DEVICE || ((uintptr_t)dframes[j] & 15)) {
            set_err(err, "async decode needs device columns and 16-byte aligned device frames");
            return false;
        }
        max_len = std::max(max_len, lens[j]);
    }
    if (!(flags & NXG_DECODE_HINT_MIXED) && seq_active(c)) {
        c->bl_frames = n;
        c->bl_launches = 0;
        if (c->seq_group && n > 1) return decode_seq_backlog(c, n, dframes, lens, douts, flags, err);
        for (uint32_t j = 0; j < n; j++) c->bl_launches += lens[j] > 0;
    }
    const bool run_path = !(flags & NXG_DECODE_HINT_MIXED) && !c->force_x &&
                          c->irregular_left == 0 && n > 1 && !seq_active(c);
    if (!run_path) {
        for (uint32_t j = 0; j < n; j++)
            if (!nxg_decode_updates_async(c, dframes[j], lens[j], douts[j], flags, err))
                return false;
        return gather_pending(c, err);
    }
    if (!set_device(c, err)) return false;
    // two descriptor arrays: frame j's probe runs beside frame j - 1's emit
    const size_t half = (16 * nxg_dec_f64r_tiles(max_len) + 255) & ~(size_t)255;
    if (!ensure_tstat(c, nxg_dec_f64r_groups(max_len), err)) return false;
    if (!ensure_rdesc(c, 2 * half, err)) return false;
    std::vector<NxgF64rFrame> fr(n);
    std::vector<NxgCtx::Pending> pend;
    pend.reserve(n);
    uint32_t nonempty = 0;  // descriptor arrays alternate over the frames that launch
    for (uint32_t j = 0; j < n; j++) {
        DevStatus* st;
        uint32_t slot;
        if (!begin_call(c, &st, &slot, err)) return false;
        NxgF64rFrame& f = fr[j];
        f.wire = dframes[j];
        f.W = lens[j];
        f.oid = douts[j]->id;
        f.oval = douts[j]->fixed;
        f.cap = douts[j]->cap_rows;
        f.desc = c->rdesc + (nonempty & 1) * half;
        if (lens[j]) nonempty++;
        f.epoch = c->epoch;
        f.st = st;
        f.zst = nxg_take_zero_slot();
        // an empty frame launches nothing: its zero-ahead slot is cleared here
        if (lens[j] == 0) HIPCHK(hipMemsetAsync(f.zst, 0, sizeof(DevStatus), c->stream));
        pend.push_back({1, FAST_RUN, dframes[j], lens[j], douts[j], nullptr, 0, st, slot});
        pend.back().seq = c->calls - 1;
    }
    // (the frames become pending only once their launches are enqueued: a failed launch leaves
    // no call behind whose status slot no kernel wrote)
    HIPCHK(nxg_launch_dec_f64r_stream(fr.data(), n, c->tstat, c->f64r_flags, c->stream));
    // (these frames skipped the sequential-id decoder: they count toward its skip)
    c->seq_left = c->seq_left > n ? c->seq_left - n : 0;
    c->pending.insert(c->pending.end(), pend.begin(), pend.end());
    return gather_pending(c, err);
}

}  // namespace

extern "C" {

// The backlog's status gather is enqueued right behind its last launch (gather_pending), so the
// statuses are in host memory the moment the last decode ends and nxg_ctx_sync waits once.
bool nxg_decode_frames_async(NxgCtx* c, uint32_t n, const uint8_t* const* dframes,
                             const uint64_t* lens, NxgColumns* const* douts, uint32_t flags,
                             NetidxError* err) {
    if (!c || (n && (!dframes || !lens || !douts))) {
        set_err(err, "null argument");
        return false;
    }
    if (decode_frames_async_impl(c, n, dframes, lens, douts, flags, err)) return true;
    gather_forget(c);
    return false;
}

// Completes every in-flight call in order (every one, even after a failure, so that each decode
// gets its fallback and each encode its length); the status returned is the last call's, or the
// first failing call's, and the first error is the one reported.
//
// A call whose fast kernel declined is finished here, after every later call of the backlog has
// run, so what it writes lands out of order. From the first such completion on, `dirty` holds the
// memory rewritten here, and every later call that reads or writes dirty memory is done again, in
// order: a decode whose columns or frame overlap it, an encode whose input columns or output
// buffer do; what those rewrite joins the set. (nxg_codec.h allows a backlog to reuse columns and
// buffers, the later call's result being the one left.)
//
// Doing a call again -- a fallback or a redo -- reads its input again: a decode its frame, an
// encode its columns. If a later call of the backlog wrote into that input, the bytes the call
// should read are gone, unless an earlier call rewrote all of it here (then it holds, the calls in
// between having been redone in order, what the call saw). Otherwise the call fails with an error
// naming it; it never works on the overwritten input.
bool nxg_ctx_sync(NxgCtx* c, NxgStatus* ust, NetidxError* err) {
    if (!c) {
        set_err(err, "null ctx");
        return false;
    }
    if (!set_device(c, err)) return false;
    // One wait: the status slots of the pending calls reach c->hst by a gather kernel in stream
    // order (nxg_status.hip), enqueued behind a backlog by nxg_decode_frames_async already and
    // here for the calls made since; the end of that kernel publishes them to the host.
    const bool gathered = gather_pending(c, err);
    std::vector<NxgCtx::Pending> ps;
    ps.swap(c->pending);
    if (!gathered) {
        // (the calls are dropped, as after any failed step of this function; the stream is
        // drained so that nothing of them is still running when the caller goes on)
        (void)hipStreamSynchronize(c->stream);
        c->gathered_to = c->calls;
        return false;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->gathered_to = c->calls;  // nothing is pending: the record starts afresh
    // (kept aside: the fallbacks below take ring slots of their own, which may wrap)
    std::vector<DevStatus> hs(ps.size());
    for (size_t i = 0; i < ps.size(); i++) hs[i] = c->hst[ps[i].slot];
    if (ust) memset(ust, 0, sizeof *ust);
    bool reported = false, ok = true;
    std::vector<Span> dirty;  // memory rewritten by a call completed out of order
    // does a call behind call i write into `rd`?
    auto written_later = [&](size_t i, const std::vector<Span>& rd) {
        for (size_t j = i + 1; j < ps.size(); j++) {
            std::vector<Span> wj;
            if (ps[j].kind == 1) cols_spans(ps[j].cols, &wj);
            else wj.push_back(span_of(ps[j].out, ps[j].cap));
            if (overlaps(rd, wj)) return true;
        }
        return false;
    };
    for (size_t i = 0; i < ps.size(); i++) {
        auto& p = ps[i];
        c->hst[p.slot] = hs[i];
        NetidxError e{nullptr};
        bool r;
        if (p.kind == 1) {
            NxgStatus s;
            bool redone = false;
            // The common case: nothing was rewritten out of order so far and this call's kernel
            // did not decline, so the call is neither stale nor read again, and no fallback can
            // rewrite its columns (every one of finish_decode's needs fast_fail): its spans are
            // not needed.
            const bool plain = dirty.empty() && !hs[i].fast_fail;
            std::vector<Span> w, fr;
            if (!plain) {
                cols_spans(p.cols, &w);
                fr.push_back(span_of(p.frame, p.len));
            }
            const bool stale = !dirty.empty() && (overlaps(dirty, w) || overlaps(dirty, fr));
            const bool reread = stale || (hs[i].fast_fail && p.fast);
            if (reread && p.len > 0 && !covered(dirty, fr) && written_later(i, fr)) {
                if (ok) {
                    ok = false;
                    set_err(err, "decode of async call %zu needs its frame again (%s), "
                                 "but a later call in the backlog wrote into that frame "
                                 "buffer; keep a frame unchanged until nxg_ctx_sync",
                            i, stale ? "redone after an earlier call's fallback" : "fallback");
                }
                continue;
            }
            if (stale) {
                r = redo_decode(c, p, &s, &e);
                redone = true;
            } else {
                r = finish_decode(c, p.frame, p.len, p.cols, p.fast, p.st, p.slot, &s, &e, true,
                                  &redone);
            }
            if (redone) {
                if (plain) cols_spans(p.cols, &w);
                dirty.insert(dirty.end(), w.begin(), w.end());
            }
            if (r) {
                p.cols->layout =
                    (!mixed_capable(p.cols) || s.path == 1) ? NXG_LAYOUT_F64 : NXG_LAYOUT_MIXED;
                if (ust && !reported) *ust = s;
                if (s.err_kind) reported = true;
            }
        } else {
            NxgColumns dummy{};
            dummy.layout = NXG_LAYOUT_F64;
            const NxgColumns* in = p.cols ? p.cols : &dummy;
            std::vector<Span> rd;
            cols_spans(in, &rd);
            const Span wr = span_of(p.out, p.cap);
            // (its output too: an earlier encode's fallback into the same buffer put that
            // encode's frame back over this one's)
            const bool stale = !dirty.empty() && (overlaps(dirty, rd) || overlaps(dirty, {wr}));
            const bool reread = stale || (p.fast && hs[i].fast_fail);
            if (reread && !covered(dirty, rd) && written_later(i, rd)) {
                r = false;
                set_err(&e, "encode of async call %zu needs its columns again (%s), but a "
                            "later call in the backlog wrote into them; keep them unchanged until "
                            "nxg_ctx_sync", i,
                        stale ? "redone after an earlier call's fallback" : "fallback");
            } else if (stale) {
                r = redo_encode(c, p, in, &e);
                dirty.push_back(wr);
            } else {
                bool redone = false;
                r = finish_encode(c, in, p.st, p.slot, p.len_out, p.cap, true, &e, true, p.fast,
                                  p.heap, p.out, &redone);
                if (redone) dirty.push_back(wr);
            }
        }
        if (!r && ok) {
            ok = false;
            set_err(err, "%s", e.msg ? e.msg : "async call failed");
        }
        nxg_error_free(&e);
    }
    return ok;
}

// Grows the device staging of a host-resident NxgWriteCols to `rows` rows.
// (at least one row: a decode into columns of capacity 0 still hands the kernels staged arrays,
// which they refuse when null; growing for a need of 0 would leave an empty buffer empty)
static bool ensure_dwcols(NxgCtx* c, uint64_t rows, NetidxError* err) {
    rows = std::max<uint64_t>(rows, 1);
    return grow(c, c->dwflags, rows, kGrowWriteCols, err) &&
           grow(c, c->dwid, rows, kGrowWriteCols, err);
}

// win: the rows are To::Write messages (nxg_encode_writes), else From::Update
static bool encode_impl(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                        uint64_t cap, uint64_t* len_out, NetidxError* err,
                        const NxgWriteCols* win = nullptr) {
    if (!c || !in) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    const bool host = in->mem == NXG_MEM_HOST || !is_device_ptr(in->id);
    const NxgColumns* din = in;
    NxgColumns view;
    NxgWriteCols wview{};
    const NxgWriteCols* dwin = win;
    if (win && host && in->n_rows) {
        if (!ensure_dwcols(c, in->n_rows, err)) return false;
        HIPCHK(hipMemcpyAsync(c->dwflags, win->wflags, in->n_rows, hipMemcpyHostToDevice,
                              c->stream));
        HIPCHK(hipMemcpyAsync(c->dwid, win->wid, in->n_rows * 8, hipMemcpyHostToDevice,
                              c->stream));
        wview = *win;
        wview.mem = NXG_MEM_DEVICE;
        wview.wflags = c->dwflags;
        wview.wid = c->dwid;
        dwin = &wview;
    }
    const uint8_t* dheap = heap;
    uint8_t* dout = out;
    uint64_t heap_len = 0;
    if (host) {
        if (!ensure_dcols(c, in, err)) return false;
        view = staged_view(c, in);
        if (!copy_cols_h2d(c, in, &view, err)) return false;
        din = &view;
        // the heap extent: everything referenced by offsets; callers pass the frame/heap whose
        // length is not part of the ABI, so stage the maximum referenced byte
        if (heap && in->layout == NXG_LAYOUT_MIXED) {
            uint64_t hi = 0;
            auto upd = [&](uint8_t t, uint64_t f, uint32_t a) {
                if (t == 12 || t == 13 || t == 18 || t == 27) hi = std::max<uint64_t>(hi, f + a);
                if (t == 20) hi = std::max<uint64_t>(hi, f + 16);
            };
            for (uint64_t i = 0; i < in->n_rows; i++) upd(in->tag[i], in->fixed[i], in->aux[i]);
            for (uint64_t i = 0; i < in->n_children; i++)
                upd(in->ctag[i], in->cfixed[i], in->caux[i]);
            for (uint64_t i = 0; i < in->n_ctl; i++)
                hi = std::max<uint64_t>(hi, in->ctl_off[i] + in->ctl_len[i]);
            heap_len = hi;
            if (!grow(c, c->dheap, heap_len + 16, kGrowFrame, err)) return false;
            if (heap_len)
                HIPCHK(hipMemcpyAsync(c->dheap, heap, heap_len, hipMemcpyHostToDevice, c->stream));
            dheap = c->dheap;
        }
        dout = nullptr;
    }
    DevStatus* st;
    uint32_t slot;
    uint64_t total = 0;
    // pass 1 (sizing) when writing to a host buffer; a device buffer is written directly. A
    // write batch is also sized first when its buffer could take more than MAX_BATCH bytes, so
    // that such a batch is refused before anything is written (a smaller buffer bounds the
    // writes itself, and the call fails below).
    const bool size_first = win && out && cap > kMaxBatch;
    if ((host && out) || size_first) {
        if (!begin_call(c, &st, &slot, err)) return false;
        int fast = 0;
        const bool ok = enqueue_encode(c, din, dheap, nullptr, 0, st, err, &fast, true, dwin);
        if (!end_call(c, err) || !ok) return false;
        if (!finish_encode(c, din, st, slot, &total, 0, false, err, false, fast, dheap, nullptr))
            return false;
        if (win && total > kMaxBatch) {
            set_err(err, "write batch of %llu bytes exceeds MAX_BATCH (%llu): split the rows",
                    (unsigned long long)total, (unsigned long long)kMaxBatch);
            return false;
        }
        if (total > cap) {
            set_err(err, "output buffer too small: need %llu bytes, have %llu",
                    (unsigned long long)total, (unsigned long long)cap);
            return false;
        }
        if (host && !grow(c, c->dframe, total + 16, kGrowFrame, err)) return false;
        if (host) dout = c->dframe;
        cap = total;
    }
    if (!begin_call(c, &st, &slot, err)) return false;
    int fast = 0;
    const bool ok = enqueue_encode(c, din, dheap, dout, out ? cap : 0, st, err, &fast, true, dwin);
    if (!end_call(c, err) || !ok) return false;
    if (!finish_encode(c, din, st, slot, &total, cap, dout != nullptr, err, false, fast, dheap,
                       dout))
        return false;
    if (win && total > kMaxBatch) {
        set_err(err, "write batch of %llu bytes exceeds MAX_BATCH (%llu): split the rows",
                (unsigned long long)total, (unsigned long long)kMaxBatch);
        return false;
    }
    if (host && out && total) {
        HIPCHK(hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (len_out) *len_out = total;
    return true;
}

// ---- archive batches (netidx-archive logfile/mod.rs:150-205) ---------------------------------
// <Vec<BatchItem> as Pack>::encode (pack.rs:941-952): the count varint here, the items by the
// general encoder's rows kernel in archive mode
bool nxg_encode_archive_batch(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                              uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!c || !in) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (in->mem != NXG_MEM_DEVICE || !mixed_capable(in) || in->n_ctl ||
        (in->n_rows && (!in->id || !is_device_ptr(in->id)))) {
        set_err(err, "archive batches encode from device MIXED-layout columns without control "
                     "messages");
        return false;
    }
    if (in->n_rows > kMaxVecBytes / kBatchItemSize) {  // Vec::encode's guard (pack.rs:943-945)
        set_err(err, "encode failed: %llu items exceed MAX_VEC (PackError::TooBig)",
                (unsigned long long)in->n_rows);
        return false;
    }
    if (!set_device(c, err)) return false;
    uint8_t hdr[10];
    uint32_t hl = 0;
    for (uint64_t v = in->n_rows;; v >>= 7) {
        if (v < 0x80) {
            hdr[hl++] = (uint8_t)v;
            break;
        }
        hdr[hl++] = (uint8_t)((v & 0x7f) | 0x80);
    }
    if (out && cap < hl) {
        set_err(err, "output buffer too small: need at least %u bytes", hl);
        return false;
    }
    if (out) HIPCHK(hipMemcpyAsync(out, hdr, hl, hipMemcpyHostToDevice, c->stream));
    const uint64_t nt = nxg_enc_general_tiles(in->n_rows);
    if (!ensure_tstat(c, nt, err) || !ensure_escratch(c, 1, err)) return false;
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    const hipError_t le = nxg_launch_enc_general(desc_of(in), heap, out, out ? cap : 0, c->escratch,
                                                 c->tstat, c->epoch, st, c->grid_enc_gen,
                                                 c->stream, hl);
    if (!end_call(c, err)) return false;
    HIPCHK(le);
    uint64_t total = 0;
    if (!finish_encode(c, in, st, slot, &total, cap, out != nullptr, err)) return false;
    if (in->n_rows == 0) total = hl;
    if (len_out) *len_out = total;
    return true;
}

struct NxgZstdDict {
    int device;
    void* ddev = nullptr;       // NxzDictDev
    uint8_t* content = nullptr;  // the dictionary's content (history before every frame)
    // encode side (nxg_archive_compress): the Huffman codes of the dictionary's weights, built
    // with the dictionary; the content's hash table and the device copy, built at first use
    uint32_t content_len = 0;
    std::vector<uint8_t> enc_host;  // NxzEncDict
    void* denc = nullptr;
    uint32_t* dtable = nullptr;
    std::mutex enc_mu;
};

NxgZstdDict* nxg_zstd_dict_new(NxgCtx* c, const uint8_t* dict, uint64_t len, NetidxError* err) {
    if (!c || (!dict && len)) {
        set_err(err, "null argument");
        return nullptr;
    }
    if (!set_device(c, err)) return nullptr;
    std::vector<uint8_t> host(nxg_zstd_dict_dev_bytes());
    NxzDictDev* hd = reinterpret_cast<NxzDictDev*>(host.data());
    uint64_t coff = 0;
    if (!nxg_zstd_build_dict(dict, len, hd, &coff)) {
        set_err(err, "not a valid zstd dictionary");
        return nullptr;
    }
    NxgZstdDict* d = new NxgZstdDict();
    d->device = c->device;
    const uint64_t clen = len - coff;
    d->content_len = (uint32_t)clen;
    d->enc_host.resize(nxg_zstd_enc_dict_bytes());
    if (!nxg_zstd_build_enc_dict(dict, len, reinterpret_cast<NxzEncDict*>(d->enc_host.data()))) {
        set_err(err, "not a valid zstd dictionary");
        delete d;
        return nullptr;
    }
    auto fail = [&](hipError_t e) -> NxgZstdDict* {
        set_err(err, "zstd dictionary upload: %s", hipGetErrorString(e));
        nxg_zstd_dict_free(d);
        return nullptr;
    };
    hipError_t e;
    if ((e = hipMalloc(&d->content, std::max<uint64_t>(clen, 1))) != hipSuccess) return fail(e);
    if (clen && (e = hipMemcpy(d->content, dict + coff, clen, hipMemcpyHostToDevice)) != hipSuccess)
        return fail(e);
    nxg_zstd_set_content(hd, d->content);
    if ((e = hipMalloc(&d->ddev, host.size())) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(d->ddev, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return fail(e);
    return d;
}

void nxg_zstd_dict_free(NxgZstdDict* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->ddev) (void)hipFree(d->ddev);
    if (d->content) (void)hipFree(d->content);
    if (d->denc) (void)hipFree(d->denc);
    if (d->dtable) (void)hipFree(d->dtable);
    delete d;
}

bool nxg_archive_decompress(NxgCtx* c, const NxgZstdDict* dict, const uint8_t* src,
                            uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                            uint8_t* dout, uint64_t cap, uint64_t* need, NetidxError* err) {
    if (!c || (n && (!recs || !src))) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (is_device_ptr(src)) {
        set_err(err, "the records must be in host memory (the archive's mmap)");
        return false;
    }
    // the records' headers on the host (reader.rs:453-466): the uncompressed length sizes each
    // output slot, the index is skipped
    struct Rec {
        uint64_t frame_off, frame_len, out_off, out_cap;
    };
    std::vector<Rec> rd(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        NxgArchiveRecord& r = recs[i];
        r.out_len = 0;
        r.err = 0;
        r.out_off = total;
        Rec& x = rd[i];
        x = Rec{0, 0, total, 0};
        if (r.off > src_len || r.len > src_len - r.off || r.len < 4) {
            r.err = 7;
            continue;
        }
        const uint8_t* p = src + r.off;
        const uint64_t uncomp = ((uint64_t)p[0] << 24) | ((uint64_t)p[1] << 16) |
                                ((uint64_t)p[2] << 8) | p[3];
        uint64_t pos = 4;
        if (indexed) {  // decode_varint (pack.rs:504-520): the index's length, prefix included
            uint64_t v = 0;
            uint32_t k = 0;
            bool ok = false;
            for (; k < 10 && pos + k < r.len; k++) {
                v |= (uint64_t)(p[pos + k] & 0x7f) << (7 * k);
                if (p[pos + k] < 0x80) {
                    ok = true;
                    break;
                }
            }
            if (!ok || v > r.len - pos) {
                r.err = 7;
                continue;
            }
            pos += v;
        }
        x.frame_off = r.off + pos;
        x.frame_len = r.len - pos;
        x.out_cap = uncomp;
        total += uncomp;
    }
    if (need) *need = total;
    if (!dout) return true;
    if (total > cap) {
        set_err(err, "output buffer too small: the records need %llu bytes, capacity %llu",
                (unsigned long long)total, (unsigned long long)cap);
        return false;
    }
    if (n == 0) return true;
    if (!set_device(c, err)) return false;
    if (!c->zdefs) {
        std::vector<uint8_t> h(nxg_zstd_defaults_bytes());
        if (!nxg_zstd_build_defaults(reinterpret_cast<NxzDefaults*>(h.data()))) {
            set_err(err, "predefined zstd tables");
            return false;
        }
        HIPCHK(hipMalloc(&c->zdefs, h.size()));
        HIPCHK(hipMemcpy(c->zdefs, h.data(), h.size(), hipMemcpyHostToDevice));
        c->zgrid = nxg_zstd_grid(c->ncu);
        HIPCHK(hipMalloc(&c->zlit, (size_t)c->zgrid * nxg_zstd_litbuf_bytes()));
    }
    const size_t rb = nxg_zstd_rec_bytes(), sb = nxg_zstd_res_bytes();
    static_assert(sizeof(Rec) == 32, "NxzRec layout");
    if (!grow(c, c->zrecs, (size_t)n * (rb + sb), kGrowZstdRecs, err)) return false;
    uint8_t* drecs = c->zrecs;
    uint8_t* dres = drecs + (size_t)n * rb;
    const uint8_t* dsrc;
    if (!frame_to_device(c, src, src_len, &dsrc, err)) return false;
    HIPCHK(hipMemcpyAsync(drecs, rd.data(), (size_t)n * rb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dres, 0, (size_t)n * sb, c->stream));
    HIPCHK(nxg_launch_zstd(dsrc, drecs, n, dict ? dict->ddev : nullptr, c->zdefs, dout, c->zlit,
                           dres, c->zgrid, c->stream));
    struct Res {
        uint64_t out_len;
        uint32_t err, pad;
    };
    std::vector<Res> hr(n);
    HIPCHK(hipMemcpyAsync(hr.data(), dres, (size_t)n * sb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; i++) {
        if (recs[i].err) continue;  // rejected on the host
        recs[i].out_len = hr[i].out_len;
        recs[i].err = hr[i].err;
        if (recs[i].err) recs[i].out_len = 0;
    }
    return true;
}

// the dictionary's encode-side device state, at the first compression with it
static bool zstd_dict_enc_ready(NxgCtx* c, NxgZstdDict* d, NetidxError* err) {
    std::lock_guard<std::mutex> g(d->enc_mu);
    if (d->denc) return true;
    if (d->device != c->device) {
        set_err(err, "the dictionary belongs to another device");
        return false;
    }
    void* tab = nullptr;
    void* enc = nullptr;
    auto fail = [&](hipError_t e) {
        set_err(err, "zstd dictionary hash table: %s", hipGetErrorString(e));
        if (tab) (void)hipFree(tab);
        if (enc) (void)hipFree(enc);
        return false;
    };
    hipError_t e;
    if ((e = hipMalloc(&tab, nxg_zstd_dict_table_bytes())) != hipSuccess) return fail(e);
    if ((e = nxg_launch_zstd_dict_hash(d->content, d->content_len, static_cast<uint32_t*>(tab),
                                       c->stream)) != hipSuccess)
        return fail(e);
    nxg_zstd_enc_dict_set(reinterpret_cast<NxzEncDict*>(d->enc_host.data()), d->content,
                          d->content_len, static_cast<uint32_t*>(tab));
    if ((e = hipMalloc(&enc, d->enc_host.size())) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(enc, d->enc_host.data(), d->enc_host.size(), hipMemcpyHostToDevice,
                            c->stream)) != hipSuccess)
        return fail(e);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(e);
    d->dtable = static_cast<uint32_t*>(tab);
    d->denc = enc;
    return true;
}

bool nxg_archive_compress(NxgCtx* c, const NxgZstdDict* dict, const uint8_t* src,
                          uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                          uint8_t* out, uint64_t cap, uint64_t* need, NetidxError* err) {
    return nxg_archive_compress_opts(c, dict, src, src_len, recs, n, indexed, nullptr, out, cap,
                                     need, err);
}

bool nxg_archive_compress_opts(NxgCtx* c, const NxgZstdDict* dict, const uint8_t* src,
                               uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                               const NxgZstdCompressOpts* opts, uint8_t* out, uint64_t cap,
                               uint64_t* need, NetidxError* err) {
    if (!c || (n && (!recs || !src))) {
        set_err(err, "null argument");
        return false;
    }
    const uint32_t literals = opts ? opts->literals : (uint32_t)NXG_ZSTD_LIT_DICT_TREE;
    if (literals > NXG_ZSTD_LIT_BLOCK_TREES) {
        set_err(err, "NxgZstdCompressOpts.literals: unknown value %u", literals);
        return false;
    }
    if (opts && (opts->reserved[0] | opts->reserved[1] | opts->reserved[2])) {
        set_err(err, "NxgZstdCompressOpts.reserved must be zero");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (is_device_ptr(src) || (out && is_device_ptr(out))) {
        set_err(err, "the records and the output must be in host memory");
        return false;
    }
    // the index prefixes and the slots on the host (compress_task, reader.rs:741-769: the index
    // is copied, the rest is the batch)
    struct Rec {
        uint64_t src_off, src_len, out_off, out_cap;
    };
    struct Res {
        uint64_t out_len;
        uint32_t err, pad;
    };
    std::vector<Rec> rd(n);
    std::vector<uint64_t> ilen(n, 0);
    uint64_t total = 0, dtotal = 0, lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        NxgArchiveRecord& r = recs[i];
        r.out_len = 0;
        r.err = 0;
        r.out_off = total;
        rd[i] = Rec{0, 0, dtotal, 0};
        if (r.off > src_len || r.len > src_len - r.off) {
            set_err(err, "record %u lies outside the source", i);
            return false;
        }
        if (r.len >= (1ull << 32)) {
            set_err(err, "record %u has 2^32 bytes or more", i);
            return false;
        }
        uint64_t pos = 0;
        if (indexed) {  // decode_varint (pack.rs:504-520): the index's length, prefix included
            const uint8_t* p = src + r.off;
            uint64_t v = 0;
            bool ok = false;
            for (uint32_t k = 0; k < 10 && k < r.len; k++) {
                v |= (uint64_t)(p[k] & 0x7f) << (7 * k);
                if (p[k] < 0x80) {
                    ok = true;
                    break;
                }
            }
            if (!ok || v > r.len) {
                r.err = 7;
                continue;
            }
            pos = v;
        }
        ilen[i] = pos;
        const uint64_t blen = r.len - pos, fb = nxg_zstd_frame_bound(blen);
        rd[i] = Rec{r.off + pos, blen, dtotal, fb};
        lo = std::min(lo, r.off + pos);
        hi = std::max(hi, r.off + r.len);
        dtotal += fb;
        total += 4 + pos + fb;
    }
    if (need) *need = total;
    if (!out) return true;
    if (total > cap) {
        set_err(err, "output buffer too small: the records need %llu bytes, capacity %llu",
                (unsigned long long)total, (unsigned long long)cap);
        return false;
    }
    if (n == 0 || dtotal == 0) return true;
    if (!set_device(c, err)) return false;
    if (dict && !zstd_dict_enc_ready(c, const_cast<NxgZstdDict*>(dict), err)) return false;
    if (!c->zc_tables) {
        std::vector<uint8_t> h(nxg_zstd_enc_tables_bytes());
        if (!nxg_zstd_build_enc_tables(h.data())) {
            set_err(err, "predefined zstd encoding tables");
            return false;
        }
        void* t = nullptr;
        HIPCHK(hipMalloc(&t, h.size()));
        if (hipMemcpy(t, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(t);
            set_err(err, "predefined zstd encoding tables: upload");
            return false;
        }
        c->zc_tables = t;
    }
    if (!c->zc_ev[1]) {
        HIPCHK(hipEventCreate(&c->zc_ev[0]));
        HIPCHK(hipEventCreate(&c->zc_ev[1]));
    }
    if (!c->zc_slab) {
        c->zc_grid = nxg_zstd_enc_grid(c->ncu);
        HIPCHK(hipMalloc(&c->zc_slab, (size_t)c->zc_grid * nxg_zstd_enc_slab_bytes()));
    }
    const size_t rb = nxg_zstd_enc_rec_bytes(), sb = nxg_zstd_enc_res_bytes();
    static_assert(sizeof(Rec) == 32 && sizeof(Res) == 16, "NxzEncRec / NxzEncRes layout");
    if (!grow(c, c->zc_recs, (size_t)n * (rb + sb + 8 + 4) + 8, kGrowZstdEnc, err)) return false;
    if (!grow(c, c->zc_out, dtotal, kGrowZstdEnc, err)) return false;
    uint8_t* drecs = c->zc_recs;
    uint8_t* dres = drecs + (size_t)n * rb;
    uint64_t* dpk = reinterpret_cast<uint64_t*>(dres + (size_t)n * sb);
    uint32_t* dticket = reinterpret_cast<uint32_t*>(dpk + n);
    uint32_t* dorder = dticket + 2;
    // the order the waves draw records in: longest first
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return rd[a].src_len > rd[b].src_len; });
    // the batches to the device in one copy: the span of the source that holds them
    if (lo > hi) lo = hi = 0;
    for (uint32_t i = 0; i < n; i++)
        if (rd[i].out_cap) rd[i].src_off -= lo;
    const uint8_t* dsrc;
    if (!frame_to_device(c, src + lo, hi - lo, &dsrc, err)) return false;
    HIPCHK(hipMemcpyAsync(drecs, rd.data(), (size_t)n * rb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dres, 0, (size_t)n * sb, c->stream));
    HIPCHK(hipMemsetAsync(dticket, 0, 8, c->stream));
    HIPCHK(hipMemcpyAsync(dorder, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->zc_ev[0], c->stream));
    HIPCHK(nxg_launch_zstd_enc(dsrc, drecs, n, dict ? dict->denc : nullptr, c->zc_tables, c->zc_out,
                               c->zc_slab, dres, dorder, dticket, c->zc_grid, literals,
                               c->stream));
    HIPCHK(hipEventRecord(c->zc_ev[1], c->stream));
    std::vector<Res> hr(n);
    HIPCHK(hipMemcpyAsync(hr.data(), dres, (size_t)n * sb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&c->zc_kernel_ms, c->zc_ev[0], c->zc_ev[1]);
    // only the bytes written come back: the frames packed on the device, one copy, then each
    // to its slot behind the record length and the index
    std::vector<uint64_t> pk(n);
    uint64_t packed = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rd[i].out_cap && (hr[i].out_len == 0 || hr[i].out_len > rd[i].out_cap)) {
            set_err(err, "record %u: the compressor reported %llu bytes for a slot of %llu", i,
                    (unsigned long long)hr[i].out_len, (unsigned long long)rd[i].out_cap);
            return false;
        }
        pk[i] = packed;
        packed += hr[i].out_len;
    }
    if (!grow(c, c->zc_pack, packed, kGrowZstdEnc, err)) return false;
    if (!grow(c, c->zc_hpin, packed, kGrowZstdEnc, err)) return false;
    uint8_t* hp = c->zc_hpin;
    HIPCHK(hipMemcpyAsync(dpk, pk.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(nxg_launch_zstd_pack(c->zc_out, drecs, dres, dpk, n, c->zc_pack, c->ncu, c->stream));
    HIPCHK(hipMemcpyAsync(hp, c->zc_pack, packed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; i++) {
        NxgArchiveRecord& r = recs[i];
        if (r.err) continue;
        uint8_t* o = out + r.out_off;
        o[0] = (uint8_t)(r.len >> 24);
        o[1] = (uint8_t)(r.len >> 16);
        o[2] = (uint8_t)(r.len >> 8);
        o[3] = (uint8_t)r.len;
        memcpy(o + 4, src + r.off, ilen[i]);
        memcpy(o + 4 + ilen[i], hp + pk[i], hr[i].out_len);
        r.out_len = 4 + ilen[i] + hr[i].out_len;
    }
    return true;
}

// diagnostics, not ABI: the compressor kernel's time in the last nxg_archive_compress (ms)
extern "C" double nxg_debug_zstd_compress_kernel_ms(NxgCtx* c) { return c ? c->zc_kernel_ms : 0.0; }

// the fast archive decoder's device results (nxg_archive_fast.hip FaHead)
struct FaHeadHost {
    uint32_t fast_fail, arrived;
    uint64_t end, end_children, items, ticket, recounts, why, why_tile;
};
static_assert(sizeof(FaHeadHost) == 64 && sizeof(FaHeadHost) <= sizeof(DevStatus), "FaHead");

// The batch header on the host: the count varint (decode_varint, pack.rs:504-520: at most 10
// bytes, bits past 64 dropped) and its length; false when it is not a complete varint (the exact
// decoder reports that) or check_sz! would refuse it (pack.rs:919-925)
static bool arch_header(NxgCtx* c, const uint8_t* buf, uint64_t len, uint64_t* count, uint32_t* p0,
                        NetidxError* err) {
    uint8_t h[10] = {0};
    const uint64_t n = std::min<uint64_t>(len, 10);
    if (n == 0) return false;
    if (is_device_ptr(buf)) {
        if (hipMemcpyAsync(h, buf, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return false;
    } else {
        memcpy(h, buf, n);
    }
    (void)err;
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t b = h[i];
        v |= i < 9 ? (b & 0x7f) << (7 * i) : (b & 1) << 63;
        if (b < 0x80) {
            *count = v;
            *p0 = i + 1;
            const uint64_t sz = v > ~0ull / 24 ? ~0ull : v * 24;  // size_of::<BatchItem>()
            return sz <= kMaxVecBytes && sz <= ((len - (i + 1)) << 8);
        }
    }
    return false;
}

bool nxg_decode_archive_batch(NxgCtx* c, const uint8_t* buf, uint64_t len, NxgColumns* out,
                              NxgStatus* ust, uint64_t* consumed, NetidxError* err) {
    if (!c || !out || (!buf && len)) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (len >= (1ull << 40)) {
        set_err(err, "batch too large (%llu bytes)", (unsigned long long)len);
        return false;
    }
    if (out->mem != NXG_MEM_DEVICE || !mixed_capable(out) || !out->id) {
        set_err(err, "archive batches decode into device MIXED-layout columns");
        return false;
    }
    if (!set_device(c, err)) return false;
    const uint8_t* df;
    // the fast path (nxg_archive_fast.hip) over a window of the buffer that grows until the batch
    // fits; anything it declines goes to the exact decoder below over the whole buffer
    uint64_t count = 0;
    uint32_t p0 = 0;
    if (!c->no_fa && arch_header(c, buf, len, &count, &p0, err) && count >= 1 &&
        count <= out->cap_rows && count < (1ull << 31) && out->tag && out->ctag) {
        const uint64_t wmax = std::min<uint64_t>(len, 0xfff00000ull);
        uint64_t W = std::min<uint64_t>(wmax, p0 + count * 24 + 65536);
        FaHeadHost* hh = reinterpret_cast<FaHeadHost*>(c->hst + kStatusRing);
#pragma unroll 1
        for (;;) {
            if (!frame_to_device(c, buf, W, &df, err)) return false;
            const size_t need = nxg_fa_scratch_bytes(W);
            if (!ensure_dscratch(c, need, err)) return false;
            HIPCHK(nxg_launch_dec_fa(df, W, p0, count, desc_of(out), c->dscratch, hh, nullptr,
                                     c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            memcpy(c->fa_last, hh, sizeof c->fa_last);
            if (!hh->fast_fail && hh->end) {
                NxgStatus s{};
                s.n_rows = count;
                s.n_children = hh->end_children;
                s.path = NXG_PATH_ARCHIVE_FAST;
                out->n_rows = count;
                out->n_children = hh->end_children;
                out->n_ctl = 0;
                out->layout = NXG_LAYOUT_MIXED;
                if (ust) *ust = s;
                if (consumed) *consumed = hh->end - 1;
                return true;
            }
            // a larger window helps only a chain that ran out of window (decline reasons 1 and
            // 2: a broken or mismatched chain); a decode error or a declined value goes straight
            // to the exact decoder
            if (W >= wmax || (hh->why & ~3ull)) break;
            W = std::min(wmax, 2 * W);
        }
    }
    if (!frame_to_device(c, buf, len, &df, err)) return false;
    const size_t need = 64 + nxg_arch_scratch_bytes(len);
    if (!ensure_dscratch(c, need, err)) return false;
    uint32_t* cap_flag = reinterpret_cast<uint32_t*>(c->dscratch.get());
    HIPCHK(hipMemsetAsync(cap_flag, 0, 4, c->stream));
    NxgArchResult r{};
    HIPCHK(nxg_arch_decode(df, len, desc_of(out), c->dscratch + 64, cap_flag, 8, &r, c->stream));
    NxgStatus s{};
    s.n_rows = r.n_rows;
    s.n_children = r.n_children;
    s.err_kind = (int32_t)r.err_kind;
    s.err_offset = r.err_offset;
    s.path = NXG_PATH_ARCHIVE;
    out->n_rows = r.n_rows;
    out->n_children = r.n_children;
    out->n_ctl = 0;
    out->layout = NXG_LAYOUT_MIXED;
    if (ust) *ust = s;
    if (consumed) *consumed = r.consumed;
    return true;
}

// ---- a window of archive records and its image (nxg_archive_window.hip) -----------------------
namespace {
bool ensure_aw(NxgCtx* c, size_t dev_bytes, size_t host_bytes, NetidxError* err) {
    return grow(c, c->aw_dev, dev_bytes, kGrowDouble, err) &&
           grow(c, c->aw_host, host_bytes, kGrowDouble, err);
}

// the ctx's scratch columns for one record of `len` bytes on the single-batch decoder (rows <=
// len / 2, children <= len)
bool ensure_aw_cols(NxgCtx* c, uint64_t len, NetidxError* err) {
    const uint64_t cr = len / 2 + 1, cc = len + 1;
    if (c->dcols_valid && c->dcols.layout == NXG_LAYOUT_MIXED && c->dcols.cap_rows >= cr &&
        c->dcols.cap_children >= cc)
        return true;
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t ck = c->dcols_valid ? std::max<uint64_t>(c->dcols.cap_ctl, 1) : 1;
    if (c->dcols_valid) cols_free_impl(&c->dcols);
    c->dcols_valid = false;
    if (!cols_alloc_impl(NXG_LAYOUT_MIXED, cr, cc, ck, NXG_MEM_DEVICE, &c->dcols, err)) return false;
    c->dcols_valid = true;
    return true;
}
}  // namespace

bool nxg_archive_decode_window(NxgCtx* c, const uint8_t* dbuf, uint64_t buf_len,
                               const NxgArchiveRecord* recs, uint32_t n,
                               const NxgArchiveWindowOpts* opts, NxgColumns* out,
                               NxgArchiveBatchInfo* info, uint64_t* need_rows,
                               uint64_t* need_children, NetidxError* err) {
    // (the arguments first, the ctx after them: misuse is reported before any device work)
    if (!out || !need_rows || !need_children || (n && (!recs || !info)) || (!dbuf && buf_len)) {
        set_err(err, "null argument");
        return false;
    }
    if (out->mem != NXG_MEM_DEVICE || !mixed_capable(out) || !out->id || !out->fixed) {
        set_err(err, "a window of archive records decodes into device MIXED-layout columns");
        return false;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (recs[i].err) continue;
        if (recs[i].out_off > buf_len || recs[i].out_len > buf_len - recs[i].out_off) {
            set_err(err, "record %u (offset %llu, %llu bytes) lies outside the buffer of %llu bytes",
                    i, (unsigned long long)recs[i].out_off, (unsigned long long)recs[i].out_len,
                    (unsigned long long)buf_len);
            return false;
        }
        if (recs[i].out_len >= (1ull << 40)) {
            set_err(err, "record %u too large (%llu bytes)", i, (unsigned long long)recs[i].out_len);
            return false;
        }
    }
    if (!c) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if (buf_len && !is_device_ptr(dbuf)) {
        set_err(err, "the window's buffer must be device memory");
        return false;
    }
    uint64_t big = opts && opts->big_record_bytes ? opts->big_record_bytes
                                                  : (uint64_t)NXG_ARCHIVE_WINDOW_BIG_DEFAULT;
    big = std::min<uint64_t>(big, 0x7fffffffull);  // the wave kernels use 32-bit record offsets
    *need_rows = *need_children = 0;
    out->n_rows = out->n_children = out->n_ctl = out->n_heartbeat = 0;
    out->layout = NXG_LAYOUT_MIXED;
    if (n == 0) return true;
    const size_t bytes = sizeof(AwHead) + (size_t)n * sizeof(AwRec);
    if (!ensure_aw(c, bytes, bytes, err)) return false;
    AwHead* hh = reinterpret_cast<AwHead*>(c->aw_host.get());
    AwRec* hr = reinterpret_cast<AwRec*>(c->aw_host + sizeof(AwHead));
    uint8_t* dhead = c->aw_dev;
    uint8_t* drecs = c->aw_dev + sizeof(AwHead);
    uint32_t n_wave = 0;
    for (uint32_t i = 0; i < n; i++) {
        AwRec r{};
        r.off = recs[i].out_off;
        r.len = recs[i].out_len;
        r.route = recs[i].err ? 0u : (r.len < big ? 1u : 2u);
        n_wave += r.route == 1u;
        hr[i] = r;
    }
    memset(hh, 0, sizeof *hh);
    HIPCHK(hipMemcpyAsync(c->aw_dev, c->aw_host, bytes, hipMemcpyHostToDevice, c->stream));
    if (n_wave) {
        HIPCHK(nxg_launch_aw_count(dbuf, drecs, n, c->ncu, c->stream));
        HIPCHK(hipMemcpyAsync(hr, drecs, (size_t)n * sizeof(AwRec), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    // the records of the single-batch decoder, in order: each into the scratch columns, then to
    // its place by the host's running sums (the device scan below gives the same offsets)
    uint64_t rows_run = 0, kids_run = 0;
    uint32_t n_emit = 0;
    bool patched = false;
    for (uint32_t i = 0; i < n; i++) {
        NxgArchiveBatchInfo f{};
        AwRec& r = hr[i];
        if (r.route == 1u && !r.declined) {
            f.path = NXG_PATH_ARCHIVE_WINDOW;
            n_emit++;
        } else if (r.route != 0u) {
            if (!ensure_aw_cols(c, r.len, err)) return false;
            NxgColumns sc = c->dcols;
            NxgStatus st{};
            uint64_t used = 0;
            if (!nxg_decode_archive_batch(c, dbuf + r.off, r.len, &sc, &st, &used, err))
                return false;
            f.err_kind = st.err_kind;
            f.err_offset = st.err_offset;
            f.path = st.path;
            r.rows = st.err_kind ? 0 : st.n_rows;
            r.kids = st.err_kind ? 0 : st.n_children;
            r.consumed = st.err_kind ? 0 : used;
            r.route = 2u;
            r.declined = 0u;
            patched = true;
            if (rows_run + r.rows <= out->cap_rows && kids_run + r.kids <= out->cap_children)
                HIPCHK(nxg_launch_aw_rebase(desc_of(&sc), desc_of(out), r.rows, r.kids, rows_run,
                                            kids_run, r.off, c->stream));
        }
        f.row_off = rows_run;
        f.n_rows = r.rows;
        f.child_off = kids_run;
        f.n_children = r.kids;
        f.consumed = r.consumed;
        info[i] = f;
        rows_run += r.rows;
        kids_run += r.kids;
    }
    *need_rows = rows_run;
    *need_children = kids_run;
    if (rows_run > out->cap_rows || kids_run > out->cap_children) {
        HIPCHK(hipStreamSynchronize(c->stream));
        set_err(err, "the window needs %llu rows and %llu children; the columns hold %llu and %llu",
                (unsigned long long)rows_run, (unsigned long long)kids_run,
                (unsigned long long)out->cap_rows, (unsigned long long)out->cap_children);
        return false;
    }
    if (n_emit) {
        if (patched)
            HIPCHK(hipMemcpyAsync(drecs, hr, (size_t)n * sizeof(AwRec), hipMemcpyHostToDevice,
                                  c->stream));
        HIPCHK(nxg_launch_aw_scan(drecs, n, dhead, c->stream));
        HIPCHK(nxg_launch_aw_emit(dbuf, drecs, n, desc_of(out), dhead, c->ncu, c->stream));
        HIPCHK(hipMemcpyAsync(c->aw_host, c->aw_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_emit) {
        bool same = hh->rows == rows_run && hh->kids == kids_run && !hh->emit_fail;
        for (uint32_t i = 0; same && i < n; i++)
            same = hr[i].row_off == info[i].row_off && hr[i].child_off == info[i].child_off;
        if (!same) {
            set_err(err, "internal error: the window's emit pass disagrees with its count pass");
            return false;
        }
    }
    out->n_rows = rows_run;
    out->n_children = kids_run;
    return true;
}

bool nxg_archive_build_image(NxgCtx* c, const NxgColumns* window, uint64_t n_ids,
                             const uint8_t* keep, NxgArchiveImage* out, NetidxError* err) {
    if (!window || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (window->mem != NXG_MEM_DEVICE || window->layout != NXG_LAYOUT_MIXED || !window->id ||
        !window->tag || !window->fixed || !window->aux) {
        set_err(err, "the image is built from device MIXED-layout columns");
        return false;
    }
    const uint64_t rows = window->n_rows;
    if (out->cap_rows < std::min(n_ids, rows)) {
        set_err(err, "the image's capacity is %llu rows; min(n_ids, window rows) = %llu",
                (unsigned long long)out->cap_rows, (unsigned long long)std::min(n_ids, rows));
        return false;
    }
    if (out->cap_rows && (!out->id || !out->tag || !out->fixed || !out->aux || !out->src_row)) {
        set_err(err, "null output array");
        return false;
    }
    if (!c) {
        set_err(err, "null argument");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if ((rows && !is_device_ptr(window->id)) || (out->cap_rows && !is_device_ptr(out->id)) ||
        (keep && !is_device_ptr(keep))) {
        set_err(err, "the image needs device columns, device outputs and a device keep array");
        return false;
    }
    out->n_rows = out->n_filtered = 0;
    if (!ensure_aw(c, sizeof(AwHead) + nxg_aw_image_scratch_bytes(n_ids), sizeof(AwHead), err))
        return false;
    HIPCHK(nxg_launch_aw_image(desc_of(window), rows, n_ids, keep, c->aw_dev + sizeof(AwHead),
                               out->cap_rows, out->id, out->tag, out->fixed, out->aux,
                               out->src_row, c->aw_dev, c->stream));
    AwHead* hh = reinterpret_cast<AwHead*>(c->aw_host.get());
    HIPCHK(hipMemcpyAsync(hh, c->aw_dev, sizeof(AwHead), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_ids == 0 && rows) hh->bad_row = 0;  // every Id is past an empty table
    if (hh->bad_row != ~0ull) {
        uint64_t v = 0;
        HIPCHK(hipMemcpy(&v, window->id + hh->bad_row, 8, hipMemcpyDeviceToHost));
        set_err(err, "Id %llu at row %llu is not below n_ids = %llu", (unsigned long long)v,
                (unsigned long long)hh->bad_row, (unsigned long long)n_ids);
        return false;
    }
    out->n_rows = hh->n_image;
    out->n_filtered = hh->n_filtered;
    return true;
}

// ---- type-partitioned view ------------------------------------------------------
bool nxg_partition_by_tag(NxgCtx* c, const NxgColumns* cols, NxgTagView* out, NetidxError* err) {
    if (!c || !cols || !out) {
        set_err(err, "null argument");
        return false;
    }
    const uint64_t n = cols->n_rows;
    if (cols->layout != NXG_LAYOUT_MIXED || !cols->tag || !cols->fixed || !cols->aux) {
        set_err(err, "the type-partitioned view needs mixed-layout columns (a tag column)");
        return false;
    }
    if (n && (!out->rank || !out->row_of || !out->fixed || !out->aux)) {
        set_err(err, "null output array");
        return false;
    }
    if (n > out->cap_rows || n > 0xffffffffull) {
        set_err(err, "%llu rows: the view's capacity is %llu (and rows must be < 2^32)",
                (unsigned long long)n, (unsigned long long)out->cap_rows);
        return false;
    }
    if (n && (!is_device_ptr(cols->tag) || !is_device_ptr(out->rank))) {
        set_err(err, "the type-partitioned view needs device columns and device outputs");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    const size_t need = nxg_part_scratch_bytes(n);
    if (!grow(c, c->pscratch, need, kGrowDouble, err)) return false;
    uint64_t* doff = nullptr;
    HIPCHK(nxg_launch_partition(cols->tag, cols->fixed, cols->aux, n, c->pscratch, out->rank,
                                out->row_of, out->fixed, out->aux, &doff, c->stream));
    HIPCHK(hipMemcpyAsync(out->off, doff, sizeof(uint64_t) * (NXG_TAG_BINS + 1),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int t = 0; t < NXG_TAG_BINS; t++) out->count[t] = out->off[t + 1] - out->off[t];
    out->n_rows = n;
    return true;
}

// ---- dispatch (connection.rs:546-567) --------------------------------------------------------
bool nxg_dispatch_updates(NxgCtx* c, const NxgSubTable* tab, const uint64_t* id, uint64_t n_rows,
                          NxgDispatch* out, NetidxError* err) {
    if (!c || !tab || !out || (n_rows && !id) || !out->chan_off) {
        set_err(err, "null argument");
        return false;
    }
    if ((tab->n_ids && !tab->slot_of_id) ||
        (tab->n_slots && (!tab->slot_sub_id || !tab->slot_stream_off || !tab->slot_has_last ||
                          !out->last_row)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row))) {
        set_err(err, "null table or output array");
        return false;
    }
    if (n_rows && tab->n_slots && !tab->stream_chan && tab->n_chans) {
        set_err(err, "null stream_chan");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t need = 64 + nxg_disp_scratch_bytes(n_rows, tab->n_chans);
    if (!ensure_dscratch(c, need, err)) return false;
    uint64_t* um = reinterpret_cast<uint64_t*>(c->dscratch.get());
    HIPCHK(nxg_launch_dispatch(*tab, id, n_rows, c->dscratch + 64, out->chan_off, out->ent_sub,
                               out->ent_row, out->cap_entries, out->last_row, um, c->ncu,
                               c->stream));
    uint64_t res[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&res[0], out->chan_off + tab->n_chans, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&res[1], um, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_entries = res[0];
    out->n_unmatched = res[1];
    if (res[0] > out->cap_entries) {
        set_err(err, "dispatch needs %llu entries, capacity is %llu", (unsigned long long)res[0],
                (unsigned long long)out->cap_entries);
        return false;
    }
    return true;
}

// ---- publisher commit (publisher/mod.rs:776-845) -----------------------------------------------
bool nxg_publish_commit(NxgCtx* c, const NxgPubTable* tab, const NxgColumns* batch,
                        const uint8_t* heap, const uint8_t* kind, const uint32_t* to_client,
                        NxgDispatch* out, NetidxError* err) {
    if (!c || !tab || !batch || !out || !out->chan_off) {
        set_err(err, "null argument");
        return false;
    }
    const uint64_t n = batch->n_rows;
    if (n && (!batch->id || !batch->fixed || !kind || !to_client)) {
        set_err(err, "null batch column, kind or to_client");
        return false;
    }
    if ((tab->n_ids && !tab->slot_of_id) ||
        (tab->n_slots && (!tab->slot_client_off || !tab->cur_fixed || !out->last_row)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row))) {
        set_err(err, "null table or output array");
        return false;
    }
    if (n >= 0xffffffffull) {
        set_err(err, "publish batches are limited to 2^32 - 1 rows");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t pub = (nxg_pub_scratch_bytes(n, tab->n_slots) + 255) & ~size_t(255);
    const size_t need = pub + 64 + nxg_disp_scratch_bytes(n, tab->n_clients);
    if (!ensure_dscratch(c, need, err)) return false;
    const NxgPubBatch b{batch->id,    batch->tag,   batch->fixed, batch->aux, batch->ctag,
                        batch->cfixed, batch->caux, heap,         kind,       n};
    HIPCHK(nxg_launch_pub_stage1(*tab, b, c->dscratch, c->ncu, c->stream));
    uint32_t flags[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(flags, nxg_pub_flags(c->dscratch), 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint8_t* mode = nullptr;
    HIPCHK(nxg_launch_pub_stage2(*tab, b, c->dscratch, flags[0] != 0, flags[1] != 0, c->ncu,
                                 c->stream, &mode));
    if (flags[1]) {
        uint32_t f23[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(f23, nxg_pub_flags(c->dscratch) + 2, 8, hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (f23[1]) {  // Decimal / container / Abstract comparisons: the stack-walk kernel
            const uint32_t* prev =
                flags[0] ? nxg_pub_prev(c->dscratch, n, tab->n_slots) : nullptr;
            HIPCHK(nxg_launch_pub_deep(*tab, b, c->dscratch, prev, c->ncu, c->stream));
            HIPCHK(hipMemcpyAsync(f23, nxg_pub_flags(c->dscratch) + 2, 4, hipMemcpyDeviceToHost,
                                  c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        flags[2] = f23[0];
        if (flags[2]) {
            set_err(err, "NXG_UNSUPPORTED: an UpdateChanged compares values nested deeper than "
                         "%d levels, or a container whose columns have no children",
                    NXG_MAX_DEPTH);
            return false;
        }
    } else {
        mode = kind;  // Update(None) = 0 and Update(Some(cl)) = 2 route as they are
    }
    // the client fan-out is the subscriber dispatch with per-row routing: clients as channels,
    // entries tagged with the row's Id, every slot tracking `current`
    const NxgSubTable st{tab->n_ids, tab->slot_of_id, tab->n_slots, nullptr, tab->slot_client_off,
                         tab->client, nullptr, tab->n_clients};
    uint8_t* ds = c->dscratch + pub;
    uint64_t* um = reinterpret_cast<uint64_t*>(ds);
    HIPCHK(nxg_launch_dispatch(st, batch->id, n, ds + 64, out->chan_off, out->ent_sub, out->ent_row,
                               out->cap_entries, out->last_row, um, c->ncu, c->stream, mode,
                               to_client));
    uint64_t res[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&res[0], out->chan_off + tab->n_clients, 8, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemcpyAsync(&res[1], um, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_entries = res[0];
    out->n_unmatched = res[1];
    if (res[0] > out->cap_entries) {
        set_err(err, "publish needs %llu entries, capacity is %llu", (unsigned long long)res[0],
                (unsigned long long)out->cap_entries);
        return false;
    }
    return true;
}

// the commit's unsubscribes (publisher/mod.rs:820-832): every pair routes to its client (row
// mode 2 of the dispatch), so each client's list keeps queue order
bool nxg_publish_unsubscribes(NxgCtx* c, const uint64_t* id, const uint32_t* client, uint64_t n,
                              uint32_t n_clients, NxgDispatch* out, NetidxError* err) {
    if (!c || !out || !out->chan_off || (n && (!id || !client)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row))) {
        set_err(err, "null argument");
        return false;
    }
    if (n >= 0xffffffffull) {
        set_err(err, "unsubscribe lists are limited to 2^32 - 1 pairs");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t mode_bytes = (n + 255) & ~uint64_t(255);
    const size_t need = mode_bytes + 64 + nxg_disp_scratch_bytes(n, n_clients);
    if (!ensure_dscratch(c, need, err)) return false;
    uint8_t* mode = c->dscratch;
    if (n) HIPCHK(hipMemsetAsync(mode, 2, n, c->stream));
    const NxgSubTable st{0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, n_clients};
    uint8_t* ds = c->dscratch + mode_bytes;
    uint64_t* um = reinterpret_cast<uint64_t*>(ds);
    HIPCHK(nxg_launch_dispatch(st, id, n, ds + 64, out->chan_off, out->ent_sub, out->ent_row,
                               out->cap_entries, nullptr, um, c->ncu, c->stream, mode, client));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, out->chan_off + n_clients, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_entries = total;
    out->n_unmatched = 0;
    if (total > out->cap_entries) {
        set_err(err, "unsubscribes need %llu entries, capacity is %llu", (unsigned long long)total,
                (unsigned long long)out->cap_entries);
        return false;
    }
    return true;
}

// ---- the commit's per-client batches, encoded (handle_updates -> queue_send per client) -------
// One gathered encode of the entry list (nxg_encode_clients.hip). pass(dout, cap) runs the tile
// kernel and reads the status and client_off back; a buffer that could take more than MAX_BATCH
// bytes is sized first, so that a client too long for one frame fails before anything is written.
bool nxg_encode_clients(NxgCtx* c, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_clients, NxgClientFrames* out,
                        NetidxError* err) {
    if (!c || !batch || !d || !out || !out->client_off || !d->chan_off) {
        set_err(err, "null argument");
        return false;
    }
    const uint64_t ne = d->n_entries;
    const bool f64 = batch->layout == NXG_LAYOUT_F64;
    if (batch->n_ctl) {
        set_err(err, "per-client batches encode from columns without control messages (n_ctl = "
                     "%llu)", (unsigned long long)batch->n_ctl);
        return false;
    }
    if (ne && (!d->ent_row || !batch->id || !batch->fixed ||
               (!f64 && (!batch->tag || !batch->aux)))) {
        set_err(err, "null entry array or batch column");
        return false;
    }
    if (batch->mem != NXG_MEM_DEVICE || !is_device_ptr(d->chan_off) ||
        !is_device_ptr(out->client_off) || (out->out && !is_device_ptr(out->out)) ||
        (ne && (!is_device_ptr(d->ent_row) || !is_device_ptr(batch->id))) ||
        (heap && !is_device_ptr(heap))) {
        set_err(err, "nxg_encode_clients takes device memory only (batch, heap, the dispatch's "
                     "arrays, out->out and out->client_off)");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    out->n_bytes = 0;
    const uint64_t cnt = (uint64_t)n_clients + 1;
    if (ne == 0) {  // no entries: every payload is empty, and no tile kernel runs
        HIPCHK(hipMemsetAsync(out->client_off, 0, cnt * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    const uint64_t nt = nxg_enc_clients_tiles(f64, ne);
    if (nt >= (1ull << 32)) {
        set_err(err, "too many entries for one call (%llu)", (unsigned long long)ne);
        return false;
    }
    if (!ensure_tstat(c, nt, err)) return false;
    const ColsDesc cd = desc_of(batch);
    const NxgGather g{d->ent_row, ne, d->chan_off, n_clients, out->client_off};
    std::vector<uint64_t> off(cnt);
    uint64_t total = 0;
    auto pass = [&](uint8_t* dout, uint64_t cap) -> bool {
        DevStatus* st;
        uint32_t slot;
        // all-ones first: a chan_off that decreases can make the tiles' walks skip a client, and
        // an element left unwritten then fails the check below (every message has at least one
        // byte, so the written offsets decrease exactly where chan_off does)
        HIPCHK(hipMemsetAsync(out->client_off, 0xff, cnt * 8, c->stream));
        if (!begin_call(c, &st, &slot, err)) return false;
        const hipError_t le = nxg_launch_enc_clients(f64, cd, heap, g, dout, cap, c->tstat,
                                                     c->epoch, st, c->grid_enc_f64,
                                                     c->grid_enc_gen, c->stream);
        if (!end_call(c, err)) return false;
        HIPCHK(le);
        HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipMemcpyAsync(off.data(), out->client_off, cnt * 8, hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const DevStatus h = c->hst[slot];
        if (h.timeout) {
            set_err(err, "device look-back watchdog expired");
            return false;
        }
        if (h.err_key) {
            set_err(err, "entry %llu names a row at or past the batch's %llu rows",
                    (unsigned long long)~h.err_key, (unsigned long long)batch->n_rows);
            return false;
        }
        if (h.err_kind) {
            if (h.err_kind == NXG_TOO_BIG)
                set_err(err, "encode failed: a message exceeds MAX_BATCH (%llu bytes) or a size "
                             "guard (PackError::TooBig)", (unsigned long long)kMaxBatch);
            else
                set_err(err, "encode failed: PackError kind %u", h.err_kind);
            return false;
        }
        bool sorted = !(h.irregular & 1u) && off[n_clients] == h.total_bytes;
        for (uint64_t i = 0; sorted && i < n_clients; i++) sorted = off[i] <= off[i + 1];
        if (!sorted) {
            set_err(err, "d->chan_off is not a dispatch's: it must not decrease and must end at "
                         "d->n_entries (%llu)", (unsigned long long)ne);
            return false;
        }
        total = h.total_bytes;
        out->n_bytes = total;
        if (dout && (h.capacity || total > cap)) {
            set_err(err, "output buffer too small: need %llu bytes, have %llu",
                    (unsigned long long)total, (unsigned long long)cap);
            return false;
        }
        return true;
    };
    // each client's payload goes out as one frame: none may pass MAX_BATCH
    auto frames_ok = [&]() -> bool {
        for (uint64_t i = 0; i < n_clients; i++)
            if (off[i + 1] - off[i] > kMaxBatch) {
                set_err(err, "client %llu's payload of %llu bytes exceeds MAX_BATCH (%llu): encode "
                             "that client's rows with nxg_encode_frames",
                        (unsigned long long)i, (unsigned long long)(off[i + 1] - off[i]),
                        (unsigned long long)kMaxBatch);
                return false;
            }
        return true;
    };
    if (!out->out) return pass(nullptr, 0);
    if (out->cap_bytes > kMaxBatch) {
        if (!pass(nullptr, 0) || !frames_ok()) return false;
        if (total > out->cap_bytes) {
            set_err(err, "output buffer too small: need %llu bytes, have %llu",
                    (unsigned long long)total, (unsigned long long)out->cap_bytes);
            return false;
        }
    }
    return pass(out->out, out->cap_bytes) && frames_ok();
}

// ---- a dispatch's entries as archive batch records (the recorder's batch loop, record.rs:307-347)
// (nxg_record.hip). Argument checks on the host, the launches, one read-back of the call's head.
namespace {
const char* rec_cause(uint32_t cause) {
    switch (cause) {
    case kRecRow: return "ent_row names a row at or past the batch's n_rows";
    case kRecTag: return "an unknown tag (PackError kind 1)";
    case kRecBig: return "a size guard (PackError::TooBig)";
    case kRecKids: return "a child range outside the batch's n_children";
    case kRecNoKids: return "a container with elements but no child columns";
    case kRecDepth: return "a value nested deeper than NXG_MAX_DEPTH";
    default: return "unknown cause";
    }
}
}  // namespace

bool nxg_record_entries(NxgCtx* c, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_chans, const NxgRecordTable* tab,
                        NxgRecordBatches* out, NetidxError* err) {
    if (!c || !batch || !d || !tab || !out || !d->chan_off || !out->rec_off ||
        (n_chans && !out->rec_items) || (tab->n_subs && !tab->arch_id_of_sub)) {
        set_err(err, "null argument");
        return false;
    }
    const uint64_t ne = d->n_entries;
    const bool f64 = batch->layout == NXG_LAYOUT_F64;
    if (ne && (!d->ent_sub || !d->ent_row)) {
        set_err(err, "null entry array");
        return false;
    }
    if (batch->n_rows && (!batch->fixed || (!f64 && (!batch->tag || !batch->aux)))) {
        set_err(err, "null batch column");
        return false;
    }
    if (ne > d->cap_entries) {
        set_err(err, "d->n_entries (%llu) exceeds d->cap_entries (%llu)", (unsigned long long)ne,
                (unsigned long long)d->cap_entries);
        return false;
    }
    if (ne >= (1ull << 39)) {
        set_err(err, "too many entries for one call (%llu)", (unsigned long long)ne);
        return false;
    }
    const bool kids = !f64 && batch->n_children && batch->ctag && batch->cfixed && batch->caux;
    {
        const void* need[] = {d->chan_off, out->rec_off, n_chans ? out->rec_items : nullptr,
                              out->out, heap, tab->n_subs ? tab->arch_id_of_sub : nullptr,
                              ne ? d->ent_sub : nullptr, ne ? d->ent_row : nullptr,
                              batch->n_rows ? batch->fixed : nullptr,
                              batch->n_rows && !f64 ? batch->tag : nullptr,
                              batch->n_rows && !f64 ? batch->aux : nullptr,
                              kids ? batch->ctag : nullptr, kids ? batch->cfixed : nullptr,
                              kids ? batch->caux : nullptr};
        bool dev = batch->mem == NXG_MEM_DEVICE;
        for (const void* p : need) dev = dev && (!p || is_device_ptr(p));
        if (!dev) {
            set_err(err, "nxg_record_entries takes device memory only (batch, heap, the dispatch's "
                         "arrays, tab->arch_id_of_sub, out->out, out->rec_off and out->rec_items)");
            return false;
        }
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    out->n_bytes = out->n_items = out->n_dropped = 0;
    if (ne == 0) {  // no entries: no record, and no kernel runs
        HIPCHK(hipMemsetAsync(out->rec_off, 0, ((uint64_t)n_chans + 1) * 8, c->stream));
        if (n_chans) HIPCHK(hipMemsetAsync(out->rec_items, 0, (uint64_t)n_chans * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgRecArgs a{};
    a.cols = desc_of(batch);
    a.cols.n_ctl = 0;
    if (f64) a.cols.tag = nullptr, a.cols.aux = nullptr;
    if (!kids) {
        a.cols.ctag = nullptr, a.cols.cfixed = nullptr, a.cols.caux = nullptr;
        a.cols.n_children = 0;
    }
    a.heap = heap;
    a.ent_sub = d->ent_sub;
    a.ent_row = d->ent_row;
    a.chan_off = d->chan_off;
    a.n_ent = ne;
    a.n_chans = n_chans;
    a.arch_id_of_sub = tab->arch_id_of_sub;
    a.n_subs = tab->n_subs;
    a.out = out->out;
    a.cap = out->out ? out->cap_bytes : 0;
    a.rec_off = out->rec_off;
    a.rec_items = out->rec_items;
    const size_t need = nxg_rec_scratch_bytes(ne, n_chans);
    if (!ensure_dscratch(c, need, err)) return false;
    NxgRecHead h;
    HIPCHK(nxg_launch_record(a, c->dscratch, c->stream));
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.chan_bad) {
        set_err(err, "d->chan_off is not a dispatch's at channel %u: it must not decrease and "
                     "must end at d->n_entries (%llu)", h.chan_bad - 1, (unsigned long long)ne);
        return false;
    }
    if (h.err_inv) {
        const uint64_t entry = ~(h.err_inv >> 8 | 0xffull << 56);
        set_err(err, "entry %llu: %s", (unsigned long long)entry,
                rec_cause((uint32_t)(h.err_inv & 0xff)));
        return false;
    }
    if (h.vec_bad) {
        set_err(err, "encode failed: channel %u's items exceed MAX_VEC (PackError::TooBig)",
                h.vec_bad - 1);
        return false;
    }
    out->n_bytes = h.n_bytes;
    out->n_items = h.n_items;
    out->n_dropped = h.n_dropped;
    if (out->out && h.n_bytes > out->cap_bytes) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)h.n_bytes, (unsigned long long)out->cap_bytes);
        return false;
    }
    return true;
}

// ---- playback: a decoded window (process_batch, session_shard.rs:196-245) or its image (reimage,
// session_shard.rs:375-409) as publisher update rows (nxg_replay.hip). Argument checks on the host,
// the launches, one read-back of the call's head; a second small launch and read-back only when a
// record missed.
static bool replay_out_ok(const NxgReplayRows* out, const char* what, NetidxError* err) {
    if (!out->rec_off || (out->cap_miss && !out->miss_row) ||
        (out->cap_rows && (!out->id || !out->tag || !out->fixed || !out->aux || !out->src_row))) {
        set_err(err, "null output array");
        return false;
    }
    const void* need[] = {out->rec_off, out->cap_miss ? out->miss_row : nullptr,
                          out->cap_rows ? out->id : nullptr, out->cap_rows ? out->tag : nullptr,
                          out->cap_rows ? out->fixed : nullptr, out->cap_rows ? out->aux : nullptr,
                          out->cap_rows ? out->src_row : nullptr};
    for (const void* p : need)
        if (p && !is_device_ptr(p)) {
            set_err(err, "%s takes device memory only (the table, the columns and every output "
                         "array)", what);
            return false;
        }
    return true;
}

// the launches and the read-backs; a.n > 0
static bool replay_run(NxgCtx* c, NxgRpArgs a, const std::vector<uint64_t>& hbeg,
                const std::vector<uint64_t>& hend, NxgReplayRows* out, NetidxError* err) {
    a.cap_rows = out->cap_rows;
    a.oid = out->id, a.otag = out->tag, a.ofixed = out->fixed, a.oaux = out->aux;
    a.osrc = out->src_row;
    a.rec_off = out->rec_off;
    a.miss_row = out->miss_row;
    a.cap_miss = out->cap_miss;
    if (!ensure_dscratch(c, nxg_rp_scratch_bytes(a.n, a.n_recs), err)) return false;
    NxgRpHead h;
    HIPCHK(nxg_launch_replay(a, c->dscratch, hbeg.data(), hend.data(), c->stream));
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.stop_inv) {  // rare: list the misses of the stopping record
        HIPCHK(nxg_launch_replay_misses(a, c->dscratch, a.order ? 0u : (uint32_t)h.n_done,
                                        c->stream));
        HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    out->n_rows = h.n_rows;
    out->n_done = h.n_done;
    out->n_miss = h.n_miss;
    // records in front of n_done hold no miss: what is not kept there was dropped
    uint64_t rows = 0;
    for (uint64_t i = 0; i < h.n_done && i < a.n_recs; i++) rows += hend[i] - hbeg[i];
    out->n_dropped = rows - h.n_rows - (a.order ? h.n_miss : 0);
    if (h.n_rows > out->cap_rows) {
        set_err(err, "the rows' capacity is %llu; the replay keeps %llu",
                (unsigned long long)out->cap_rows, (unsigned long long)h.n_rows);
        return false;
    }
    return true;
}

bool nxg_replay_window(NxgCtx* c, const NxgColumns* window, const NxgArchiveBatchInfo* info,
                       uint32_t n_recs, const NxgReplayTable* tab, NxgReplayRows* out,
                       NetidxError* err) {
    if (!c || !window || !tab || !out || (n_recs && !info) || (tab->n_ids && !tab->pub_id_of_arch)) {
        set_err(err, "null argument");
        return false;
    }
    if (window->mem != NXG_MEM_DEVICE || window->layout != NXG_LAYOUT_MIXED ||
        (window->n_rows && (!window->id || !window->tag || !window->fixed || !window->aux))) {
        set_err(err, "a window is replayed from device MIXED-layout columns");
        return false;
    }
    std::vector<uint64_t> hbeg((size_t)n_recs + 1), hend(n_recs);
    for (uint32_t i = 0; i < n_recs; i++) {
        const uint64_t lo = info[i].row_off, cnt = info[i].n_rows;
        if (lo > window->n_rows || cnt > window->n_rows - lo) {
            set_err(err, "info[%u]: rows [%llu, + %llu) leave the window's %llu rows", i,
                    (unsigned long long)lo, (unsigned long long)cnt,
                    (unsigned long long)window->n_rows);
            return false;
        }
        if (i && lo < hend[i - 1]) {
            set_err(err, "info[%u].row_off (%llu) lies in front of the end of record %u (%llu): "
                         "row_off must not decrease and records must not overlap", i,
                    (unsigned long long)lo, i - 1, (unsigned long long)hend[i - 1]);
            return false;
        }
        hbeg[i] = lo;
        hend[i] = lo + cnt;
    }
    const uint64_t first = n_recs ? hbeg[0] : 0, n = n_recs ? hend[n_recs - 1] - first : 0;
    hbeg[n_recs] = first + n;
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if (!replay_out_ok(out, "nxg_replay_window", err)) return false;
    if ((n && !is_device_ptr(window->id)) || (tab->n_ids && !is_device_ptr(tab->pub_id_of_arch))) {
        set_err(err, "nxg_replay_window takes device memory only (the table, the columns and every "
                     "output array)");
        return false;
    }
    out->n_rows = out->n_dropped = out->n_miss = 0;
    out->n_done = n_recs;
    if (n == 0) {  // no rows: no update, and no kernel runs
        HIPCHK(hipMemsetAsync(out->rec_off, 0, ((uint64_t)n_recs + 1) * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgRpArgs a{};
    a.id = window->id;
    a.tag = window->tag, a.fixed = window->fixed, a.aux = window->aux;
    a.first = first, a.n = n;
    a.n_recs = n_recs;
    a.pub_id_of_arch = tab->pub_id_of_arch;
    a.n_ids = tab->n_ids;
    return replay_run(c, a, hbeg, hend, out, err);
}

bool nxg_replay_image(NxgCtx* c, const NxgArchiveImage* image, const uint32_t* order,
                      uint64_t n_order, const NxgReplayTable* tab, NxgReplayRows* out,
                      NetidxError* err) {
    if (!c || !image || !tab || !out || (n_order && !order) ||
        (tab->n_ids && !tab->pub_id_of_arch)) {
        set_err(err, "null argument");
        return false;
    }
    if (image->n_rows > image->cap_rows ||
        (image->n_rows && (!image->id || !image->tag || !image->fixed || !image->aux))) {
        set_err(err, "the image's arrays are null or n_rows exceeds cap_rows");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if (!replay_out_ok(out, "nxg_replay_image", err)) return false;
    if ((n_order && !is_device_ptr(order)) || (image->n_rows && !is_device_ptr(image->id)) ||
        (tab->n_ids && !is_device_ptr(tab->pub_id_of_arch))) {
        set_err(err, "nxg_replay_image takes device memory only (the image, order, the table and "
                     "every output array)");
        return false;
    }
    out->n_rows = out->n_dropped = out->n_miss = 0;
    out->n_done = 1;
    if (n_order == 0) {
        HIPCHK(hipMemsetAsync(out->rec_off, 0, 2 * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgRpArgs a{};
    a.order = order;
    a.img_id = image->id;
    a.n_img = image->n_rows;
    a.tag = image->tag, a.fixed = image->fixed, a.aux = image->aux;
    a.first = 0, a.n = n_order;
    a.n_recs = 1;
    a.pub_id_of_arch = tab->pub_id_of_arch;
    a.n_ids = tab->n_ids;
    const std::vector<uint64_t> hbeg{0, n_order}, hend{n_order};
    return replay_run(c, a, hbeg, hend, out, err);
}

// ---- the value table: `pbl.current = v` and a subscription's `last`, on the device --------------
// (nxg_value_table.hip). Every call: argument checks on the host, the launches, one read-back of
// the call's head, then the table's counters.
namespace {
const char* vt_cause(uint32_t cause) {
    switch (cause & ~kVtOld) {
    case kVtRow: return "src_row names a row at or past the batch's n_rows";
    case kVtTag: return "a tag outside 0..27 and NXG_TAG_UNSUBSCRIBED";
    case kVtHeap: return "a payload outside the heap";
    case kVtKids: return "a child range outside the child columns";
    case kVtNoKids: return "a container without child columns";
    case kVtDepth: return "a value nested deeper than NXG_MAX_DEPTH";
    case kVtNotF64: return "NXG_NOT_F64: a value that is not F64 for a table without a tag column";
    case kVtSlot: return "a slot at or past n_slots";
    default: return "unknown cause";
    }
}

bool vt_refused(const NxgVtHead& h, NetidxError* err) {
    if (!h.err_inv) return false;
    const uint32_t cause = (uint32_t)(h.err_inv & 0xff);
    const uint64_t slot = ~(h.err_inv >> 8 | 0xffull << 56);
    set_err(err, "slot %llu: %s%s", (unsigned long long)slot, vt_cause(cause),
            (cause & kVtOld) ? " (the value the table holds)" : "");
    return true;
}

bool vt_table_ok(const NxgValueTable* t, const char* name, NetidxError* err) {
    const bool mixed = t->tag != nullptr;
    if (t->n_slots >= 0xffffffffull) {
        set_err(err, "%s: a table holds fewer than 2^32 - 1 slots", name);
        return false;
    }
    if ((t->n_slots && !t->fixed) || (mixed && !t->aux) ||
        (mixed && t->cap_bytes && !t->heap) ||
        (mixed && t->cap_children && (!t->ctag || !t->cfixed || !t->caux))) {
        set_err(err, "%s: null array", name);
        return false;
    }
    if (mixed && (t->heap_used > t->cap_bytes || t->child_used > t->cap_children ||
                  t->heap_live > t->heap_used || t->child_live > t->child_used)) {
        set_err(err, "%s: counters past their capacities (heap %llu live / %llu used / %llu, "
                     "children %llu / %llu / %llu)", name, (unsigned long long)t->heap_live,
                (unsigned long long)t->heap_used, (unsigned long long)t->cap_bytes,
                (unsigned long long)t->child_live, (unsigned long long)t->child_used,
                (unsigned long long)t->cap_children);
        return false;
    }
    const void* ptrs[] = {t->tag, t->fixed, t->aux, mixed ? t->heap : nullptr,
                          mixed ? t->ctag : nullptr, mixed ? t->cfixed : nullptr,
                          mixed ? t->caux : nullptr};
    for (const void* p : ptrs)
        if (p && !is_device_ptr(p)) {
            set_err(err, "%s: an array is not device memory", name);
            return false;
        }
    return true;
}

void vt_spans(const NxgValueTable* t, std::vector<Span>* v) {
    const bool mixed = t->tag != nullptr;
    const uint64_t n = t->n_slots, k = mixed ? t->cap_children : 0;
    const std::pair<const void*, uint64_t> a[] = {
        {t->tag, n},       {t->fixed, n * 8},  {t->aux, mixed ? n * 4 : 0},
        {t->heap, mixed ? t->cap_bytes : 0},   {t->ctag, k},
        {t->cfixed, k * 8}, {t->caux, k * 4}};
    for (const auto& x : a)
        if (x.first && x.second) v->push_back(span_of(x.first, x.second));
}

NxgVtDst vt_dst(const NxgValueTable* t, bool fresh) {
    const bool mixed = t->tag != nullptr;
    NxgVtDst d{};
    d.tag = t->tag;
    d.fixed = t->fixed;
    d.aux = mixed ? t->aux : nullptr;
    d.n_slots = t->n_slots;
    if (mixed) {
        d.heap = t->heap;
        d.ctag = t->ctag;
        d.cfixed = t->cfixed;
        d.caux = t->caux;
        d.cap_bytes = t->cap_bytes;
        d.cap_children = t->cap_children;
        d.heap_used = fresh ? 0 : t->heap_used;
        d.child_used = fresh ? 0 : t->child_used;
    }
    return d;
}

// the table as a source of values: what it has written so far bounds every range
NxgVtSrc vt_src_of_table(const NxgValueTable* t) {
    const bool mixed = t->tag != nullptr;
    NxgVtSrc s{};
    s.tag = t->tag;
    s.fixed = t->fixed;
    s.aux = mixed ? t->aux : nullptr;
    s.n_rows = t->n_slots;
    if (mixed) {
        s.heap = t->heap;
        s.heap_len = t->heap_used;
        if (t->child_used) {
            s.ctag = t->ctag;
            s.cfixed = t->cfixed;
            s.caux = t->caux;
            s.n_children = t->child_used;
        }
    }
    return s;
}

bool vt_batch(const NxgColumns* b, const uint8_t* heap, uint64_t heap_len, const uint64_t* src_row,
              uint64_t n_sel, NxgVtSrc* out, std::vector<Span>* spans, NetidxError* err) {
    NxgVtSrc s{};
    if (b) {
        const bool f64 = b->layout == NXG_LAYOUT_F64;
        if (b->mem != NXG_MEM_DEVICE) {
            set_err(err, "batch->mem: the value table takes device columns");
            return false;
        }
        if (b->n_rows && (!b->fixed || (!f64 && (!b->tag || !b->aux)))) {
            set_err(err, "batch: null column");
            return false;
        }
        if (!f64 && b->n_children && (!b->ctag || !b->cfixed || !b->caux)) {
            set_err(err, "batch: n_children without child columns");
            return false;
        }
        s.tag = f64 ? nullptr : b->tag;
        s.fixed = b->fixed;
        s.aux = f64 ? nullptr : b->aux;
        s.n_rows = b->n_rows;
        if (!f64 && b->n_children) {
            s.ctag = b->ctag;
            s.cfixed = b->cfixed;
            s.caux = b->caux;
            s.n_children = b->n_children;
        }
        cols_spans(b, spans);
    }
    if (heap_len && !heap) {
        set_err(err, "heap: null with heap_len %llu", (unsigned long long)heap_len);
        return false;
    }
    s.heap = heap;
    s.heap_len = heap ? heap_len : 0;
    const void* ptrs[] = {s.tag, s.fixed, s.aux, s.ctag, s.cfixed, s.caux, s.heap, src_row};
    for (const void* p : ptrs)
        if (p && !is_device_ptr(p)) {
            set_err(err, "batch, heap or src_row: not device memory");
            return false;
        }
    if (s.heap && s.heap_len) spans->push_back(span_of(s.heap, s.heap_len));
    if (src_row && n_sel) spans->push_back(span_of(src_row, n_sel * 8));
    *out = s;
    return true;
}

// the launches and the read-back; a segment list that turns out too short (rows named by many
// slots) repeats the call once with the size just learned -- nothing was written
bool vt_run(NxgCtx* c, NxgVtArgs a, uint64_t seg_cap, NxgVtHead* h, NetidxError* err) {
    for (int attempt = 0;; attempt++) {
        const size_t need = nxg_vt_scratch_bytes(a.dst.n_slots, seg_cap,
                                                 a.dst.tag ? kVtPathMixed : kVtPathF64);
        if (!ensure_dscratch(c, need, err)) return false;
        a.seg_cap = seg_cap;
        HIPCHK(nxg_launch_vt_apply(a, c->dscratch, c->ncu, c->stream));
        HIPCHK(hipMemcpyAsync(h, c->dscratch, sizeof *h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const bool fits = h->need_bytes <= a.dst.cap_bytes - a.dst.heap_used &&
                          h->need_children <= a.dst.cap_children - a.dst.child_used;
        if (!h->seg_short || h->err_inv || !fits || attempt) return true;
        seg_cap = h->n_leaves;
    }
}

bool vt_entry(NxgCtx* c, NetidxError* err) {
    if (!no_pending(c, err)) return false;
    return set_device(c, err);
}
}  // namespace

bool nxg_value_table_init(NxgCtx* c, NxgValueTable* t, NetidxError* err) {
    if (!c || !t) {
        set_err(err, "null argument");
        return false;
    }
    {
        NxgValueTable z = *t;  // the counters are outputs: reset only once nothing can refuse
        z.heap_used = z.heap_live = z.child_used = z.child_live = 0;
        if (!vt_table_ok(&z, "t", err) || !vt_entry(c, err)) return false;
    }
    if (t->n_slots) {
        if (t->tag) {
            HIPCHK(hipMemsetAsync(t->tag, 16, t->n_slots, c->stream));  // Value::Null
            HIPCHK(hipMemsetAsync(t->aux, 0, t->n_slots * 4, c->stream));
        }
        HIPCHK(hipMemsetAsync(t->fixed, 0, t->n_slots * 8, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    t->heap_used = t->heap_live = t->child_used = t->child_live = 0;
    return true;
}

bool nxg_value_table_apply(NxgCtx* c, NxgValueTable* t, const NxgColumns* batch,
                           const uint8_t* heap, uint64_t heap_len, const uint64_t* src_row,
                           NxgValueApply* out, NetidxError* err) {
    if (!c || !t || !batch || !out || (t->n_slots && !src_row)) {
        set_err(err, "null argument");
        return false;
    }
    *out = NxgValueApply{};
    if (!vt_table_ok(t, "t", err)) return false;
    NxgVtArgs a{};
    std::vector<Span> tb, in;
    if (!vt_batch(batch, heap, heap_len, src_row, t->n_slots, &a.batch, &in, err)) return false;
    vt_spans(t, &tb);
    if (overlaps(tb, in)) {
        set_err(err, "the batch, its heap or src_row overlaps the table's arrays");
        return false;
    }
    if (!vt_entry(c, err)) return false;
    if (!t->n_slots) return true;
    a.old = vt_src_of_table(t);
    a.dst = vt_dst(t, false);
    a.src_row = src_row;
    a.n_sel = t->n_slots;
    NxgVtHead h{};
    const uint64_t seg = std::min(batch->n_rows + a.batch.n_children,
                                  a.dst.cap_bytes - a.dst.heap_used);
    if (!vt_run(c, a, seg, &h, err)) return false;
    if (vt_refused(h, err)) return false;
    out->n_applied = h.n_applied;
    if (!t->tag) return true;  // an F64 table: no payload
    out->need_bytes = h.need_bytes;
    out->need_children = h.need_children;
    out->live_bytes = t->heap_live - std::min(t->heap_live, h.old_bytes) + h.need_bytes;
    out->live_children = t->child_live - std::min(t->child_live, h.old_children) + h.need_children;
    if (!h.ok) {
        set_err(err, "NXG_CAPACITY: the new values need %llu heap bytes and %llu child slots, the "
                     "table has %llu and %llu left; it would hold %llu live bytes and %llu live "
                     "child slots (nxg_value_table_rebuild)",
                (unsigned long long)h.need_bytes, (unsigned long long)h.need_children,
                (unsigned long long)(t->cap_bytes - t->heap_used),
                (unsigned long long)(t->cap_children - t->child_used),
                (unsigned long long)out->live_bytes, (unsigned long long)out->live_children);
        return false;
    }
    t->heap_used += h.need_bytes;
    t->child_used += h.need_children;
    t->heap_live = out->live_bytes;
    t->child_live = out->live_children;
    return true;
}

bool nxg_value_table_rebuild(NxgCtx* c, const NxgValueTable* src, const NxgColumns* batch,
                             const uint8_t* heap, uint64_t heap_len, const uint64_t* src_row,
                             NxgValueTable* dst, NxgValueApply* out, NetidxError* err) {
    if (!c || !src || !dst || !out) {
        set_err(err, "null argument");
        return false;
    }
    *out = NxgValueApply{};
    if (!vt_table_ok(src, "src", err)) return false;
    {
        NxgValueTable d = *dst;  // dst's counters are outputs
        d.heap_used = d.heap_live = d.child_used = d.child_live = 0;
        if (!vt_table_ok(&d, "dst", err)) return false;
    }
    if (dst->n_slots < src->n_slots || (dst->tag == nullptr) != (src->tag == nullptr)) {
        set_err(err, "dst: it needs at least src's %llu slots and src's kind (with or without a "
                     "tag column)", (unsigned long long)src->n_slots);
        return false;
    }
    if (!batch) src_row = nullptr;
    NxgVtArgs a{};
    std::vector<Span> db, in;
    if (!vt_batch(batch, heap, heap_len, src_row, src->n_slots, &a.batch, &in, err)) return false;
    vt_spans(src, &in);
    vt_spans(dst, &db);
    if (overlaps(db, in)) {
        set_err(err, "dst overlaps src, the batch, its heap or src_row");
        return false;
    }
    if (!vt_entry(c, err)) return false;
    if (!dst->n_slots) {
        dst->heap_used = dst->heap_live = dst->child_used = dst->child_live = 0;
        return true;
    }
    a.old = vt_src_of_table(src);
    a.dst = vt_dst(dst, true);
    a.src_row = src_row;
    a.n_sel = src->n_slots;
    a.rebuild = 1;
    NxgVtHead h{};
    const uint64_t seg = std::min(a.batch.n_rows + a.batch.n_children + src->n_slots +
                                      a.old.n_children, a.dst.cap_bytes);
    if (!vt_run(c, a, seg, &h, err)) return false;
    if (vt_refused(h, err)) return false;
    out->n_applied = h.n_applied;
    if (!dst->tag) return true;
    out->need_bytes = out->live_bytes = h.need_bytes;
    out->need_children = out->live_children = h.need_children;
    if (!h.ok) {
        set_err(err, "NXG_CAPACITY: the table's values need %llu heap bytes and %llu child slots, "
                     "dst holds %llu and %llu",
                (unsigned long long)h.need_bytes, (unsigned long long)h.need_children,
                (unsigned long long)dst->cap_bytes, (unsigned long long)dst->cap_children);
        return false;
    }
    dst->heap_used = dst->heap_live = h.need_bytes;
    dst->child_used = dst->child_live = h.need_children;
    return true;
}

bool nxg_value_table_set_unsubscribed(NxgCtx* c, NxgValueTable* t, const uint32_t* slot,
                                      uint64_t n, NetidxError* err) {
    if (!c || !t || (n && !slot)) {
        set_err(err, "null argument");
        return false;
    }
    if (!vt_table_ok(t, "t", err)) return false;
    if (!t->tag) {
        set_err(err, "t: a table without a tag column cannot hold Event::Unsubscribed");
        return false;
    }
    if (n >= 0xffffffffull || (n && !is_device_ptr(slot))) {
        set_err(err, "slot: device memory, fewer than 2^32 - 1 entries");
        return false;
    }
    std::vector<Span> tb;
    vt_spans(t, &tb);
    if (n && overlaps(tb, {span_of(slot, n * 4)})) {
        set_err(err, "slot overlaps the table's arrays");
        return false;
    }
    if (!vt_entry(c, err)) return false;
    if (!n) return true;
    NxgVtArgs a{};
    a.old = vt_src_of_table(t);
    a.dst = vt_dst(t, false);
    const size_t need = nxg_vt_scratch_bytes(t->n_slots, 0, kVtPathUnsub);
    if (!ensure_dscratch(c, need, err)) return false;
    HIPCHK(nxg_launch_vt_unsub(a, slot, n, c->dscratch, c->stream));
    NxgVtHead h{};
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (vt_refused(h, err)) return false;
    t->heap_live -= std::min(t->heap_live, h.old_bytes);
    t->child_live -= std::min(t->child_live, h.old_children);
    return true;
}

bool nxg_encoded_len(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint64_t* len_out,
                     NetidxError* err) {
    return encode_impl(c, in, heap, nullptr, 0, len_out, err);
}

bool nxg_encode_updates(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                        uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!out) {
        set_err(err, "null output buffer");
        return false;
    }
    return encode_impl(c, in, heap, out, cap, len_out, err);
}

// ---- subscriber write batches: publisher::To (publisher.rs:50-70) ------------------------------
bool nxg_write_cols_alloc(NxgCtx* c, uint64_t cap_rows, uint32_t mem, NxgWriteCols* out,
                          NetidxError* err) {
    if (!c || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (mem != NXG_MEM_DEVICE && mem != NXG_MEM_HOST) {
        set_err(err, "unknown memory kind %u", mem);
        return false;
    }
    if (!set_device(c, err)) return false;
    memset(out, 0, sizeof *out);
    out->mem = mem;
    out->cap_rows = cap_rows;
    const size_t n = std::max<uint64_t>(cap_rows, 2);
    const hipError_t e1 = mem == NXG_MEM_DEVICE
                              ? hipMalloc((void**)&out->wflags, n)
                              : hipHostMalloc((void**)&out->wflags, n, hipHostMallocDefault);
    const hipError_t e2 = e1 != hipSuccess ? e1
                          : mem == NXG_MEM_DEVICE
                              ? hipMalloc((void**)&out->wid, n * 8)
                              : hipHostMalloc((void**)&out->wid, n * 8, hipHostMallocDefault);
    if (e2 != hipSuccess) {
        set_err(err, "write column allocation of %zu rows failed: %s", n, hipGetErrorString(e2));
        nxg_write_cols_free(c, out);
        return false;
    }
    return true;
}

void nxg_write_cols_free(NxgCtx* c, NxgWriteCols* w) {
    if (!w) return;
    if (c) (void)hipSetDevice(c->device);
    void* ps[] = {w->wflags, w->wid};
    for (void* p : ps) {
        if (!p) continue;
        if (w->mem == NXG_MEM_DEVICE) (void)hipFree(p);
        else (void)hipHostFree(p);
    }
    memset(w, 0, sizeof *w);
}

// Replaces con.receive_batch(batch) on a publisher's connection (publisher/server.rs:660): the
// general decoder's To instantiation (nxg_decode_gen.hip), synchronously.
bool nxg_decode_writes(NxgCtx* c, const uint8_t* frame, uint64_t len, NxgColumns* out,
                       NxgWriteCols* wout, NxgStatus* ust, NetidxError* err) {
    return nxg_decode_writes_opts(c, frame, len, out, wout, nullptr, ust, err);
}

// opts->fast: the fast To decoder (nxg_decode_writes_fast.hip) first; a frame it declines
// (DevStatus.fast_fail) is rerun on the general decoder here, as finish_decode does for FAST_MIX.
bool nxg_decode_writes_opts(NxgCtx* c, const uint8_t* frame, uint64_t len, NxgColumns* out,
                            NxgWriteCols* wout, const NxgWriteDecodeOpts* opts, NxgStatus* ust,
                            NetidxError* err) {
    if (!c || !out || !wout || !ust || (!frame && len)) {
        set_err(err, "null argument");
        return false;
    }
    if (opts && (opts->fast > 1u || opts->reserved != 0u)) {
        set_err(err, "NxgWriteDecodeOpts: fast = %u (0 or 1), reserved = %u (must be 0)",
                opts->fast, opts->reserved);
        return false;
    }
    const bool try_fast = opts && opts->fast == 1u && nxg_wfast_takes(len);
    // (the argument checks come before any use of the context)
    if (!mixed_capable(out) || !out->id || !out->fixed) {
        set_err(err, "write batches decode into MIXED-layout columns");
        return false;
    }
    if (!wout->wflags || !wout->wid || wout->cap_rows < out->cap_rows) {
        set_err(err, "write columns hold %llu rows, the columns %llu",
                (unsigned long long)wout->cap_rows, (unsigned long long)out->cap_rows);
        return false;
    }
    if (out->mem != wout->mem || (out->mem != NXG_MEM_DEVICE && out->mem != NXG_MEM_HOST)) {
        set_err(err, "columns and write columns must both be device or both pinned host memory");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (len >= (1ull << 40)) {
        set_err(err, "frame too large (%llu bytes)", (unsigned long long)len);
        return false;
    }
    if (!set_device(c, err)) return false;
    const bool host_out = out->mem == NXG_MEM_HOST;
    NxgColumns* target = out;
    NxgColumns view;
    NxgWriteCols wtarget = *wout;
    if (host_out) {
        if (!ensure_dcols(c, out, err) || !ensure_dwcols(c, out->cap_rows, err)) return false;
        view = staged_view(c, out);
        target = &view;
        wtarget.wflags = c->dwflags;
        wtarget.wid = c->dwid;
    } else {
        // every array a kernel writes through must be device memory
        const void* ps[] = {out->id,     out->tag,     out->fixed,   out->aux,
                            out->ctag,   out->cfixed,  out->caux,    out->ctl_row,
                            out->ctl_off, out->ctl_len, out->ctl_variant, wout->wflags, wout->wid};
        for (const void* p : ps) {
            if (!is_device_ptr(p)) {
                set_err(err, "a column array is not device memory");
                return false;
            }
        }
    }
    const uint8_t* df;
    if (!frame_to_device(c, frame, len, &df, err)) return false;
    DevStatus* st;
    uint32_t slot;
    bool took = false;  // the fast decoder took the frame
    if (try_fast) {
        if (!begin_call(c, &st, &slot, err)) return false;
        // one buffer for both decoders, so that a fallback does not reallocate
        bool ok = ensure_glws(c, std::max(nxg_wfast_scratch_bytes(len), nxg_dec_gen_scratch_bytes(len)),
                              err);
        if (ok) {
            const ColsDesc d = desc_of(target, &wtarget);
            const hipError_t le = nxg_launch_dec_wfast(df, len, d, c->glws,
                                                       st, c->stream);
            if (le != hipSuccess) {
                set_err(err, "fast To decode launch failed: %s", hipGetErrorString(le));
                ok = false;
            }
        }
        if (!end_call(c, err) || !ok) return false;
        HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        took = !c->hst[slot].fast_fail;
    }
    if (!took) {
        if (!begin_call(c, &st, &slot, err)) return false;
        bool ok = ensure_glws(c, nxg_dec_gen_scratch_bytes(len), err);
        if (ok) {
            const ColsDesc d = desc_of(target, &wtarget);
            const hipError_t le =
                nxg_launch_dec_gen(df, len, d, reinterpret_cast<uint32_t*>(c->glws.get()), c->gruns,
                                   c->gruns + (size_t)gdec2::MAX_RUNS * gdec2::RUN_WORDS,
                                   c->wgs_dec_gen, st, c->stream, true);
            if (le != hipSuccess) {
                set_err(err, "To decode launch failed: %s", hipGetErrorString(le));
                ok = false;
            }
        }
        if (!end_call(c, err) || !ok) return false;
    }
    NxgStatus s;
    if (!finish_decode(c, df, len, target, FAST_NONE, st, slot, &s, err, took)) return false;
    s.path = took ? NXG_PATH_WRITES_FAST : NXG_PATH_WRITES;
    s.n_heartbeat = 0;
    out->layout = NXG_LAYOUT_MIXED;
    out->n_heartbeat = 0;
    if (s.err_kind == NXG_CAPACITY || (!s.err_kind && (s.n_rows > out->cap_rows ||
                                                       s.n_children > out->cap_children ||
                                                       s.n_ctl > out->cap_ctl))) {
        out->n_rows = out->n_children = out->n_ctl = 0;
        set_err(err, "column capacity exceeded (NXG_CAPACITY): the frame holds %llu rows, %llu "
                     "children, %llu control messages",
                (unsigned long long)s.n_rows, (unsigned long long)s.n_children,
                (unsigned long long)s.n_ctl);
        return false;
    }
    if (s.err_kind) s.n_rows = s.n_children = s.n_ctl = 0;  // the frame fails as a whole
    if (host_out && !s.err_kind) {
        target->n_rows = s.n_rows;
        target->n_children = s.n_children;
        target->n_ctl = s.n_ctl;
        if (s.n_rows) {
            HIPCHK(hipMemcpyAsync(wout->wflags, c->dwflags, s.n_rows, hipMemcpyDeviceToHost,
                                  c->stream));
            HIPCHK(hipMemcpyAsync(wout->wid, c->dwid, s.n_rows * 8, hipMemcpyDeviceToHost,
                                  c->stream));
        }
        NxgColumns hv = *out;
        if (!copy_cols_d2h(c, target, &hv, err)) return false;
    }
    out->n_rows = s.n_rows;
    out->n_children = s.n_children;
    out->n_ctl = s.n_ctl;
    *ust = s;
    return true;
}

static bool writes_args_ok(NxgCtx* c, const NxgColumns* in, const NxgWriteCols* win,
                           NetidxError* err) {
    if (!c || !in || !win) {
        set_err(err, "null argument");
        return false;
    }
    if (in->layout != NXG_LAYOUT_MIXED || !mixed_capable(in)) {
        set_err(err, "write batches encode from MIXED-layout columns");
        return false;
    }
    if (in->n_rows && (!win->wflags || !win->wid || win->cap_rows < in->n_rows)) {
        set_err(err, "write columns hold %llu rows, the batch %llu",
                (unsigned long long)win->cap_rows, (unsigned long long)in->n_rows);
        return false;
    }
    if (in->n_rows && (in->mem != win->mem || is_device_ptr(in->id) != is_device_ptr(win->wid))) {
        set_err(err, "columns and write columns must both be device or both host memory");
        return false;
    }
    return true;
}

bool nxg_encoded_writes_len(NxgCtx* c, const NxgColumns* in, const NxgWriteCols* win,
                            const uint8_t* heap, uint64_t* len_out, NetidxError* err) {
    if (!writes_args_ok(c, in, win, err)) return false;
    return encode_impl(c, in, heap, nullptr, 0, len_out, err, win);
}

// Replaces the subscriber's queue_send(&To::Write(..)) loop (subscriber/connection.rs:384-399):
// the general encoder's rows kernel in Write mode (nxg_encode_general.hip).
bool nxg_encode_writes(NxgCtx* c, const NxgColumns* in, const NxgWriteCols* win,
                       const uint8_t* heap, uint8_t* out, uint64_t cap, uint64_t* len_out,
                       NetidxError* err) {
    if (!writes_args_ok(c, in, win, err)) return false;
    return encode_impl(c, in, heap, out, cap, len_out, err, win);
}

// ---- write routing (publisher/server.rs:171-245, 497-576) ---------------------------------------
// Replaces handle_batch_inner's Write and Unsubscribe arms: nxg_route_writes.hip's passes, the
// dispatch of nxg_dispatch.hip for the channel fan-out, one copy of the head, one synchronisation.
bool nxg_route_writes(NxgCtx* c, const NxgWriteTable* tab, const uint8_t* frame,
                      const NxgColumns* cols, const NxgWriteCols* wcols, uint64_t row_begin,
                      uint64_t ctl_begin, uint64_t fresh_wid, NxgWriteRoute* out, NetidxError* err) {
    // (the argument checks come before any use of the context)
    if (!c || !tab || !cols || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (!wcols) {
        set_err(err, "wcols is null: the rows' wflags / wid come from nxg_decode_writes");
        return false;
    }
    if (cols->mem != NXG_MEM_DEVICE || wcols->mem != NXG_MEM_DEVICE) {
        set_err(err, "cols->mem / wcols->mem: write routing takes device columns");
        return false;
    }
    if (cols->layout != NXG_LAYOUT_MIXED || !mixed_capable(cols) || !cols->id) {
        set_err(err, "cols->layout: write batches are MIXED-layout columns");
        return false;
    }
    const uint64_t n_rows = cols->n_rows, n_ctl = cols->n_ctl;
    if (row_begin > n_rows) {
        set_err(err, "row_begin %llu is past the batch's %llu rows", (unsigned long long)row_begin,
                (unsigned long long)n_rows);
        return false;
    }
    if (ctl_begin > n_ctl) {
        set_err(err, "ctl_begin %llu is past the batch's %llu control spans",
                (unsigned long long)ctl_begin, (unsigned long long)n_ctl);
        return false;
    }
    const uint64_t rows = n_rows - row_begin, spans = n_ctl - ctl_begin;
    if (rows >= 0xffffffffull) {
        set_err(err, "row_begin: a call covers fewer than 2^32 rows");
        return false;
    }
    if (n_rows && (!wcols->wflags || !wcols->wid || wcols->cap_rows < n_rows)) {
        set_err(err, "wcols holds %llu rows, the batch %llu", (unsigned long long)wcols->cap_rows,
                (unsigned long long)n_rows);
        return false;
    }
    if (spans && !frame) {
        set_err(err, "frame is null: the Unsubscribe spans' Ids are read from it");
        return false;
    }
    if ((tab->n_ids && (!tab->perm_of_id || !tab->slot_of_id)) ||
        (tab->n_slots && !tab->slot_chan_off)) {  // (chan may be null: every list empty)
        set_err(err, "tab: null table array");
        return false;
    }
    if (out->cap_rows < n_rows || (n_rows && !out->outcome)) {
        set_err(err, "out->cap_rows: outcome[] holds %llu rows, the batch %llu",
                (unsigned long long)out->cap_rows, (unsigned long long)n_rows);
        return false;
    }
    if (!out->disp.chan_off || (out->disp.cap_entries && (!out->disp.ent_sub || !out->disp.ent_row)) ||
        (out->cap_wait && (!out->wait_row || !out->wait_id || !out->wait_wid)) ||
        (out->cap_unsub && !out->unsub_id) || (out->cap_reply && !out->reply)) {
        set_err(err, "out: null output array");
        return false;
    }
    if (!no_pending(c, err)) return false;
    HIPCHK(hipSetDevice(c->device));
    // the first-unsubscribe table: grown (and cleared) on demand, never cleared per call
    if (!grow(c, c->rw_first, tab->n_ids, kGrowFirstTable, err)) return false;
    if (++c->rw_epoch >= (1u << 24)) {  // wrap: stale words could alias epoch 1 again
        c->rw_epoch = 1;
        if (c->rw_first) HIPCHK(hipMemsetAsync(c->rw_first, 0, c->rw_first.cap() * 8, c->stream));
    }
    const size_t rw = (nxg_rw_scratch_bytes(rows, spans) + 255) & ~size_t(255);
    const size_t last = (tab->n_slots * 8 + 255) & ~size_t(255);
    const size_t need = rw + last + 64 + nxg_disp_scratch_bytes(rows, tab->n_chans);
    if (!ensure_dscratch(c, need, err)) return false;
    NxgRwArgs a{};
    a.tab = *tab;
    a.frame = frame;
    a.id = cols->id;
    a.wflags = wcols->wflags;
    a.wid = wcols->wid;
    a.ctl_row = cols->ctl_row;
    a.ctl_off = cols->ctl_off;
    a.ctl_len = cols->ctl_len;
    a.ctl_variant = cols->ctl_variant;
    a.n_rows = n_rows;
    a.n_ctl = n_ctl;
    a.row_begin = row_begin;
    a.ctl_begin = ctl_begin;
    a.fresh_wid = fresh_wid;
    a.first_unsub = c->rw_first;
    a.epoch = c->rw_epoch;
    a.outcome = out->outcome;
    a.wait_row = out->wait_row;
    a.wait_id = out->wait_id;
    a.wait_wid = out->wait_wid;
    a.cap_wait = out->cap_wait;
    a.unsub_id = out->unsub_id;
    a.cap_unsub = out->cap_unsub;
    a.reply = out->reply;
    a.cap_reply = out->cap_reply;
    HIPCHK(nxg_launch_route_writes(a, c->dscratch, c->dscratch + rw + last, out->disp.chan_off,
                                   out->disp.ent_sub, out->disp.ent_row, out->disp.cap_entries,
                                   reinterpret_cast<uint64_t*>(c->dscratch + rw), c->ncu,
                                   c->stream));
    NxgRwHead h;
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t s = h.first_sub_inv ? ~h.first_sub_inv : n_ctl;
    out->n_entries = out->disp.n_entries = h.n_entries;
    out->disp.n_unmatched = 0;
    out->n_wait = h.n_wait;
    out->n_unsub = s - ctl_begin;
    out->n_replies = h.n_row_replies + out->n_unsub;
    out->reply_len = h.row_bytes + h.span_bytes;
    out->n_fresh = h.n_fresh;
    for (int o = 0; o < 4; o++) out->n_outcome[o] = h.n_outcome[o];
    out->next_row = h.next_row;
    out->next_ctl = h.next_ctl;
    out->stopped_at_subscribe = s < n_ctl ? 1u : 0u;
    out->pad = 0;
    if (h.n_entries > out->disp.cap_entries || h.n_wait > out->cap_wait ||
        out->n_unsub > out->cap_unsub || out->reply_len > out->cap_reply) {
        set_err(err, "write routing needs %llu entries, %llu wait-list rows, %llu unsubscribed ids, "
                     "%llu reply bytes; capacities are %llu, %llu, %llu, %llu (NXG_CAPACITY)",
                (unsigned long long)h.n_entries, (unsigned long long)h.n_wait,
                (unsigned long long)out->n_unsub, (unsigned long long)out->reply_len,
                (unsigned long long)out->disp.cap_entries, (unsigned long long)out->cap_wait,
                (unsigned long long)out->cap_unsub, (unsigned long long)out->cap_reply);
        return false;
    }
    return true;
}

// ---- the path table and Subscribe routing (nxg_route_subscribes.hip) ----------------------------
struct NxgPathTable {
    int device = 0;
    uint64_t cap_paths = 0, cap_bytes = 0;
    uint64_t len = 0;        // live paths
    uint64_t heap_used = 0;  // bytes of the heap handed out (removed paths' bytes included)
    uint64_t used = 0;       // slots that are not empty: live + tombstones
    NxgPtView v{};
    DevBuf<uint8_t> stage;  // per-call device staging, grown on demand
};

namespace {

void pt_free_arrays(NxgPtView* v, bool heap) {
    if (v->hash) (void)hipFree(v->hash);
    if (v->key_off) (void)hipFree(v->key_off);
    if (v->key_len) (void)hipFree(v->key_len);
    if (v->id) (void)hipFree(v->id);
    if (heap && v->heap) (void)hipFree(v->heap);
    v->hash = v->key_off = v->id = nullptr;
    v->key_len = nullptr;
    if (heap) v->heap = nullptr;
}

// the slot arrays of a table of `slots` slots, every slot empty
bool pt_alloc_arrays(NxgCtx* c, uint64_t slots, NxgPtView* v, NetidxError* err) {
    v->mask = slots - 1;
    HIPCHK(hipMalloc(&v->hash, slots * 8));
    HIPCHK(hipMalloc(&v->key_off, slots * 8));
    HIPCHK(hipMalloc(&v->key_len, slots * 4));
    HIPCHK(hipMalloc(&v->id, slots * 8));
    HIPCHK(hipMemsetAsync(v->hash, 0, slots * 8, c->stream));
    return true;
}

bool pt_stage(NxgCtx* c, NxgPathTable* t, size_t need, NetidxError* err) {
    return grow(c, t->stage, need, kGrowDouble, err);
}

// the call's path list: offsets ascending, every path shorter than 2^32 bytes
bool pt_offsets_ok(const uint64_t* off, uint64_t n, NetidxError* err) {
    for (uint64_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xffffffffull) {
            set_err(err, "off: path %llu has no valid length", (unsigned long long)i);
            return false;
        }
    }
    return true;
}

bool pt_call_ok(NxgCtx* c, const NxgPathTable* t, NetidxError* err) {
    if (!c || !t) {
        set_err(err, "null argument");
        return false;
    }
    if (t->device != c->device) {
        set_err(err, "the path table belongs to device %d, the ctx to %d", t->device, c->device);
        return false;
    }
    return no_pending(c, err);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

NxgPathTable* nxg_path_table_new(NxgCtx* c, uint64_t cap_paths, uint64_t cap_bytes,
                                 NetidxError* err) {
    if (!c) {
        set_err(err, "null argument");
        return nullptr;
    }
    if (cap_paths > (1ull << 40) || cap_bytes > (1ull << 44)) {
        set_err(err, "cap_paths / cap_bytes: too large");
        return nullptr;
    }
    if (!set_device(c, err)) return nullptr;
    NxgPathTable* t = new NxgPathTable();
    t->device = c->device;
    t->cap_paths = cap_paths;
    t->cap_bytes = cap_bytes;
    uint64_t slots = 16;
    while (slots < 2 * cap_paths) slots *= 2;
    const auto fail = [&]() -> NxgPathTable* {
        pt_free_arrays(&t->v, true);
        delete t;
        return nullptr;
    };
    if (!pt_alloc_arrays(c, slots, &t->v, err)) return fail();
    // (16 spare bytes: keys are read in aligned 8-byte words)
    if (hipMalloc(&t->v.heap, cap_bytes + 16) != hipSuccess ||
        hipMemsetAsync(t->v.heap, 0, cap_bytes + 16, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_err(err, "path table: allocating %llu heap bytes failed", (unsigned long long)cap_bytes);
        return fail();
    }
    return t;
}

void nxg_path_table_free(NxgPathTable* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    pt_free_arrays(&t->v, true);
    delete t;
}

uint64_t nxg_path_table_len(const NxgPathTable* t) { return t ? t->len : 0; }

bool nxg_path_table_insert(NxgCtx* c, NxgPathTable* t, const uint8_t* paths, const uint64_t* off,
                           const uint64_t* id, uint64_t n, uint64_t* n_dup, NetidxError* err) {
    if (!pt_call_ok(c, t, err)) return false;
    if (n_dup) *n_dup = 0;
    if (!n) return true;
    if (!off || !id) {
        set_err(err, "off / id is null");
        return false;
    }
    if (!pt_offsets_ok(off, n, err)) return false;
    const uint64_t total = off[n] - off[0];
    if (total && !paths) {
        set_err(err, "paths is null");
        return false;
    }
    for (uint64_t i = 0; i < n; i++) {
        if (id[i] == NXG_NO_ID) {
            set_err(err, "id[%llu] is NXG_NO_ID", (unsigned long long)i);
            return false;
        }
    }
    if (n > t->cap_paths - t->len || total > t->cap_bytes - t->heap_used) {
        set_err(err, "path table holds %llu of %llu paths and %llu of %llu bytes; the call adds "
                     "%llu paths, %llu bytes (NXG_CAPACITY)",
                (unsigned long long)t->len, (unsigned long long)t->cap_paths,
                (unsigned long long)t->heap_used, (unsigned long long)t->cap_bytes,
                (unsigned long long)n, (unsigned long long)total);
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    const uint64_t slots = t->v.mask + 1;
    if (t->used + n > slots / 4 * 3) {  // tombstones piled up: the live entries into fresh arrays
        NxgPtView nv = t->v;
        nv.hash = nv.key_off = nv.id = nullptr;
        nv.key_len = nullptr;
        if (!pt_alloc_arrays(c, slots, &nv, err)) {
            pt_free_arrays(&nv, false);
            return false;
        }
        HIPCHK(nxg_launch_pt_rehash(t->v, nv, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        pt_free_arrays(&t->v, false);
        t->v = nv;
        t->used = t->len;
    }
    uint64_t m = 16;
    while (m < 2 * n) m *= 2;
    // head | off | id | h | tslot | tmp | state
    const size_t o_off = 256, o_id = o_off + up256((n + 1) * 8), o_h = o_id + up256(n * 8),
                 o_ts = o_h + up256(n * 8), o_tmp = o_ts + up256(n * 8), o_st = o_tmp + up256(m * 8);
    if (!pt_stage(c, t, o_st + up256(n), err)) return false;
    uint8_t* s = t->stage;
    HIPCHK(hipMemsetAsync(s, 0, 256, c->stream));
    HIPCHK(hipMemsetAsync(s + o_tmp, 0xff, m * 8, c->stream));
    HIPCHK(hipMemcpyAsync(s + o_off, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s + o_id, id, n * 8, hipMemcpyHostToDevice, c->stream));
    if (total)
        HIPCHK(hipMemcpyAsync(t->v.heap + t->heap_used, paths + off[0], total,
                              hipMemcpyHostToDevice, c->stream));
    NxgPtHead* dh = reinterpret_cast<NxgPtHead*>(s);
    HIPCHK(nxg_launch_pt_insert(t->v, t->heap_used - off[0], reinterpret_cast<uint64_t*>(s + o_off),
                                reinterpret_cast<uint64_t*>(s + o_id), n,
                                reinterpret_cast<uint64_t*>(s + o_h),
                                reinterpret_cast<uint64_t*>(s + o_tmp), m - 1,
                                reinterpret_cast<uint64_t*>(s + o_ts), s + o_st, dh, c->stream));
    NxgPtHead h;
    HIPCHK(hipMemcpyAsync(&h, dh, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    t->len += n - h.n_dup;
    t->heap_used += total;
    t->used += h.n_fresh;
    if (n_dup) *n_dup = h.n_dup;
    return true;
}

bool nxg_path_table_remove(NxgCtx* c, NxgPathTable* t, const uint8_t* paths, const uint64_t* off,
                           uint64_t n, uint64_t* n_missing, NetidxError* err) {
    if (!pt_call_ok(c, t, err)) return false;
    if (n_missing) *n_missing = 0;
    if (!n) return true;
    if (!off) {
        set_err(err, "off is null");
        return false;
    }
    if (!pt_offsets_ok(off, n, err)) return false;
    const uint64_t total = off[n] - off[0];
    if (total && !paths) {
        set_err(err, "paths is null");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    // head | off | the paths (16 spare bytes: read in aligned 8-byte words)
    const size_t o_off = 256, o_keys = o_off + up256((n + 1) * 8);
    if (!pt_stage(c, t, o_keys + up256(total + 16), err)) return false;
    uint8_t* s = t->stage;
    HIPCHK(hipMemsetAsync(s, 0, 256, c->stream));
    HIPCHK(hipMemcpyAsync(s + o_off, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (total)
        HIPCHK(hipMemcpyAsync(s + o_keys, paths + off[0], total, hipMemcpyHostToDevice, c->stream));
    NxgPtHead* dh = reinterpret_cast<NxgPtHead*>(s);
    HIPCHK(nxg_launch_pt_remove(t->v, s + o_keys - off[0], reinterpret_cast<uint64_t*>(s + o_off),
                                n, dh, c->stream));
    NxgPtHead h;
    HIPCHK(hipMemcpyAsync(&h, dh, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    t->len -= n - h.n_missing;
    if (n_missing) *n_missing = h.n_missing;
    return true;
}

bool nxg_path_table_lookup(NxgCtx* c, const NxgPathTable* t, const uint8_t* dheap,
                           const uint64_t* doff, const uint32_t* dlen, uint64_t n,
                           uint64_t* did_out, NetidxError* err) {
    if (!pt_call_ok(c, t, err)) return false;
    if (!n) return true;
    if (!is_device_ptr(doff) || !is_device_ptr(dlen) || !is_device_ptr(did_out)) {
        set_err(err, "doff / dlen / did_out: a path lookup takes device arrays");
        return false;
    }
    if (dheap && !is_device_ptr(dheap)) {  // (null: every path empty)
        set_err(err, "dheap: a path lookup takes device arrays");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(nxg_launch_pt_lookup(t->v, dheap, doff, dlen, n, did_out, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return true;
}

bool nxg_path_is_plain(const uint8_t* p, uint64_t len) {
    if (!p || !len) return false;
    for (uint64_t i = 0; i < len; i++) {
        if (p[i] == '\\') return false;
        if (p[i] == '/' && i + 1 < len && p[i + 1] == '/') return false;
    }
    return p[len - 1] != '/' || len == 1;
}

uint64_t nxg_path_hash(const uint8_t* p, uint64_t len) {
    uint64_t h = nxgpath::kSeed ^ len;
    for (uint64_t i = 0; p && i < len; i += 8) {
        uint64_t w = 0;  // the little-endian word of bytes i .. i + 8, zero past the end
        for (uint64_t b = 0; b < 8 && i + b < len; b++) w |= (uint64_t)p[i + b] << (8 * b);
        h = nxgpath::mix(h, w);
    }
    return nxgpath::finish_hash(h);
}

bool nxg_route_subscribes(NxgCtx* c, const NxgSubscribeTable* tab, const uint8_t* frame,
                          const NxgColumns* cols, uint64_t row_begin, uint64_t ctl_begin,
                          const uint32_t* span_perm, NxgSubscribeRoute* out, NetidxError* err) {
    // (the argument checks come before any use of the context)
    if (!c || !cols || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (!tab || !tab->paths || !tab->pub) {
        set_err(err, "tab: the table, tab->paths or tab->pub is null");
        return false;
    }
    if (cols->mem != NXG_MEM_DEVICE) {
        set_err(err, "cols->mem: subscribe routing takes device columns");
        return false;
    }
    if (cols->layout != NXG_LAYOUT_MIXED || !mixed_capable(cols)) {
        set_err(err, "cols->layout: To frames are decoded into MIXED-layout columns");
        return false;
    }
    const uint64_t n_ctl = cols->n_ctl;
    if (ctl_begin > n_ctl) {
        set_err(err, "ctl_begin %llu is past the batch's %llu control spans",
                (unsigned long long)ctl_begin, (unsigned long long)n_ctl);
        return false;
    }
    if (row_begin > cols->n_rows) {
        set_err(err, "row_begin %llu is past the batch's %llu rows", (unsigned long long)row_begin,
                (unsigned long long)cols->n_rows);
        return false;
    }
    const uint64_t spans = n_ctl - ctl_begin;
    if (spans >= 0xffffffffull) {
        set_err(err, "ctl_begin: a call covers fewer than 2^32 spans");
        return false;
    }
    const NxgPubTable* pub = tab->pub;
    if (out->cap_spans < n_ctl || (n_ctl && (!out->outcome || !out->span_id))) {
        set_err(err, "out->cap_spans: outcome[] / span_id[] hold %llu spans, the batch %llu",
                (unsigned long long)out->cap_spans, (unsigned long long)n_ctl);
        return false;
    }
    if ((out->cap_sub && (!out->sub_id || !out->sub_perm)) || (out->cap_deferred && !out->deferred) ||
        (out->cap_reply && !out->reply)) {
        set_err(err, "out: null output array");
        return false;
    }
    if ((pub->n_ids && !pub->slot_of_id) || (pub->n_slots && !pub->cur_fixed) ||
        (tab->n_defaults && (!tab->default_off || !tab->default_heap))) {
        set_err(err, "tab: null table array");
        return false;
    }
    if (tab->paths->device != c->device) {
        set_err(err, "tab->paths belongs to device %d, the ctx to %d", tab->paths->device,
                c->device);
        return false;
    }
    if (!no_pending(c, err)) return false;
    out->n_spans = out->n_sub = out->n_deferred = out->n_replies = out->reply_len = 0;
    for (int o = 0; o < 5; o++) out->n_outcome[o] = 0;
    out->next_ctl = ctl_begin;
    out->stopped = 0;
    out->pad = 0;
    if (!spans) return true;  // the end of the spans: nothing to launch
    // every pointer a kernel gets is device memory (a host pointer would fault there)
    struct {
        const void* p;
        bool need;
        const char* name;
    } const ptrs[] = {
        {frame, true, "frame"},
        {cols->ctl_row, true, "cols->ctl_row"},
        {cols->ctl_off, true, "cols->ctl_off"},
        {cols->ctl_len, true, "cols->ctl_len"},
        {cols->ctl_variant, true, "cols->ctl_variant"},
        {span_perm, false, "span_perm"},
        {out->outcome, true, "out->outcome"},
        {out->span_id, true, "out->span_id"},
        {out->sub_id, out->cap_sub != 0, "out->sub_id"},
        {out->sub_perm, out->cap_sub != 0, "out->sub_perm"},
        {out->deferred, out->cap_deferred != 0, "out->deferred"},
        {out->reply, out->cap_reply != 0, "out->reply"},
        {tab->allow_of_id, false, "tab->allow_of_id"},
        {tab->default_heap, tab->n_defaults != 0, "tab->default_heap"},
        {tab->default_off, tab->n_defaults != 0, "tab->default_off"},
        {pub->slot_of_id, pub->n_ids != 0, "tab->pub->slot_of_id"},
        {pub->cur_fixed, pub->n_slots != 0, "tab->pub->cur_fixed"},
        {pub->cur_tag, false, "tab->pub->cur_tag"},
        {pub->cur_aux, false, "tab->pub->cur_aux"},
        {pub->cur_heap, false, "tab->pub->cur_heap"},
        {pub->cur_ctag, false, "tab->pub->cur_ctag"},
        {pub->cur_cfixed, false, "tab->pub->cur_cfixed"},
        {pub->cur_caux, false, "tab->pub->cur_caux"},
    };
    for (const auto& q : ptrs) {
        if ((q.p || q.need) && !is_device_ptr(q.p)) {
            set_err(err, "%s: %s", q.name, q.p ? "not device memory" : "null");
            return false;
        }
    }
    if (pub->cur_ctag && (!pub->cur_cfixed || !pub->cur_caux)) {
        set_err(err, "tab->pub: cur_ctag without cur_cfixed / cur_caux");
        return false;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t need = nxg_rs_scratch_bytes(spans);
    if (!ensure_dscratch(c, need, err)) return false;
    NxgRsArgs a{};
    a.paths = tab->paths->v;
    a.cur.tag = const_cast<uint8_t*>(pub->cur_tag);
    a.cur.fixed = const_cast<uint64_t*>(pub->cur_fixed);
    a.cur.aux = const_cast<uint32_t*>(pub->cur_aux);
    a.cur.ctag = const_cast<uint8_t*>(pub->cur_ctag);
    a.cur.cfixed = const_cast<uint64_t*>(pub->cur_cfixed);
    a.cur.caux = const_cast<uint32_t*>(pub->cur_caux);
    a.cur_heap = pub->cur_heap;
    a.n_ids = pub->n_ids;
    a.n_slots = pub->n_slots;
    a.slot_of_id = pub->slot_of_id;
    a.allow_of_id = tab->allow_of_id;
    a.n_defaults = tab->n_defaults;
    a.default_heap = tab->default_heap;
    a.default_off = tab->default_off;
    a.deferred_room = tab->deferred_room;
    a.frame = frame;
    a.ctl_row = cols->ctl_row;
    a.ctl_off = cols->ctl_off;
    a.ctl_len = cols->ctl_len;
    a.ctl_variant = cols->ctl_variant;
    a.span_perm = span_perm;
    a.n_ctl = n_ctl;
    a.row_begin = row_begin;
    a.ctl_begin = ctl_begin;
    a.outcome = out->outcome;
    a.span_id = out->span_id;
    a.sub_id = out->sub_id;
    a.sub_perm = out->sub_perm;
    a.cap_sub = out->cap_sub;
    a.deferred = out->deferred;
    a.cap_deferred = out->cap_deferred;
    a.reply = out->reply;
    a.cap_reply = out->cap_reply;
    HIPCHK(nxg_launch_route_subscribes(a, c->dscratch, c->stream));
    NxgRsHead h;
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_spans = h.next_ctl - ctl_begin;
    out->n_sub = h.n_sub;
    out->n_deferred = h.n_outcome[NXG_SUB_DEFERRED];
    out->n_replies = h.n_replies;
    out->reply_len = h.reply_bytes;
    for (int o = 0; o < 5; o++) out->n_outcome[o] = h.n_outcome[o];
    out->next_ctl = h.next_ctl;
    out->stopped = h.stopped;
    // (a span behind the final stop was resolved before a path in front of it lowered the stop)
    const uint64_t bad_k = ~(h.bad_inv >> 8 | 0xffull << 56), bad_kind = h.bad_inv & 0xff;
    if (h.bad_inv && bad_k < h.next_ctl) {
        set_err(err, "tab->pub: the current value of span %llu's Id cannot be encoded (%s)",
                (unsigned long long)bad_k,
                bad_kind == 6   ? "nested deeper than NXG_MAX_DEPTH"
                : bad_kind == 2 ? "a container past MAX_VEC, or no child columns"
                                : "unknown tag");
        return false;
    }
    if (out->n_sub > out->cap_sub || out->n_deferred > out->cap_deferred ||
        out->reply_len > out->cap_reply) {
        set_err(err, "subscribe routing needs %llu subscribed ids, %llu deferred spans, %llu reply "
                     "bytes; capacities are %llu, %llu, %llu (NXG_CAPACITY)",
                (unsigned long long)out->n_sub, (unsigned long long)out->n_deferred,
                (unsigned long long)out->reply_len, (unsigned long long)out->cap_sub,
                (unsigned long long)out->cap_deferred, (unsigned long long)out->cap_reply);
        return false;
    }
    return true;
}

// ---- reply routing (subscriber/connection.rs:67-83, 409-541) ------------------------------------
// Replaces process_batch: nxg_route_replies.hip's passes, the dispatch of nxg_dispatch.hip over the
// call's items for the fan-out, one copy of the head, one synchronisation.
bool nxg_route_replies(NxgCtx* c, const NxgReplyTable* tab, const uint8_t* frame,
                       const NxgColumns* cols, uint64_t row_begin, uint64_t ctl_begin,
                       NxgReplyRoute* out, NetidxError* err) {
    // (the argument checks come before any use of the context)
    if (!c || !cols || !out) {
        set_err(err, "null argument");
        return false;
    }
    if (!tab || !tab->subs || !tab->pending) {
        set_err(err, "tab: the table, tab->subs or tab->pending is null");
        return false;
    }
    if (cols->mem != NXG_MEM_DEVICE) {
        set_err(err, "cols->mem: reply routing takes device columns");
        return false;
    }
    if (cols->layout != NXG_LAYOUT_MIXED || !mixed_capable(cols)) {
        set_err(err, "cols->layout: frames with control messages are decoded into MIXED-layout "
                     "columns");
        return false;
    }
    const uint64_t n_rows = cols->n_rows, n_ctl = cols->n_ctl;
    if (row_begin > n_rows) {
        set_err(err, "row_begin %llu is past the batch's %llu rows", (unsigned long long)row_begin,
                (unsigned long long)n_rows);
        return false;
    }
    if (ctl_begin > n_ctl) {
        set_err(err, "ctl_begin %llu is past the batch's %llu control spans",
                (unsigned long long)ctl_begin, (unsigned long long)n_ctl);
        return false;
    }
    const uint64_t rows = n_rows - row_begin, spans = n_ctl - ctl_begin;
    if (rows + spans >= 0xffffffffull) {
        set_err(err, "row_begin / ctl_begin: a call covers fewer than 2^32 rows and spans");
        return false;
    }
    const NxgSubTable* st = tab->subs;
    if (out->cap_spans < n_ctl) {
        set_err(err, "out->cap_spans: outcome[] / span_q[] / span_id[] hold %llu spans, the batch "
                     "%llu", (unsigned long long)out->cap_spans, (unsigned long long)n_ctl);
        return false;
    }
    if (tab->pending->device != c->device) {
        set_err(err, "tab->pending belongs to device %d, the ctx to %d", tab->pending->device,
                c->device);
        return false;
    }
    // every pointer a kernel gets is device memory (a host pointer would fault there)
    struct {
        const void* p;
        bool need;
        const char* name;
    } const ptrs[] = {
        {frame, spans != 0, "frame"},
        {cols->id, rows != 0, "cols->id"},
        {cols->ctl_row, n_ctl != 0, "cols->ctl_row"},
        {cols->ctl_off, spans != 0, "cols->ctl_off"},
        {cols->ctl_len, spans != 0, "cols->ctl_len"},
        {cols->ctl_variant, spans != 0, "cols->ctl_variant"},
        {st->slot_of_id, st->n_ids != 0, "tab->subs->slot_of_id"},
        {st->slot_sub_id, st->n_slots != 0, "tab->subs->slot_sub_id"},
        {st->slot_stream_off, st->n_slots != 0, "tab->subs->slot_stream_off"},
        {st->slot_has_last, st->n_slots != 0, "tab->subs->slot_has_last"},
        {st->stream_chan, false, "tab->subs->stream_chan"},
        {tab->pend_slot, tab->n_pending != 0, "tab->pend_slot"},
        {tab->pend_alive, false, "tab->pend_alive"},
        {out->outcome, n_ctl != 0, "out->outcome"},
        {out->span_q, n_ctl != 0, "out->span_q"},
        {out->span_id, n_ctl != 0, "out->span_id"},
        {out->disp.chan_off, true, "out->disp.chan_off"},
        {out->disp.ent_sub, out->disp.cap_entries != 0, "out->disp.ent_sub"},
        {out->disp.ent_row, out->disp.cap_entries != 0, "out->disp.ent_row"},
        {out->disp.last_row, st->n_slots != 0, "out->disp.last_row"},
        {out->sub_span, out->cap_sub != 0, "out->sub_span"},
        {out->sub_q, out->cap_sub != 0, "out->sub_q"},
        {out->sub_id, out->cap_sub != 0, "out->sub_id"},
        {out->unsub_id, out->cap_unsub != 0, "out->unsub_id"},
        {out->unsub_slot, out->cap_unsub != 0, "out->unsub_slot"},
        {out->reply, out->cap_reply != 0, "out->reply"},
    };
    for (const auto& q : ptrs) {
        if ((q.p || q.need) && !is_device_ptr(q.p)) {
            set_err(err, "%s: %s", q.name, q.p ? "not device memory" : "null");
            return false;
        }
    }
    if (st->n_slots && st->n_chans && !st->stream_chan) {
        // (a table whose every stream list is empty may leave it null: no entry is ever read)
        uint32_t last = 0;
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpy(&last, st->slot_stream_off + st->n_slots, 4, hipMemcpyDeviceToHost));
        if (last) {
            set_err(err, "tab->subs->stream_chan: null");
            return false;
        }
    }
    if (!no_pending(c, err)) return false;
    HIPCHK(hipSetDevice(c->device));
    // the epoch-tagged tables: grown (and cleared) on demand, never cleared per call
    if (!grow(c, c->rr_first_id, st->n_ids, kGrowFirstTable, err) ||
        !grow(c, c->rr_first_q, tab->n_pending, kGrowFirstTable, err))
        return false;
    if (++c->rr_epoch >= (1u << 24)) {  // wrap: stale words could alias epoch 1 again
        c->rr_epoch = 1;
        if (c->rr_first_id)
            HIPCHK(hipMemsetAsync(c->rr_first_id, 0, c->rr_first_id.cap() * 8, c->stream));
        if (c->rr_first_q)
            HIPCHK(hipMemsetAsync(c->rr_first_q, 0, c->rr_first_q.cap() * 8, c->stream));
    }
    const size_t rr = (nxg_rr_scratch_bytes(rows, spans) + 255) & ~size_t(255);
    const size_t need = rr + 64 + nxg_disp_scratch_bytes(rows + spans, st->n_chans);
    if (!ensure_dscratch(c, need, err)) return false;
    NxgRrArgs a{};
    a.subs = *st;
    a.pending = tab->pending->v;
    a.n_pending = tab->n_pending;
    a.pend_slot = tab->pend_slot;
    a.pend_alive = tab->pend_alive;
    a.frame = frame;
    a.id = cols->id;
    a.ctl_row = cols->ctl_row;
    a.ctl_off = cols->ctl_off;
    a.ctl_len = cols->ctl_len;
    a.ctl_variant = cols->ctl_variant;
    a.n_rows = n_rows;
    a.n_ctl = n_ctl;
    a.row_begin = row_begin;
    a.ctl_begin = ctl_begin;
    a.first_id = c->rr_first_id;
    a.first_q = c->rr_first_q;
    a.epoch = c->rr_epoch;
    a.outcome = out->outcome;
    a.span_q = out->span_q;
    a.span_id = out->span_id;
    a.sub_span = out->sub_span;
    a.sub_q = out->sub_q;
    a.sub_id = out->sub_id;
    a.cap_sub = out->cap_sub;
    a.unsub_id = out->unsub_id;
    a.unsub_slot = out->unsub_slot;
    a.cap_unsub = out->cap_unsub;
    a.reply = out->reply;
    a.cap_reply = out->cap_reply;
    a.last_row = out->disp.last_row;
    HIPCHK(nxg_launch_route_replies(a, c->dscratch, c->dscratch + rr, out->disp.chan_off,
                                    out->disp.ent_sub, out->disp.ent_row, out->disp.cap_entries,
                                    c->ncu, c->stream));
    NxgRrHead h;
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_entries = out->disp.n_entries = h.n_entries;
    out->disp.n_unmatched = h.n_unmatched;
    out->n_sub = h.n_sub;
    out->n_unsub = h.n_unsub;
    out->n_replies = h.n_span_replies + h.n_unmatched;
    out->reply_len = h.span_bytes + h.row_bytes;
    for (int o = 0; o < 7; o++) out->n_outcome[o] = h.n_outcome[o];
    out->next_row = h.next_row;
    out->next_ctl = h.next_ctl;
    out->stopped = h.stopped;
    out->pad = 0;
    if (h.bad_inv) {
        const uint64_t bad_k = ~(h.bad_inv >> 8 | 0xffull << 56);
        set_err(err, (h.bad_inv & 0xff) == 1
                         ? "tab->pending: the path of span %llu maps to a request >= tab->n_pending"
                         : "tab->pend_slot: the request of span %llu's path has a slot >= "
                           "tab->subs->n_slots",
                (unsigned long long)bad_k);
        return false;
    }
    if (h.n_entries > out->disp.cap_entries || out->n_sub > out->cap_sub ||
        out->n_unsub > out->cap_unsub || out->reply_len > out->cap_reply) {
        set_err(err, "reply routing needs %llu entries, %llu subscribed spans, %llu unsubscribed ids, "
                     "%llu reply bytes; capacities are %llu, %llu, %llu, %llu (NXG_CAPACITY)",
                (unsigned long long)h.n_entries, (unsigned long long)out->n_sub,
                (unsigned long long)out->n_unsub, (unsigned long long)out->reply_len,
                (unsigned long long)out->disp.cap_entries, (unsigned long long)out->cap_sub,
                (unsigned long long)out->cap_unsub, (unsigned long long)out->cap_reply);
        return false;
    }
    return true;
}

bool nxg_encode_updates_async(NxgCtx* c, const NxgColumns* din, const uint8_t* dheap,
                              uint8_t* dout, uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!c || !din || !dout) {
        set_err(err, "null argument");
        return false;
    }
    if (c->pending.size() >= kStatusRing / 2) {
        set_err(err, "too many in-flight async calls (max %d); call nxg_ctx_sync", kStatusRing / 2);
        return false;
    }
    // the control-span prefix lives in shared ctx scratch: one such encode in flight at a time
    for (auto& p : c->pending)
        if (p.kind == 2 && din->layout == NXG_LAYOUT_MIXED && din->n_ctl) {
            set_err(err, "sync the previous encode before an async encode with control spans");
            return false;
        }
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    const uint32_t seq = c->calls - 1;
    int fast = 0;
    const bool ok = enqueue_encode(c, din, dheap, dout, cap, st, err, &fast);
    if (!end_call(c, err) || !ok) return false;
    c->pending.push_back({2, fast, nullptr, 0, const_cast<NxgColumns*>(din), len_out, cap, st,
                          slot, 0, dheap, dout, seq});
    return true;
}

bool nxg_encode_frames(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                       uint64_t cap, uint64_t* len_out, uint64_t* chunk_len_out,
                       uint64_t cap_chunks, uint64_t* n_chunks, NetidxError* err) {
    if (!out || !n_chunks || (cap_chunks && !chunk_len_out)) {
        set_err(err, "null argument");
        return false;
    }
    uint64_t total = 0;
    if (!encode_impl(c, in, heap, out, cap, &total, err)) return false;
    if (len_out) *len_out = total;
    uint64_t ch[2];
    uint64_t k = 0;
    if (total == 0) {
        k = 0;
    } else if (total <= kMaxBatch) {
        ch[k++] = total;
    } else {
        if (!c->last_split) {
            set_err(err, "frame split: the encoder recorded no boundary for a %llu-byte batch",
                    (unsigned long long)total);
            return false;
        }
        const uint64_t c1 = c->last_split - 1;
        // the next cut is before the first message ending past MAX_BATCH + c1 (channel.rs:187)
        if (total > kMaxBatch + c1) {
            set_err(err, "frame split: a %llu-byte batch needs more than one cut (the reference "
                         "then cuts before every message); split the batch or use "
                         "nxg_frame_split with the message lengths", (unsigned long long)total);
            return false;
        }
        ch[k++] = c1;
        ch[k++] = total - c1;
    }
    if (k > cap_chunks) {
        set_err(err, "frame split: %llu frames, capacity %llu", (unsigned long long)k,
                (unsigned long long)cap_chunks);
        return false;
    }
    for (uint64_t i = 0; i < k; i++) chunk_len_out[i] = ch[i];
    *n_chunks = k;
    return true;
}

// ---- byte-range decode (multi-GPU) ---------------------------------------------------------------
bool nxg_decode_range(NxgCtx* c, const uint8_t* dframe, uint64_t W, uint64_t begin, uint64_t end,
                      NxgColumns* out, NxgRange* rng, NetidxError* err) {
    if (!c || !out || !rng || (!dframe && W)) {
        set_err(err, "null argument");
        return false;
    }
    if (begin > end || end > W) {
        set_err(err, "bad range [%llu, %llu) of a %llu-byte frame", (unsigned long long)begin,
                (unsigned long long)end, (unsigned long long)W);
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (out->mem != NXG_MEM_DEVICE || !is_device_ptr(dframe)) {
        set_err(err, "range decode needs a device frame and device columns");
        return false;
    }
    if (!set_device(c, err)) return false;
    memset(rng, 0, sizeof *rng);
    rng->begin = begin;
    rng->end = end;
    if (begin == end) {  // an empty range: the chain passes through; linked as identity
        rng->entry = rng->exit = ~0ull;
        rng->ok = 1;
        return true;
    }
    const uint64_t R = end - begin;
    DevStatus* st;
    uint32_t slot;
    if (!begin_call(c, &st, &slot, err)) return false;
    bool ok = ensure_tstat(c, nxg_dec_f64r_groups(R), err) &&
              ensure_rdesc(c, 16 * nxg_dec_f64r_tiles(R), err);
    if (ok) {
        const hipError_t e = nxg_launch_dec_f64r(dframe, W, begin, end, out->id, out->fixed,
                                                 out->cap_rows, c->rdesc, c->tstat, c->epoch,
                                                 c->f64r_flags, st, c->stream);
        if (e != hipSuccess) {
            set_err(err, "range decode launch: %s", hipGetErrorString(e));
            ok = false;
        }
    }
    if (!end_call(c, err) || !ok) return false;
    const uint64_t nt = nxg_dec_f64r_tiles(R);
    uint8_t d0[16], dl[16];
    HIPCHK(hipMemcpyAsync(c->hst + slot, st, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(d0, c->rdesc, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(dl, c->rdesc + 16 * (nt - 1), 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const DevStatus& h = c->hst[slot];
    if (h.timeout) {
        set_err(err, "device look-back watchdog expired");
        return false;
    }
    // (a copy: later attempts take other ring slots)
    const DevStatus h0 = h;
    c->last = h0;
    bool declined = h0.fast_fail != 0;
    if (declined && (h0.irregular & 3u) == 1u) {
        // record lengths that vary record to record (ids in any order: a batch updating an
        // arbitrary subset of a publisher's values): the single-pass decoder in range mode
        DevStatus* st2;
        uint32_t slot2;
        if (!begin_call(c, &st2, &slot2, err)) return false;
        bool ok2 = ensure_tstat(c, nxg_dec_f64x_groups(R), err);
        if (ok2) {
            const hipError_t e = nxg_launch_dec_f64x_range(dframe, W, begin, end, out->id,
                                                           out->fixed, out->cap_rows, c->tstat,
                                                           c->epoch, st2, c->stream);
            if (e != hipSuccess) {
                set_err(err, "range decode launch: %s", hipGetErrorString(e));
                ok2 = false;
            }
        }
        if (!end_call(c, err) || !ok2) return false;
        HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const DevStatus& h2 = c->hst[slot2];
        c->last = h2;
        if (!h2.fast_fail && h2.diag[2] && h2.diag[3]) {
            rng->entry = begin + h2.diag[2] - 1;
            rng->exit = begin + h2.diag[3] - 1;
            rng->n_rows = h2.n_rows;
            rng->ok = 1;
            rng->err_kind = h2.capacity ? NXG_CAPACITY : 0;
            out->n_rows = h2.n_rows;
            out->layout = NXG_LAYOUT_F64;
            return true;
        }
    }
    if (declined && mixed_capable(out) && R < (1ull << 32)) {
        // not an f64 frame: the fast mixed decoder in range mode (frames of short Updates and
        // Heartbeats; anything it declines is ok = 0, for the caller to decode whole)
        DevStatus* st2;
        uint32_t slot2;
        if (!begin_call(c, &st2, &slot2, err)) return false;
        const ColsDesc d = desc_of(out);
        bool ok2 = ensure_glws(c, nxg_fmx_scratch_bytes(R), err);
        if (ok2) {
            const hipError_t e = nxg_launch_dec_fmx_range(dframe, W, begin, end, d,
                                                          c->glws,
                                                          c->wgs_fmx, st2, c->stream);
            if (e != hipSuccess) {
                set_err(err, "range decode launch: %s", hipGetErrorString(e));
                ok2 = false;
            }
        }
        if (!end_call(c, err) || !ok2) return false;
        HIPCHK(hipMemcpyAsync(c->hst + slot2, st2, sizeof(DevStatus), hipMemcpyDeviceToHost,
                              c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const DevStatus& h2 = c->hst[slot2];
        c->last = h2;
        if (h2.fast_fail || h2.path != 4 || !h2.diag[2] || !h2.diag[3]) {  // ok = 0
            if (h2.capacity) rng->err_kind = NXG_CAPACITY;  // declined: the columns are short
            return true;
        }
        rng->entry = begin + h2.diag[2] - 1;
        rng->exit = begin + h2.diag[3] - 1;
        rng->n_rows = h2.n_rows;
        rng->ok = 1;
        out->n_rows = h2.n_rows;
        out->n_children = h2.n_children;
        out->n_ctl = h2.n_ctl;
        out->n_heartbeat = h2.n_heartbeat;
        out->layout = NXG_LAYOUT_MIXED;
        return true;
    }
    if (declined) return true;  // ok = 0: not a range these decoders take
    // Desc: base u64 | count u16 | ks u16 | x u16 | entry u8 | mode u8 (nxg_decode_f64_run.hip)
    uint16_t xl;
    memcpy(&xl, dl + 12, 2);
    rng->entry = begin + d0[14];
    rng->exit = begin + (nt - 1) * nxg_dec_f64r_tile_bytes() + xl;
    rng->n_rows = h.n_rows;
    rng->ok = 1;
    rng->err_kind = h.capacity ? NXG_CAPACITY : 0;
    out->n_rows = h.n_rows;
    out->layout = NXG_LAYOUT_F64;
    return true;
}

bool nxg_range_link(const NxgRange* r, uint32_t n, uint64_t W, uint64_t* row_off, uint32_t* bad,
                    NetidxError* err) {
    if (!r || (n && !row_off)) {
        set_err(err, "null argument");
        return false;
    }
    uint64_t at = 0, rows = 0;  // where the chain is, rows so far
    uint64_t expect_begin = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (r[i].begin != expect_begin || r[i].end < r[i].begin || !r[i].ok) {
            if (bad) *bad = i;
            set_err(err, "range %u is not the next contiguous, decoded range", i);
            return false;
        }
        expect_begin = r[i].end;
        row_off[i] = rows;
        if (r[i].begin == r[i].end) continue;  // empty: the chain passes through
        if (r[i].entry != at) {
            if (bad) *bad = i;
            set_err(err, "range %u enters the chain at %llu, its predecessor leaves at %llu", i,
                    (unsigned long long)r[i].entry, (unsigned long long)at);
            return false;
        }
        at = r[i].exit;
        rows += r[i].n_rows;
    }
    if (expect_begin != W || at != W) {
        if (bad) *bad = n ? n - 1 : 0;
        set_err(err, "the ranges cover [0, %llu) and the chain ends at %llu; the frame has %llu "
                     "bytes", (unsigned long long)expect_begin, (unsigned long long)at,
                (unsigned long long)W);
        return false;
    }
    return true;
}

// ---- one share of a frame's rows (nxg_decode_sharded's fallback) --------------------------------
// The frame decoded whole (every decoder in turn, as nxg_decode_updates), into ctx-owned device
// columns sized `shares` times the caller's (each rank's share should fit its own columns), or to
// the frame's totals when that is short; then rows [N*share/shares, N*(share+1)/shares) with their
// children and the control spans before them (the last share: also those after the last row)
// into `out`, re-based (nxg_share.hip).
bool nxg_decode_share(NxgCtx* c, const uint8_t* dframe, uint64_t W, uint32_t share,
                      uint32_t shares, NxgColumns* out, uint64_t* row_off, NxgStatus* ust,
                      NetidxError* err) {
    if (!c || !out || (!dframe && W) || shares == 0 || share >= shares) {
        set_err(err, "bad argument (share %u of %u)", share, shares);
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (W >= (1ull << 40)) {
        set_err(err, "frame too large (%llu bytes)", (unsigned long long)W);
        return false;
    }
    if (out->mem != NXG_MEM_DEVICE || (W && !is_device_ptr(dframe))) {
        set_err(err, "share decode needs a device frame and device columns");
        return false;
    }
    if (!set_device(c, err)) return false;
    if (row_off) *row_off = 0;
    // the whole-frame columns: the caller's shape, `shares` times its capacities (at most the
    // frame's bounds, include/nxg_codec.h), grown to the frame's totals after a capacity miss
    auto times = [&](uint64_t x, uint64_t bound) {
        return std::max<uint64_t>(1, std::min<uint64_t>(x > bound / shares ? bound : x * shares, bound));
    };
    NxgColumns like = *out;
    like.cap_rows = times(out->cap_rows, W / 4 + 1);
    like.cap_children = times(out->cap_children, W + 1);
    like.cap_ctl = times(out->cap_ctl, W / 2 + 1);
    NxgColumns v{};
    NxgStatus s{};
    for (int attempt = 0;; attempt++) {
        if (!ensure_dcols(c, &like, err)) return false;
        v = staged_view(c, &like);
        DevStatus* st;
        uint32_t slot;
        if (!begin_call(c, &st, &slot, err)) return false;
        int fast = FAST_NONE;
        const bool ok = enqueue_dec_fast(c, dframe, W, &v, st, &fast, err);
        if (!end_call(c, err) || !ok) return false;
        if (!finish_decode(c, dframe, W, &v, fast, st, slot, &s, err)) return false;
        if (s.err_kind != NXG_CAPACITY || attempt == 2) break;
        const uint64_t r = std::min<uint64_t>(std::max(s.n_rows, 2 * like.cap_rows), W / 4 + 1);
        const uint64_t k = std::min<uint64_t>(std::max(s.n_children, 2 * like.cap_children), W + 1);
        const uint64_t q = std::min<uint64_t>(std::max(s.n_ctl, 2 * like.cap_ctl), W / 2 + 1);
        if (r == like.cap_rows && k == like.cap_children && q == like.cap_ctl) break;
        like.cap_rows = r;
        like.cap_children = k;
        like.cap_ctl = q;
    }
    NxgStatus o{};
    o.path = s.path;
    o.err_kind = s.err_kind;
    o.err_offset = s.err_offset;
    if (s.err_kind) {  // the frame fails as a whole (connection.rs:228-231): no rows in any share
        out->n_rows = out->n_children = out->n_ctl = out->n_heartbeat = 0;
        if (ust) *ust = o;
        return true;
    }
    const uint64_t N = s.n_rows;
    const uint64_t r0 = (uint64_t)((unsigned __int128)N * share / shares);
    const uint64_t r1 = (uint64_t)((unsigned __int128)N * (share + 1) / shares);
    const bool last = share + 1 == shares;
    const bool f64_rows = s.path == 1 || !mixed_capable(&v);  // tag / children not written
    ColsDesc src = desc_of(&v);
    src.n_rows = N;
    src.n_children = f64_rows ? 0 : s.n_children;
    src.n_ctl = f64_rows ? 0 : s.n_ctl;
    if (f64_rows) src.tag = nullptr;
    uint64_t c0 = 0, c1 = 0, k0 = 0, k1 = 0;
    if (!ensure_escratch(c, 8, err)) return false;
    if (!f64_rows && (src.n_children || src.n_ctl)) {
        uint64_t b[4];
        HIPCHK(nxg_launch_share_bounds(src, r0, r1, c->escratch, c->stream));
        HIPCHK(hipMemcpyAsync(b, c->escratch, sizeof b, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c0 = std::min<uint64_t>(b[0], src.n_children);
        c1 = std::min<uint64_t>(b[1], src.n_children);
        k0 = std::min<uint64_t>(b[2], src.n_ctl);
        k1 = last ? src.n_ctl : std::min<uint64_t>(b[3], src.n_ctl);
    }
    const uint64_t nr = r1 - r0, nc = c1 - c0, nk = k1 - k0;
    if (nr > out->cap_rows || nc > out->cap_children || nk > out->cap_ctl ||
        ((nc || nk) && !mixed_capable(out))) {
        o.err_kind = (nc || nk) && !mixed_capable(out) ? NXG_NOT_F64 : NXG_CAPACITY;
        o.n_rows = nr;
        o.n_children = nc;
        o.n_ctl = nk;
        out->n_rows = out->n_children = out->n_ctl = out->n_heartbeat = 0;
        if (ust) *ust = o;
        return true;
    }
    ColsDesc dst = desc_of(out);
    if (f64_rows) dst.tag = nullptr;
    HIPCHK(nxg_launch_share_copy(src, dst, r0, nr, c0, nc, k0, nk, c->escratch + 4, c->stream));
    uint64_t hb = 0;
    HIPCHK(hipMemcpyAsync(&hb, c->escratch + 4, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_rows = nr;
    out->n_children = nc;
    out->n_ctl = nk;
    out->n_heartbeat = hb;
    out->layout = f64_rows ? NXG_LAYOUT_F64 : NXG_LAYOUT_MIXED;
    o.n_rows = nr;
    o.n_children = nc;
    o.n_ctl = nk;
    o.n_heartbeat = hb;
    if (row_off) *row_off = r0;
    if (ust) *ust = o;
    return true;
}

// ---- host framing ------------------------------------------------------------------------

// WriteChannel::queue_send (channel.rs:177-202) + try_flush (237-257). `boundries` holds chunk
// LENGTHS. A new boundary is recorded when (buf_len - last boundary length) + len > MAX_BATCH,
// i.e. the comparison uses the last chunk's length, not the sum (channel.rs:187-190).
int64_t nxg_frame_split(const uint64_t* msg_len, uint64_t n_msgs, uint64_t* chunk_len_out,
                        uint64_t cap_chunks) {
    const uint64_t MAX_BATCH = 0x3FFFFFFF;
    uint64_t buf_len = 0, sum_b = 0, last_b = 0, nb = 0;
    for (uint64_t i = 0; i < n_msgs; i++) {
        const uint64_t len = msg_len[i];
        if (len > MAX_BATCH) return -1;
        if ((buf_len - (nb ? last_b : 0)) + len > MAX_BATCH) {
            const uint64_t b = buf_len - sum_b;
            if (nb >= cap_chunks) return -1;
            chunk_len_out[nb++] = b;
            sum_b += b;
            last_b = b;
        }
        buf_len += len;
    }
    if (buf_len > sum_b) {
        if (nb >= cap_chunks) return -1;
        chunk_len_out[nb++] = buf_len - sum_b;
    }
    return (int64_t)nb;
}

// flush_buf (channel.rs:107-126)
void nxg_frame_header(uint32_t payload_len, bool encrypted, uint8_t out[4]) {
    const uint32_t v = encrypted ? (payload_len | 0x80000000u) : payload_len;
    out[0] = (uint8_t)(v >> 24);
    out[1] = (uint8_t)(v >> 16);
    out[2] = (uint8_t)(v >> 8);
    out[3] = (uint8_t)v;
}

// read_task (channel.rs:389-398): hdr > LEN_MASK => encrypted, len = hdr & LEN_MASK
uint32_t nxg_frame_parse_header(const uint8_t* buf, uint64_t avail, uint32_t* payload_len,
                                bool* encrypted) {
    if (avail < 4) return 0;
    const uint32_t hdr = ((uint32_t)buf[0] << 24) | ((uint32_t)buf[1] << 16) |
                         ((uint32_t)buf[2] << 8) | buf[3];
    *encrypted = hdr > 0x7FFFFFFFu;
    *payload_len = hdr & 0x7FFFFFFFu;
    return 4;
}

// ---- read_task's frame assembly (channel.rs:379-443) -------------------------------------------
struct NxgFrameReader {
    std::vector<uint8_t> buf;  // bytes read from the socket, not yet handed out
    size_t head = 0;           // start of the unconsumed bytes
};

NxgFrameReader* nxg_frame_reader_new(NetidxError* err) {
    try {
        return new NxgFrameReader();
    } catch (...) {
        set_err(err, "out of memory");
        return nullptr;
    }
}

void nxg_frame_reader_free(NxgFrameReader* r) { delete r; }

bool nxg_frame_reader_push(NxgFrameReader* r, const uint8_t* data, uint64_t len,
                           NetidxError* err) {
    if (!r || (len && !data)) {
        set_err(err, "null argument");
        return false;
    }
    // drop what was handed out before growing (payload pointers from _next end here)
    if (r->head) {
        r->buf.erase(r->buf.begin(), r->buf.begin() + (ptrdiff_t)r->head);
        r->head = 0;
    }
    try {
        r->buf.insert(r->buf.end(), data, data + len);
    } catch (...) {
        set_err(err, "out of memory");
        return false;
    }
    return true;
}

int nxg_frame_reader_next(NxgFrameReader* r, const uint8_t** payload, uint64_t* len,
                          NetidxError* err) {
    if (!r || !payload || !len) {
        set_err(err, "null argument");
        return -1;
    }
    const uint64_t avail = r->buf.size() - r->head;
    uint32_t plen = 0;
    bool enc = false;
    if (!nxg_frame_parse_header(r->buf.data() + r->head, avail, &plen, &enc)) return 0;
    if (avail - 4 < plen) return 0;  // "less than batch len, reading more"
    if (enc) {  // no security context here (krb5 is out of scope): channel.rs:420-422
        set_err(err, "encryption is not supported");
        return -1;
    }
    *payload = r->buf.data() + r->head + 4;
    *len = plen;
    r->head += 4 + (size_t)plen;
    return 1;
}

uint64_t nxg_frame_reader_buffered(const NxgFrameReader* r) {
    return r ? r->buf.size() - r->head : 0;
}

}  // extern "C"
