// nxg_internal.h -- structures shared by the kernels and the host dispatch layer (not ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nxg_codec.h"

// Per-call device status block (a ring slot, zeroed kStatusRing/2 = 512 calls ahead: zero_status).
struct DevStatus {
    uint64_t n_rows, n_children, n_ctl, n_heartbeat;  // totals written by the last tile
    uint32_t err_kind;                                 // first error in wire order
    uint32_t path;
    uint64_t err_offset;
    uint32_t fast_fail;  // homogeneous-f64 kernel rejected the frame (=> general path)
    uint32_t timeout;    // a bounded spin expired (protocol bug); reported as NXG_TIMEOUT
    uint32_t capacity;   // a column overflowed its capacity
    uint32_t runs_valid;   // general decode: runs on the true chain, 0 = all (resolve -> emit)
    uint64_t total_bytes;  // encode: bytes written
    uint32_t nonf64;       // general path ran into content that F64-only columns cannot hold
    // f64 run decode: bit 0 record lengths vary too often (=> the single-pass decoder), bit 1
    // not an f64 frame (=> the mixed decoders); sequential-id decode: bit 2 the ids do not count
    // up by one (=> the length-run decoder)
    uint32_t irregular;
    // general decode: first error as ~(offset << 8 | kind), combined with atomicMax (0 = none)
    uint64_t err_key;
    // encode: 1 + the start offset of the message that holds byte MAX_BATCH, i.e. where
    // WriteChannel::queue_send records its first frame boundary (channel.rs:187-191); 0 = none
    uint64_t split_start;
    // diagnostics (general decode): 0 redo tiles, 1 look-back fallbacks, 2 repair rounds,
    // 3 lane walks, 4 speculation attempts, 5 tiles without a speculated entry,
    // 6 exhausted (budgeted) walks, 7 work-list entries of the emit pass. The fast mixed decode
    // (path 4) uses diag[7] as its resolve pass's arrival counter (zeroed with the slot).
    unsigned long long diag[8];
};
static_assert(sizeof(DevStatus) == 160, "DevStatus layout");

// Look-back status granule (one 8-byte word, written with one sc1 store):
//   bits 63:62 flag (1 aggregate, 2 inclusive), 61:44 call epoch, 43:0 value.
// A word whose epoch differs from the current call's reads as "not ready", so the status
// arrays need no per-call memset (they are zeroed only when the 18-bit epoch wraps).
constexpr uint64_t kFlagAgg = 1ull << 62;
constexpr uint64_t kFlagInc = 2ull << 62;
constexpr uint64_t kFlagMask = 3ull << 62;
constexpr int kEpochShift = 44;
constexpr uint64_t kEpochMax = (1ull << 18) - 1;
constexpr uint64_t kValMask = (1ull << kEpochShift) - 1;
constexpr uint64_t kMaxBatch = 0x3FFFFFFF;  // MAX_BATCH, netidx/src/channel.rs:34
constexpr uint64_t kMaxVecBytes = 2ull * 1024 * 1024 * 1024;  // MAX_VEC, pack.rs:917
constexpr uint64_t kBatchItemSize = 24;  // size_of::<BatchItem>() (logfile/mod.rs:188; unpinned)
// encode: note the message [pos, pos + len) if it holds byte MAX_BATCH (exactly one does, in a
// frame longer than MAX_BATCH)
__device__ inline void note_split(DevStatus* st, uint64_t pos, uint64_t len) {
    if (pos <= kMaxBatch && kMaxBatch < pos + len) st->split_start = pos + 1;
}
__host__ __device__ inline uint64_t lb_word(uint64_t flag, uint32_t epoch, uint64_t v) {
    return flag | ((uint64_t)epoch << kEpochShift) | (v & kValMask);
}
__host__ __device__ inline uint64_t lb_flag(uint64_t w, uint32_t epoch) {
    return ((w >> kEpochShift) & kEpochMax) == epoch ? (w & kFlagMask) : 0ull;
}

// ---- general decode geometry (nxg_decode_gen.hip) ----
namespace gdec2 {
constexpr int TPB = 256;            // 4 independent waves per workgroup, one run each
constexpr int CH = 64;              // bytes per lane
constexpr uint32_t TILE = 64 * CH;  // 4 KiB per tile
constexpr uint32_t IMG = TILE + 1024;  // LDS image: tile + 1 KiB look-ahead
constexpr int MAX_RUNS = 8192;      // runs (waves) per pass
constexpr int RUN_WORDS = 8;        // per-run summary words
}  // namespace gdec2

// ---- f64 encode geometry ----
namespace f64enc {
constexpr int LB_U = 1;                 // look-back window rows (64 tiles each); wider measured slower
constexpr int TPB = 256;
constexpr int RPT = 4;                 // records per thread
constexpr int TILE = TPB * RPT;        // records per tile
constexpr int MAXB = TILE * 15 + 32;   // staging bytes (f64 records <= 15 B for ids < 2^28)
}  // namespace f64enc

// Polls of an unpublished look-back predecessor before its aggregate is computed by the waiting
// workgroup itself (self-help look-backs); NXG_LOOKBACK_PATIENCE at context creation (tests: 0,
// every unpublished predecessor computed).
extern thread_local uint32_t nxg_patience;

// launchers (each defined next to its kernel)
struct ColsDesc;
// Every launcher takes the call's status slot `st` and `zst`, the slot that the call 512 calls
// later will use (nxg_take_zero_slot()). Block 0 of the kernel that receives it zeroes `zst` on
// entry, so the ring needs no per-call memset; a call that launches no such kernel (an empty
// frame or batch) has the host zero it instead (nxg_zero_used, nxg_ctx.cpp).
__device__ inline void zero_status(DevStatus* zst) {
    if (zst && blockIdx.x == 0 && threadIdx.x == 0) *zst = DevStatus{};
}
extern thread_local DevStatus* nxg_zero_slot;  // host side: passed through to the kernels
extern thread_local bool nxg_zero_used;         // a kernel of this call zeroes nxg_zero_slot
inline DevStatus* nxg_take_zero_slot() {
    nxg_zero_used = true;
    return nxg_zero_slot;
}
// status gather (nxg_status.hip): ring slots s0, s0 + 1, ... (n of them, modulo `ring`) copied to
// the pinned host mirror, whose device address is `hst_dev`, in stream order
hipError_t nxg_launch_status_gather(const DevStatus* dst, DevStatus* hst_dev, uint32_t s0,
                                    uint32_t n, uint32_t ring, hipStream_t s);
// f64 decode of any f64 frame in one pass (nxg_decode_f64_x.hip): `tstat` holds
// nxg_dec_f64x_groups(W) epoch-tagged words (no initialisation needed).
uint64_t nxg_dec_f64x_groups(uint64_t W);
// the records that start in [begin, end) of a W-byte frame; entry / exit (+1, relative to begin)
// in DevStatus.diag[2] / diag[3]
hipError_t nxg_launch_dec_f64x_range(const uint8_t* wire, uint64_t W, uint64_t begin,
                                     uint64_t end, uint64_t* oid, uint64_t* oval, uint64_t cap,
                                     uint64_t* tstat, uint32_t epoch, DevStatus* st,
                                     hipStream_t s);
hipError_t nxg_launch_dec_f64x(const uint8_t* wire, uint64_t W, uint64_t* oid, uint64_t* oval,
                               uint64_t cap, uint64_t* tstat, uint32_t epoch, DevStatus* st,
                               hipStream_t s);
// f64 decode of a frame whose ids count up by one (nxg_decode_f64_seq.hip): one launch, no scratch.
// Declines with fast_fail + DevStatus.irregular bit 1 (not f64) or bit 2 (another f64 frame).
uint64_t nxg_dec_f64s_groups(uint64_t W);
hipError_t nxg_launch_dec_f64s(const uint8_t* wire, uint64_t W, uint64_t* oid, uint64_t* oval,
                               uint64_t cap, DevStatus* st, DevStatus* zst, hipStream_t s);
// A backlog of such frames in one launch of a resident grid (nxg_f64s_backlog_kernel): frames
// shorter than the Infinity Cache only (nxg_f64s_backlog_takes), at most kF64sBacklogMax, each with
// its own status slot and zero slot. kF64sReuse marks a frame that writes the columns of an earlier
// frame of the launch; that is allowed only where both have the same oid, oval, cap and W.
constexpr uint32_t kF64sBacklogMax = 32;
constexpr uint32_t kF64sReuse = 1;
struct NxgF64sFrame {
    const uint8_t* wire;
    uint64_t W;
    uint64_t* oid;
    uint64_t* oval;
    uint64_t cap;
    DevStatus* st;
    DevStatus* zst;
    uint32_t tiles_per_wave;  // nxg_f64s_tiles_per_wave(W, 4 * the launch's workgroups)
    uint32_t flags;
};
struct NxgF64sBacklog {
    uint32_t n, pad;
    NxgF64sFrame f[kF64sBacklogMax];
};
static_assert(sizeof(NxgF64sBacklog) <= 2560, "kernel arguments of the backlog kernel");
bool nxg_f64s_backlog_takes(uint64_t W);
uint32_t nxg_f64s_tiles_per_wave(uint64_t W, uint32_t waves);
int nxg_f64s_backlog_wgs(int ncu);
hipError_t nxg_launch_dec_f64s_backlog(const NxgF64sBacklog& b, int wgs, hipStream_t s);
// f64 decode by length runs (nxg_decode_f64_run.hip): probe + emit launches. `desc` holds 16 bytes
// per tile (nxg_dec_f64r_tiles(W)), `tstat` nxg_dec_f64r_groups(W) epoch-tagged words. Sets
// DevStatus.irregular (and fast_fail) for frames whose record lengths vary record to record.
uint64_t nxg_dec_f64r_tiles(uint64_t W);
uint64_t nxg_dec_f64r_tile_bytes();
uint64_t nxg_dec_f64r_groups(uint64_t W);
// Records starting in [begin, end) of a W-byte frame (the whole frame: begin 0, end W).
hipError_t nxg_launch_dec_f64r(const uint8_t* wire, uint64_t W, uint64_t begin, uint64_t end,
                               uint64_t* oid, uint64_t* oval, uint64_t cap, void* desc,
                               uint64_t* tstat, uint32_t epoch, uint32_t flags, DevStatus* st,
                               hipStream_t s);
// A stream of whole frames (nxg_decode_frames_async): probe(0), then per frame one fused launch
// of emit(j) and probe(j + 1). Consecutive frames need different `desc` arrays; each frame has its
// own status slot and zero slot (`zst`, zeroed by its probe).
struct NxgF64rFrame {
    const uint8_t* wire;
    uint64_t W;
    uint64_t* oid;
    uint64_t* oval;
    uint64_t cap;
    void* desc;
    uint32_t epoch;
    DevStatus* st;
    DevStatus* zst;
};
hipError_t nxg_launch_dec_f64r_stream(const NxgF64rFrame* fr, uint32_t n, uint64_t* tstat,
                                      uint32_t flags, hipStream_t s);
uint64_t nxg_enc_f64_tiles(uint64_t n);  // tiles (and tstat words) of an f64 encode
hipError_t nxg_launch_enc_f64(const uint64_t* id, const uint64_t* val, uint64_t n, uint8_t* out,
                              uint64_t cap, uint64_t* tstat, uint32_t epoch, DevStatus* st,
                              int grid, hipStream_t s);
// f64 encode of a batch whose ids count up by one (nxg_encode_f64_seq.hip): one launch, no
// look-back; declines with fast_fail + DevStatus.irregular bit 2 (out NULL: sizing only)
uint64_t nxg_enc_f64s_groups(uint64_t n);
hipError_t nxg_launch_enc_f64s(const uint64_t* id, const uint64_t* val, uint64_t n, uint8_t* out,
                               uint64_t cap, DevStatus* st, hipStream_t s);
// the type-partitioned view (nxg_partition.hip): count + scan + offsets + place launches;
// `scratch` holds nxg_part_scratch_bytes(n) bytes; *off_out = the per-tag offsets (device, 257)
uint64_t nxg_part_scratch_bytes(uint64_t n);
hipError_t nxg_launch_partition(const uint8_t* tag, const uint64_t* fixed, const uint32_t* aux,
                                uint64_t n, uint8_t* scratch, uint32_t* rank, uint32_t* row_of,
                                uint64_t* dfixed, uint32_t* daux, uint64_t** off_out,
                                hipStream_t s);
uint64_t nxg_enc_general_tiles(uint64_t n);  // tiles (and tstat words) of a general encode
// arch_base > 0: archive-batch rows after an arch_base-byte count header (nxg_encode_general.hip)
// writes: To::Write rows from cols.wflags / cols.wid (nxg_encode_writes; arch_base 0)
hipError_t nxg_launch_enc_general(const ColsDesc& cols, const uint8_t* heap, uint8_t* out,
                                  uint64_t cap, uint64_t* scratch, uint64_t* tstat,
                                  uint32_t epoch, DevStatus* st, int grid, hipStream_t s,
                                  uint64_t arch_base = 0, bool writes = false);
// general decode: count + resolve + emit + fix. `lws` holds nxg_dec_gen_scratch_bytes(W) bytes
// (64 u32 lane words per tile, then the emit pass's work list), `runs` gdec2::MAX_RUNS *
// RUN_WORDS u64, `base` gdec2::MAX_RUNS * 4 u64; none needs zeroing.
uint64_t nxg_dec_gen_tiles(uint64_t W);
uint64_t nxg_dec_gen_scratch_bytes(uint64_t W);
// to: the frame is a To stream (nxg_decode_writes); `cols` then needs the mixed layout and
// wflags / wid.
hipError_t nxg_launch_dec_gen(const uint8_t* wire, uint64_t W, const ColsDesc& cols, uint32_t* lws,
                              uint64_t* runs, uint64_t* base, int wgs, DevStatus* st,
                              hipStream_t s, bool to = false);
int nxg_dec_gen_wgs(int ncu);
// fast mixed decode (nxg_decode_mixed.hip): frames of Update messages shorter than 128 bytes with
// flat values; sets fast_fail for anything else. `scratch`: nxg_fmx_scratch_bytes(W), no zeroing.
uint64_t nxg_fmx_scratch_bytes(uint64_t W);
void nxg_fmx_wgs(int ncu, int* wgs);  // persistent grid sizes (count, emit)
// lean_count: the count pass from one-byte-prefix Update candidates only, then a recount of the
// tiles where that found no chain from every candidate kind (DevStatus.diag[5] counts them, with
// the resolve pass's recounts)
hipError_t nxg_launch_dec_fmx(const uint8_t* wire, uint64_t W, const ColsDesc& cols,
                              uint8_t* scratch, const int* wgs, DevStatus* st, hipStream_t s,
                              bool lean_count = false);
// the messages that start in [begin, end) of a W-byte frame (rows etc. from 0, text / control
// offsets in frame bytes); entry / exit (+1, relative to begin) in DevStatus.diag[2] / diag[3]
hipError_t nxg_launch_dec_fmx_range(const uint8_t* wire, uint64_t W, uint64_t begin, uint64_t end,
                                    const ColsDesc& cols, uint8_t* scratch, const int* wgs,
                                    DevStatus* st, hipStream_t s, bool lean_count = false);
// fast To decode (nxg_decode_writes_fast.hip): frames of Writes with flat values, Unsubscribes and
// Subscribes of at most 256 bytes; sets fast_fail for anything else (and for columns too small).
// `scratch`: nxg_wfast_scratch_bytes(W), no zeroing. Only frames nxg_wfast_takes(W) accepts.
uint64_t nxg_wfast_scratch_bytes(uint64_t W);
bool nxg_wfast_takes(uint64_t W);
hipError_t nxg_launch_dec_wfast(const uint8_t* wire, uint64_t W, const ColsDesc& cols,
                                uint8_t* scratch, DevStatus* st, hipStream_t s);
// subscriber dispatch (nxg_dispatch.hip): `scratch` holds nxg_disp_scratch_bytes(n, n_chans)
// bytes (no initialisation needed); `unmatched` one u64. item_slot (reply routing,
// nxg_route_replies.hip): row i is an item whose slot is item_slot[i] (NXG_NO_SLOT: no entries);
// no Id is looked up, nothing counts as unmatched and last_row is neither cleared nor written.
uint64_t nxg_disp_scratch_bytes(uint64_t n, uint32_t n_chans);
hipError_t nxg_launch_dispatch(const NxgSubTable& tb, const uint64_t* id, uint64_t n,
                               uint8_t* scratch, uint64_t* chan_off, uint64_t* ent_sub,
                               uint64_t* ent_row, uint64_t cap, uint64_t* last_row,
                               uint64_t* unmatched, int ncu, hipStream_t s,
                               const uint8_t* row_mode = nullptr,
                               const uint32_t* to_client = nullptr,
                               const uint32_t* item_slot = nullptr);
// publisher commit (nxg_publish.hip): stage 1 counts slots and sets flags (dup, changed,
// unsupported: three u32 at nxg_pub_flags(scratch)); stage 2 routes the UpdateChanged rows
// (mode array for nxg_launch_dispatch, or null when the kinds route as they are).
struct NxgPubBatch {
    const uint64_t* id;
    const uint8_t* tag;
    const uint64_t* fixed;
    const uint32_t* aux;
    const uint8_t* ctag;  // the batch's children (Array/Map/Error(Value) elements)
    const uint64_t* cfixed;
    const uint32_t* caux;
    const uint8_t* heap;
    const uint8_t* kind;
    uint64_t n_rows;
};
uint64_t nxg_pub_scratch_bytes(uint64_t n, uint64_t n_slots);
hipError_t nxg_launch_pub_stage1(const NxgPubTable& tb, const NxgPubBatch& b, uint8_t* scratch,
                                 int ncu, hipStream_t s);
const uint32_t* nxg_pub_flags(uint8_t* scratch);
hipError_t nxg_launch_pub_stage2(const NxgPubTable& tb, const NxgPubBatch& b, uint8_t* scratch,
                                 bool dup, bool changed, int ncu, hipStream_t s,
                                 const uint8_t** mode_out);
// stage 3, when flags[3] is set: the UpdateChanged comparisons that need the stack walk
// (prev_used: nxg_pub_prev(scratch) if stage 2 sorted, else null)
hipError_t nxg_launch_pub_deep(const NxgPubTable& tb, const NxgPubBatch& b, uint8_t* scratch,
                               const uint32_t* prev_used, int ncu, hipStream_t s);
const uint32_t* nxg_pub_prev(uint8_t* scratch, uint64_t n, uint64_t n_slots);
// write routing (nxg_route_writes.hip): the call's head (device, zeroed per call, copied back
// whole after the last launch) and the arguments every kernel of the call takes by value
struct NxgRwHead {
    uint64_t first_sub_inv;  // ~k of the first Subscribe span k >= ctl_begin (atomicMax; 0: none)
    uint64_t n_fresh, n_wait;
    uint64_t span_bytes, row_bytes;  // reply bytes of the Unsubscribe spans / of the rows
    uint64_t n_row_replies;
    uint64_t n_outcome[4];
    uint64_t n_entries, next_row, next_ctl;
    uint64_t pad[3];
};
static_assert(sizeof(NxgRwHead) == 128, "NxgRwHead layout");
constexpr int kRwBlock = 256;  // rows (and spans) per workgroup of the scans
struct NxgRwArgs {
    NxgWriteTable tab;
    const uint8_t* frame;
    const uint64_t* id;  // the decoded columns
    const uint8_t* wflags;
    const uint64_t* wid;
    const uint64_t* ctl_row;
    const uint64_t* ctl_off;
    const uint32_t* ctl_len;
    const uint8_t* ctl_variant;
    uint64_t n_rows, n_ctl, row_begin, ctl_begin, fresh_wid;
    uint64_t* first_unsub;  // [>= n_ids] ctx-owned: epoch << 40 | ~(the Id's first Unsubscribe row)
    uint32_t epoch;
    // outputs
    uint8_t* outcome;
    uint64_t* wait_row;
    uint64_t* wait_id;
    uint64_t* wait_wid;
    uint64_t cap_wait;
    uint64_t* unsub_id;
    uint64_t cap_unsub;
    uint8_t* reply;
    uint64_t cap_reply;
    // scratch, placed by the launcher
    NxgRwHead* head;
    uint64_t* cblk;  // per row block: (rows without a WriteId, rows on the wait list), packed
    uint64_t* oblk;  // per row block: rows of outcome (0, 1), then of (2, 3), packed likewise
    uint64_t* zblk;  // per row block: reply bytes
    uint64_t* nblk;  // per row block: replies
    uint64_t* sblk;  // per span block: reply bytes
    uint64_t* uid;   // per span: the Unsubscribe's Id
    uint32_t* rloc;  // per row / span: reply bytes before it within its block
    uint32_t* sloc;
    uint8_t* mode;   // per row from row_begin: the dispatch's row_mode
};
// `scratch` holds nxg_rw_scratch_bytes(rows from row_begin, spans from ctl_begin) bytes,
// `disp_scratch` 64 + nxg_disp_scratch_bytes(those rows, n_chans); neither needs initialising.
// `last_row`: n_slots words for the dispatch. a.head is at `scratch` afterwards.
uint64_t nxg_rw_scratch_bytes(uint64_t rows, uint64_t spans);
hipError_t nxg_launch_route_writes(NxgRwArgs a, uint8_t* scratch, uint8_t* disp_scratch,
                                   uint64_t* chan_off, uint64_t* ent_sub, uint64_t* ent_row,
                                   uint64_t cap_entries, uint64_t* last_row, int ncu,
                                   hipStream_t s);
// exclusive sums of M u32 counts into u64 offsets (nxg_publish.hip); bsum: M / 4096 + 2 words
hipError_t nxg_scan_u32(const uint32_t* hist, uint64_t M, uint64_t* off, uint64_t* bsum,
                        hipStream_t s);
// archive batches (nxg_archive.hip): Vec<BatchItem> decode. Synchronous on `s`.
struct NxgArchResult {
    uint64_t count, n_rows, n_children, consumed, err_offset;
    uint32_t err_kind;
    int rounds;  // chain rounds run (-1: the serial fallback)
};
uint64_t nxg_arch_scratch_bytes(uint64_t W);
// the fast path of archive batch decode (nxg_archive_fast.hip)
uint64_t nxg_fa_scratch_bytes(uint64_t W);
hipError_t nxg_launch_dec_fa(const uint8_t* buf, uint64_t W, uint32_t p0, uint64_t count,
                             const ColsDesc& cols, uint8_t* scratch, void* hhead, DevStatus* st,
                             hipStream_t s);
hipError_t nxg_arch_decode(const uint8_t* buf, uint64_t W, const ColsDesc& cols, uint8_t* scratch,
                           uint32_t* cap_flag, int max_rounds, NxgArchResult* res, hipStream_t s);
// a window of archive records and its image (nxg_archive_window.hip)
// one record of the window (uploaded by the host, counted and placed on the device)
struct AwRec {
    uint64_t off, len;             // the batch in dbuf
    uint64_t rows, kids;           // count pass (wave route), or the host (decoder route)
    uint64_t consumed;
    uint64_t row_off, child_off;   // scan
    uint32_t route;                // 0 skipped, 1 the wave kernels, 2 the single-batch decoder
    uint32_t declined;             // count pass: the record goes to the single-batch decoder
};
static_assert(sizeof(AwRec) == 64, "AwRec layout");
struct AwHead {
    uint64_t rows, kids;     // scan: totals
    uint32_t emit_fail;      // emit: a record the count pass took did not decode again (a bug)
    uint32_t pad;
    uint64_t n_image;        // image: rows gathered
    uint64_t n_filtered;     // image: rows dropped by `keep`
    uint64_t bad_row;        // image: the first row whose Id is >= n_ids (~0: none)
    uint64_t pad2[2];
};
static_assert(sizeof(AwHead) == 64, "AwHead layout");
hipError_t nxg_launch_aw_count(const uint8_t* dbuf, void* drecs, uint32_t n, int ncu,
                               hipStream_t s);
hipError_t nxg_launch_aw_scan(void* drecs, uint32_t n, void* dhead, hipStream_t s);
hipError_t nxg_launch_aw_emit(const uint8_t* dbuf, const void* drecs, uint32_t n,
                              const ColsDesc& cols, void* dhead, int ncu, hipStream_t s);
hipError_t nxg_launch_aw_rebase(const ColsDesc& src, const ColsDesc& dst, uint64_t nr, uint64_t nc,
                                uint64_t row_off, uint64_t child_off, uint64_t text_off,
                                hipStream_t s);
uint64_t nxg_aw_image_scratch_bytes(uint64_t n_ids);
hipError_t nxg_launch_aw_image(const ColsDesc& win, uint64_t n_rows, uint64_t n_ids,
                               const uint8_t* keep, uint8_t* scratch, uint64_t cap, uint64_t* oid,
                               uint8_t* otag, uint64_t* ofixed, uint32_t* oaux, uint64_t* osrc,
                               void* dhead, hipStream_t s);
// zstd decompression of compressed archive records (nxg_zstd.hip): host-side table builders and
// the launch; the device structures are opaque here (their sizes from the *_bytes functions)
struct NxzDictDev;
struct NxzDefaults;
bool nxg_zstd_build_dict(const uint8_t* d, uint64_t n, NxzDictDev* out, uint64_t* content_off);
bool nxg_zstd_build_defaults(NxzDefaults* o);
void nxg_zstd_set_content(NxzDictDev* d, const uint8_t* dcontent);
uint64_t nxg_zstd_dict_dev_bytes();
uint64_t nxg_zstd_defaults_bytes();
uint64_t nxg_zstd_rec_bytes();
uint64_t nxg_zstd_res_bytes();
uint64_t nxg_zstd_litbuf_bytes();
int nxg_zstd_grid(int ncu);
hipError_t nxg_launch_zstd(const uint8_t* dsrc, const void* drecs, uint32_t n, const void* ddict,
                           const void* ddefs, uint8_t* dout, uint8_t* dlit, void* dres, int grid,
                           hipStream_t s);
// zstd compression of archive records (nxg_zstd_enc.hip): the encode-side tables (built on the
// host by the code the device runs, nxg_zstd_enc.h), the dictionary content's hash table (built on
// the device), the compressor and the kernel that packs the frames for the copy back
struct NxzEncDict;
bool nxg_zstd_build_enc_dict(const uint8_t* d, uint64_t n, NxzEncDict* out);
void nxg_zstd_enc_dict_set(NxzEncDict* d, const uint8_t* dcontent, uint32_t content_len,
                           const uint32_t* dtable);
bool nxg_zstd_build_enc_tables(void* o);
uint64_t nxg_zstd_enc_dict_bytes();
uint64_t nxg_zstd_enc_tables_bytes();
uint64_t nxg_zstd_enc_rec_bytes();
uint64_t nxg_zstd_enc_res_bytes();
uint64_t nxg_zstd_enc_slab_bytes();
uint64_t nxg_zstd_dict_table_bytes();
uint64_t nxg_zstd_frame_bound(uint64_t len);
int nxg_zstd_enc_grid(int ncu);
hipError_t nxg_launch_zstd_dict_hash(const uint8_t* dcontent, uint32_t content_len, uint32_t* dtable,
                                     hipStream_t s);
hipError_t nxg_launch_zstd_enc(const uint8_t* dsrc, const void* drecs, uint32_t n,
                               const void* ddict, const void* dtables, uint8_t* dout,
                               uint8_t* dslab, void* dres, const uint32_t* dorder,
                               uint32_t* dticket, int grid, uint32_t literals, hipStream_t s);
hipError_t nxg_launch_zstd_pack(const uint8_t* dout, const void* drecs, const void* dres,
                                const uint64_t* dpk, uint32_t n, uint8_t* dpacked, int ncu,
                                hipStream_t s);
// one share of a decoded frame's rows (nxg_share.hip): bounds (4 u64 in device memory: the first
// child slot of a container row >= r0 / >= r1, the first control span with ctl_row >= r0 / >= r1;
// ~0 for none), then the copy of rows [r0, r0 + nr), children [c0, c0 + nc) and control spans
// [k0, k0 + nk), re-based, with the Heartbeats among those spans counted into *hb (device u64)
hipError_t nxg_launch_share_bounds(const ColsDesc& src, uint64_t r0, uint64_t r1, uint64_t* b,
                                   hipStream_t s);
hipError_t nxg_launch_share_copy(const ColsDesc& src, const ColsDesc& dst, uint64_t r0,
                                 uint64_t nr, uint64_t c0, uint64_t nc, uint64_t k0, uint64_t nk,
                                 uint64_t* hb, hipStream_t s);
// per-client encode (nxg_encode_clients): the tile encoders over a dispatch's entry list. Entry e
// is the row ent_row[e] of the columns; client c's payload starts at the byte offset of entry
// chan_off[c], stored to client_off[c] by the tile that holds the entry (the last tile also
// stores the total for every chan_off[c] >= n_ent). DevStatus of a gathered encode: err_key =
// ~(the first entry whose row is >= the batch's n_rows) (atomicMax; 0: none), irregular bit 0 = a
// chan_off past n_ent.
struct NxgGather {
    const uint64_t* ent_row;
    uint64_t n_ent;
    const uint64_t* chan_off;  // [n_clients + 1]
    uint32_t n_clients;
    uint64_t* client_off;      // [n_clients + 1]
};
uint64_t nxg_enc_f64_gather_tiles(uint64_t n_ent);
hipError_t nxg_launch_enc_f64_gather(const uint64_t* id, const uint64_t* val, uint64_t n_rows,
                                     const NxgGather& g, uint8_t* out, uint64_t cap,
                                     uint64_t* tstat, uint32_t epoch, DevStatus* st, int grid,
                                     hipStream_t s);
uint64_t nxg_enc_rows_gather_tiles(uint64_t n_ent);
hipError_t nxg_launch_enc_rows_gather(const ColsDesc& cols, const uint8_t* heap,
                                      const NxgGather& g, uint8_t* out, uint64_t cap,
                                      uint64_t* tstat, uint32_t epoch, DevStatus* st, int grid,
                                      hipStream_t s);
// the layout's gathered encoder (nxg_encode_clients.hip) and its tiles (= tstat words)
uint64_t nxg_enc_clients_tiles(bool f64, uint64_t n_ent);
hipError_t nxg_launch_enc_clients(bool f64, const ColsDesc& cols, const uint8_t* heap,
                                  const NxgGather& g, uint8_t* out, uint64_t cap, uint64_t* tstat,
                                  uint32_t epoch, DevStatus* st, int grid_f64, int grid_gen,
                                  hipStream_t s);
int nxg_occupancy_enc_f64();
int nxg_occupancy_enc_general();

// the value table (nxg_value_table.hip): values folded into columns and storage the table owns.
// A source of values: rows (tag null: all F64, aux null: 0), their children and their heap, each
// with the bound the sizing pass checks against.
struct NxgVtSrc {
    const uint8_t* tag;
    const uint64_t* fixed;
    const uint32_t* aux;
    const uint8_t* ctag;
    const uint64_t* cfixed;
    const uint32_t* caux;
    const uint8_t* heap;
    uint64_t n_rows, n_children, heap_len;
};
struct NxgVtDst {
    uint8_t* tag;  // null: an F64 table
    uint64_t* fixed;
    uint32_t* aux;
    uint8_t* heap;
    uint8_t* ctag;
    uint64_t* cfixed;
    uint32_t* caux;
    uint64_t n_slots, cap_bytes, cap_children;
    uint64_t heap_used, child_used;  // the appends start here
};
// causes of a refused slot (the low byte of NxgVtHead.err_inv); kVtOld is added when the value
// walked was the slot's old one
enum : uint32_t {
    kVtRow = 1, kVtTag = 2, kVtHeap = 3, kVtKids = 4, kVtNoKids = 5, kVtDepth = 6, kVtNotF64 = 7,
    kVtSlot = 8, kVtOld = 16
};
struct NxgVtHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t err_inv;  // ~slot << 8 | cause of the lowest refused slot (atomicMax; 0: none)
    uint64_t n_applied;
    uint64_t need_bytes, need_children, n_leaves;  // the new values' payload (the top kernel)
    uint64_t old_bytes, old_children;              // the replaced values' payload
    uint32_t ok;         // the top kernel: no refusal and everything fits; nothing is written before
    uint32_t seg_short;  // more heap-borne leaves than the segment list holds
    uint64_t pad[8];
};
static_assert(sizeof(NxgVtHead) == 128, "NxgVtHead layout");
struct NxgVtArgs {
    NxgVtSrc batch;  // the values of the selected slots: row src_row[s] - 1
    NxgVtSrc old;    // apply: the table itself (old values are sized); rebuild: the source table
    NxgVtDst dst;
    const uint64_t* src_row;  // [n_sel] 1 + row, 0: not selected; null: none selected
    uint64_t n_sel;           // apply: n_slots; rebuild: the source table's slots
    uint32_t rebuild;         // unselected slots take old's value (past n_sel: Null)
    // scratch, placed by the launcher
    NxgVtHead* head;
    uint64_t* lbytes;   // per slot: new heap bytes / child slots / leaves before it in its block
    uint64_t* lkids;
    uint64_t* lleaves;
    uint64_t* bbytes;   // per block of kVtBlock slots: the sums, then (top kernel) the bases
    uint64_t* bkids;
    uint64_t* bleaves;
    uint64_t* bold;     // per block, three arrays of n blocks: replaced bytes, replaced child slots,
                        // selected slots (summed by the top kernel: no atomics on one word)
    uint64_t* seg_dst;  // [seg_cap + 1] per heap-borne leaf: where its bytes go in dst.heap ...
    uint64_t* seg_src;  // [seg_cap] ... and where they are (an address)
    uint64_t seg_cap;
    uint32_t* bitmap;   // set_unsubscribed: one bit per slot (zeroed)
};
constexpr int kVtBlock = 256;
// `scratch` holds nxg_vt_scratch_bytes(dst.n_slots, seg_cap, path) bytes, `path` being the one the
// launcher takes (apply: mixed or F64 by dst.tag; unsub); only the head (at its start) is
// initialised, by the launchers. a.head is at `scratch` afterwards.
enum { kVtPathMixed = 0, kVtPathF64 = 1, kVtPathUnsub = 2 };
uint64_t nxg_vt_scratch_bytes(uint64_t n_slots, uint64_t seg_cap, int path);
hipError_t nxg_launch_vt_apply(NxgVtArgs a, uint8_t* scratch, int ncu, hipStream_t s);
// the named slots' old values sized (each slot once) and replaced by NXG_TAG_UNSUBSCRIBED
hipError_t nxg_launch_vt_unsub(NxgVtArgs a, const uint32_t* slot, uint64_t n, uint8_t* scratch,
                               hipStream_t s);

// Device-side copy of the column pointers (passed by value to kernels).
struct ColsDesc {
    uint64_t cap_rows, cap_children, cap_ctl;
    uint64_t n_rows, n_children, n_ctl;  // encode input counts
    uint64_t* id;
    uint8_t* tag;
    uint64_t* fixed;
    uint32_t* aux;
    uint8_t* ctag;
    uint64_t* cfixed;
    uint32_t* caux;
    uint64_t* ctl_row;
    uint64_t* ctl_off;
    uint32_t* ctl_len;
    uint8_t* ctl_variant;
    // To::Write rows (NxgWriteCols): NxgWriteFlags and the WriteId per row; null for From
    uint8_t* wflags;
    uint64_t* wid;
};

// the path table and Subscribe routing (nxg_route_subscribes.hip)
// A path table as the kernels see it: open addressing, linear probing from hash & mask. A slot's
// hash word is 0 (empty: a probe ends here), 1 (tombstone: probed past, reused by inserts) or the
// key's 64-bit hash (>= 2); a hit is a hash match confirmed by all of the key's bytes.
struct NxgPtView {
    uint64_t* hash;     // [mask + 1]
    uint64_t* key_off;  // [mask + 1]: the key's bytes at heap + key_off
    uint32_t* key_len;
    uint64_t* id;
    uint8_t* heap;      // the table's own copy of the inserted paths (16 readable bytes past it)
    uint64_t mask;      // slots - 1 (slots: a power of two, >= 2 * cap_paths)
};
struct NxgPtHead {  // device, zeroed per call, copied back after the last launch
    uint64_t n_dup;      // insert: paths that lost (already present, or a lower index of the call)
    uint64_t n_missing;  // remove: paths not found
    uint64_t n_fresh;    // insert: empty slots taken (tombstones reused are not counted)
    uint64_t pad;
};
// insert: path i is heap[heap_base + off[i] .. heap_base + off[i + 1]) (already copied there).
// hash pass (the hash, and whether the table has the path), claim pass (the call's equal paths
// meet in a scratch table `tmp` of tmp_mask + 1 words preset to ~0: atomicMin keeps the lowest
// index), place pass (the winners into the table). `h`: n words, `tslot`: n words, `state`: n bytes.
hipError_t nxg_launch_pt_insert(const NxgPtView& t, uint64_t heap_base, const uint64_t* off,
                                const uint64_t* id, uint64_t n, uint64_t* h, uint64_t* tmp,
                                uint64_t tmp_mask, uint64_t* tslot, uint8_t* state,
                                NxgPtHead* head, hipStream_t s);
// remove: path i is keys[off[i] .. off[i + 1]) (device staging, 16 readable bytes past it)
hipError_t nxg_launch_pt_remove(const NxgPtView& t, const uint8_t* keys, const uint64_t* off,
                                uint64_t n, NxgPtHead* head, hipStream_t s);
hipError_t nxg_launch_pt_lookup(const NxgPtView& t, const uint8_t* heap, const uint64_t* off,
                                const uint32_t* len, uint64_t n, uint64_t* id_out, hipStream_t s);
// every live entry of `from` into `to` (empty, at least as many slots): drops the tombstones
hipError_t nxg_launch_pt_rehash(const NxgPtView& from, const NxgPtView& to, hipStream_t s);

struct NxgRsHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t stop_inv;   // ~k of the first span k >= ctl_begin that ends the run (atomicMax; 0: none)
    uint64_t bad_inv;    // ~k << 8 | cause, of the first span k whose current value cannot be
                         // encoded (atomicMax: one word, so the cause is that span's; 0: none)
    uint64_t pad0;
    uint64_t reply_bytes;
    uint64_t n_replies, n_sub;
    uint64_t n_outcome[5];
    uint64_t next_ctl;
    uint32_t stopped, pad1;
    uint64_t pad[3];
};
static_assert(sizeof(NxgRsHead) == 128, "NxgRsHead layout");
struct NxgRsArgs {
    NxgPtView paths;
    ColsDesc cur;  // the published values: tag / fixed / aux by slot, the children; null tag: F64
    const uint8_t* cur_heap;
    uint64_t n_ids, n_slots;
    const uint32_t* slot_of_id;
    const uint8_t* allow_of_id;
    uint64_t n_defaults;
    const uint8_t* default_heap;
    const uint64_t* default_off;
    uint64_t deferred_room;
    const uint8_t* frame;
    const uint64_t* ctl_row;
    const uint64_t* ctl_off;
    const uint32_t* ctl_len;
    const uint8_t* ctl_variant;
    const uint32_t* span_perm;
    uint64_t n_ctl, row_begin, ctl_begin;
    // outputs
    uint8_t* outcome;
    uint64_t* span_id;
    uint64_t* sub_id;
    uint32_t* sub_perm;
    uint64_t cap_sub;
    uint64_t* deferred;
    uint64_t cap_deferred;
    uint8_t* reply;
    uint64_t cap_reply;
    // scratch, placed by the launcher (per span from ctl_begin / per block of kRwBlock spans)
    NxgRsHead* head;
    uint64_t* poff;   // the path's first byte in the frame
    uint64_t* vlen;   // |Value| of the current value (Subscribed spans)
    uint64_t* zloc;   // reply bytes before the span within its block
    uint64_t* sid;    // the Id its path resolves to, or NXG_NO_ID
    uint32_t* plen;
    uint32_t* cloc;   // deferral candidates before the span within its block
    uint32_t* sloc;   // Subscribed spans before it within its block
    uint8_t* pre;     // the resolve pass's verdict (an NxgSubscribeOutcome, or kRsCandidate)
    uint64_t* cblk;   // per block: deferral candidates
    uint64_t* zblk;   // per block: reply bytes
    uint64_t* nblk;   // per block: replies | Subscribed << 32
    uint64_t* oblk;   // per block, three arrays: outcomes 0 | 1 << 32, 2 | 3 << 32, 4
};
uint64_t nxg_rs_scratch_bytes(uint64_t spans);
// a.head is at `scratch` afterwards; `scratch` needs no initialising
hipError_t nxg_launch_route_subscribes(NxgRsArgs a, uint8_t* scratch, hipStream_t s);

// reply routing (nxg_route_replies.hip): the call's head (device, zeroed per call, copied back
// whole after the last launch) and the arguments every kernel of the call takes by value
struct NxgRrHead {
    uint64_t stop_inv;  // ~k of the first span k >= ctl_begin the call stops in front of
                        // (atomicMax; 0: none)
    uint64_t bad_inv;   // ~k << 8 | cause, of the first span k whose path names a request the
                        // tables do not hold: 1 q >= n_pending, 2 pend_slot[q] >= n_slots
    uint64_t span_bytes, row_bytes;  // reply bytes of the spans / of the rows
    uint64_t n_span_replies, n_unmatched;
    uint64_t n_sub, n_unsub;
    uint64_t n_outcome[7];
    uint64_t n_entries, next_row, next_ctl;
    uint32_t stopped, pad1;
    uint64_t pad[5];
};
static_assert(sizeof(NxgRrHead) == 192, "NxgRrHead layout");
struct NxgRrArgs {
    NxgSubTable subs;
    NxgPtView pending;
    uint64_t n_pending;
    const uint32_t* pend_slot;
    const uint8_t* pend_alive;
    const uint8_t* frame;
    const uint64_t* id;  // the decoded columns
    const uint64_t* ctl_row;
    const uint64_t* ctl_off;
    const uint32_t* ctl_len;
    const uint8_t* ctl_variant;
    uint64_t n_rows, n_ctl, row_begin, ctl_begin;
    // ctx-owned, never cleared: epoch << 40 | ~j of the first span ctl_begin + j of this call that
    // names the Id (an Unsubscribed or Subscribed span) / the pending request's path
    uint64_t* first_id;  // [>= n_ids]
    uint64_t* first_q;   // [>= n_pending]
    uint32_t epoch;
    // outputs
    uint8_t* outcome;
    uint64_t* span_q;
    uint64_t* span_id;
    uint64_t* sub_span;
    uint64_t* sub_q;
    uint64_t* sub_id;
    uint64_t cap_sub;
    uint64_t* unsub_id;
    uint32_t* unsub_slot;
    uint64_t cap_unsub;
    uint8_t* reply;
    uint64_t cap_reply;
    uint64_t* last_row;
    // scratch, placed by the launcher
    NxgRrHead* head;
    uint64_t* sid;    // per span: its Id (variants 2, 3), or NXG_NO_ID
    uint64_t* sq;     // per span: the request its path names (variants 0, 1, 3), or NXG_NO_ID
    uint64_t* sloc;   // per span: bytes | replies | SUBSCRIBED | UNSUBSCRIBED before it in its block
    uint64_t* zblk;   // per span block: reply bytes
    uint64_t* nblk;   // per span block: replies
    uint64_t* sblk;   // per span block: SUBSCRIBED spans
    uint64_t* ublk;   // per span block: UNSUBSCRIBED spans
    uint64_t* oblk;   // per span block, four arrays: outcomes 0 | 1 << 32, 2 | 3, 4 | 5, 6
    uint64_t* rzblk;  // per row block: reply bytes
    uint64_t* rnblk;  // per row block: replies
    uint64_t* item_val;   // per item: the row, or NXG_ENT_SPAN | k
    uint32_t* item_slot;  // per item: its slot at that point, or NXG_NO_SLOT
    uint32_t* rloc;   // per row: reply bytes before it within its block, bit 31: it replies
    uint8_t* skind;   // per span: the stop it would be (0: none; 1, 2; 3: 2, path not plain)
};
// `scratch` holds nxg_rr_scratch_bytes(rows from row_begin, spans from ctl_begin) bytes,
// `disp_scratch` 64 + nxg_disp_scratch_bytes(those rows + spans, n_chans); neither needs
// initialising. a.head is at `scratch` afterwards.
uint64_t nxg_rr_scratch_bytes(uint64_t rows, uint64_t spans);
hipError_t nxg_launch_route_replies(NxgRrArgs a, uint8_t* scratch, uint8_t* disp_scratch,
                                    uint64_t* chan_off, uint64_t* ent_sub, uint64_t* ent_row,
                                    uint64_t cap_entries, int ncu, hipStream_t s);
