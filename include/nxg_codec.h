/*
 * nxg_codec.h -- C ABI of the MI355X-native netidx batch-update codec.
 *
 * The reference codec is the generic Rust `trait Pack` (netidx-core/src/pack.rs:149-165). It is
 * called once per message at two seams:
 *
 *   encode: ClientCtx::handle_updates   netidx/src/publisher/server.rs:604-629
 *           -> WriteChannel::queue_send netidx/src/channel.rs:177-202
 *           -> <From as Pack>::encode   (netidx-derive/src/lib.rs:289-381)
 *   decode: decode_task                 netidx/src/subscriber/connection.rs:209-242
 *           -> ReadChannel::receive_batch_fn   netidx/src/channel.rs:504-521
 *           -> <From as Pack>::decode   (netidx-derive/src/lib.rs:482-601)
 *
 * This ABI replaces each of those per-message loops with ONE batch call. Each call covers all
 * the messages of one frame payload, executed by hand-written gfx950 HIP kernels. The wire bytes
 * are identical to the reference.
 *
 * Conventions follow netidx-ffi (netidx-ffi/netidx.h, netidx-ffi/src/error.rs:19-29):
 * - fallible calls return `bool`;
 * - on failure they fill a caller-provided `NetidxError*` whose `msg` must be released with
 *   nxg_error_free;
 * - handles are opaque.
 *
 * Threading: an NxgCtx is not internally synchronised. Use one ctx per connection/thread. Each ctx
 * owns one HIP stream (or a caller-provided one).
 *
 * Columnar layout (the decode output and the encode input):
 *
 *   rows (one per From::Update, in wire order):
 *     id    u64  publisher::Id (netidx-netproto/src/publisher.rs:7)
 *     tag   u8   Value wire tag (netidx-value/src/lib.rs:361-468); 17 is normalised to 16, and
 *                Error(String) is always 18
 *     fixed u64  scalar payload: integers (signed values sign-extended), f32/f64 bit patterns,
 *                DateTime/Duration seconds, bool as 1/0; for String/Bytes/Error(String)/Decimal/
 *                Abstract: byte offset of the payload in the heap (decode: the frame itself);
 *                for Array/Map/Error(Value): index of the first child slot
 *     aux   u32  DateTime/Duration nanoseconds; byte length of String/Bytes/Decimal/Abstract;
 *                element count of Array, entry count of Map, 1 for Error(Value)
 *   children (elements of Array, key/value pairs of Map, inner of Error(Value)): ctag/cfixed/
 *     caux with the same meaning. Each container's elements are contiguous, allocated
 *     depth-first.
 *   ctl (every other From message, with Heartbeat included, kept as validated raw spans):
 *     ctl_row     index of the first Update row that follows it
 *     ctl_off     byte offset of the message in the frame
 *     ctl_len     byte length of the message
 *     ctl_variant From variant (0 NoSuchValue, 1 Denied, 2 Unsubscribed, 3 Subscribed,
 *                 5 Heartbeat, 6 WriteResult)
 *
 * NXG_LAYOUT_F64 is the homogeneous fast path. It is valid only when every message is
 * From::Update with an F64 value. Only id and fixed (the f64 bits) are meaningful; tag is
 * implicitly 9.
 */
#ifndef NXG_CODEC_H
#define NXG_CODEC_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* netidx-ffi/netidx.h:162-164 */
typedef struct NetidxError {
    char* msg;
} NetidxError;

typedef struct NxgCtx NxgCtx;

/* PackError (netidx-core/src/pack.rs:89-95) plus codec-level kinds */
enum NxgErrKind {
    NXG_OK = 0,
    NXG_UNKNOWN_TAG = 1,
    NXG_TOO_BIG = 2,
    NXG_INVALID_FORMAT = 3,
    NXG_BUFFER_SHORT = 4,
    NXG_DEPTH = 6,    /* Value nesting deeper than NXG_MAX_DEPTH (documented deviation) */
    NXG_CAPACITY = 7, /* output columns too small */
    NXG_NOT_F64 = 8,  /* valid batch, but F64-only columns were supplied for mixed content */
    NXG_TIMEOUT = 9,  /* device-side progress watchdog fired (should never happen) */
    NXG_UNSUPPORTED = 10, /* publish: an UpdateChanged comparison of values nested deeper than
                             NXG_MAX_DEPTH levels (every Value variant's equality is implemented,
                             netidx-value/src/op.rs:133-172) */
};

#define NXG_MAX_DEPTH 32

enum NxgLayout { NXG_LAYOUT_F64 = 1, NXG_LAYOUT_MIXED = 2 };
enum NxgMem { NXG_MEM_DEVICE = 0, NXG_MEM_HOST = 1 /* pinned host */ };
enum NxgDecodeFlags {
    NXG_DECODE_DEFAULT = 0,
    NXG_DECODE_HINT_MIXED = 1, /* skip the homogeneous-f64 attempt */
};

typedef struct NxgColumns {
    uint32_t layout; /* NxgLayout: alloc-time capability; after decode, what was written */
    uint32_t mem;    /* NxgMem */
    uint64_t cap_rows, cap_children, cap_ctl;
    uint64_t n_rows, n_children, n_ctl, n_heartbeat;
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
} NxgColumns;

typedef struct NxgStatus {
    uint64_t n_rows, n_children, n_ctl, n_heartbeat;
    int32_t err_kind;    /* NxgErrKind of the FIRST failing message (reference is sequential) */
    uint32_t path;       /* 1 = homogeneous-f64 kernel, 2 = general kernel, 4 = fast mixed kernel */
    uint64_t err_offset; /* byte offset of the first failing message */
} NxgStatus;

/* ---- lifetime -------------------------------------------------------------------------- */
NxgCtx* nxg_ctx_new(int device, NetidxError* err);
void nxg_ctx_destroy(NxgCtx* ctx);
/* Use `hip_stream` (a hipStream_t) instead of the ctx's own stream; NULL restores it. */
bool nxg_ctx_set_stream(NxgCtx* ctx, void* hip_stream, NetidxError* err);
void* nxg_ctx_stream(NxgCtx* ctx);
void nxg_error_free(NetidxError* err);
/* library version string, e.g. "nxg 0.1.0 gfx950" */
const char* nxg_version(void);

/* ---- columns ------------------------------------------------------------------------------
 * layout F64 allocates id+fixed only; MIXED allocates every array. mem: device or pinned host.
 * Capacity bounds for a frame of W bytes: rows <= W/4 (the smallest Update, `04 04 00 10`),
 * children <= W, ctl <= W/2 (`02 05`). */
bool nxg_columns_alloc(NxgCtx* ctx, uint32_t layout, uint64_t cap_rows, uint64_t cap_children,
                       uint64_t cap_ctl, uint32_t mem, NxgColumns* out, NetidxError* err);
void nxg_columns_free(NxgCtx* ctx, NxgColumns* cols);

/* ---- decode: replaces decode_task's receive_batch_fn loop (connection.rs:209-242) ---------
 * `frame` is one frame payload (no u32 header; channel.rs:379-443 strips it), host or device
 * memory. `out` must come from nxg_columns_alloc. Synchronous. Returns false only on API
 * misuse or a HIP failure. A malformed frame returns true with st->err_kind != 0, and the whole
 * frame is rejected, as in connection.rs:228-231.
 * A well-formed frame that needs more rows, children or control spans than out->cap_rows,
 * cap_children or cap_ctl returns true with st->err_kind = NXG_CAPACITY (its err_offset is
 * unspecified). No element at or past any capacity of any array is written, whatever the outcome.
 * After NXG_CAPACITY n_rows, n_children and n_ctl (in *st and in *out) are what the frame needs,
 * so columns of those sizes take it; what the arrays hold below the capacities is unspecified. A
 * format error takes precedence over NXG_CAPACITY. The same holds for the async forms below, whose
 * status nxg_ctx_sync fills; in a backlog the other frames' columns are decoded as usual. */
bool nxg_decode_updates(NxgCtx* ctx, const uint8_t* frame, uint64_t len, NxgColumns* out,
                        uint32_t flags, NxgStatus* st, NetidxError* err);
/* Asynchronous device-resident variant: enqueue on the ctx stream; no host sync. Only the
 * path selected up front runs (flags). nxg_ctx_sync completes it, runs the general fallback if
 * the homogeneous path rejected the frame, and fills the status. At most 512 async calls
 * (decode and encode together) may be in flight between syncs; the next one fails. A frame must
 * stay unchanged until nxg_ctx_sync: a fallback (or a redo, see nxg_ctx_sync) re-reads it
 * there, after every later call has run, and a later call of the backlog that wrote into it
 * makes nxg_ctx_sync fail that decode with an error (it never decodes the overwritten bytes). */
bool nxg_decode_updates_async(NxgCtx* ctx, const uint8_t* dframe, uint64_t len, NxgColumns* dout,
                              uint32_t flags, NetidxError* err);
/* Completes every in-flight call, in order; a backlog leaves behind what its calls would have,
 * each run to completion before the next. The status is the last decode's (or the first failing
 * one's), the error the first failing call's. A call whose fast kernel declined is finished here,
 * after the calls behind it have run; every later call that reads or writes memory rewritten in
 * this way is then done again, in order, so columns and buffers may be reused within a backlog
 * (the later call's result is the one left). Doing a call again reads its input again -- a
 * decode its frame, an encode its columns: if a later call of the backlog wrote into that input
 * and no earlier call's completion here has put it back, that call fails with an error naming
 * it ("async call <index> ... keep ... unchanged until nxg_ctx_sync"), the sync returns false,
 * and what the failed call and the calls that read its output leave behind is undefined. Whether
 * a fast kernel declines depends on the data and on the frames and batches the ctx saw before,
 * so only a backlog in which no call writes into what an earlier call reads is sure to complete. */
bool nxg_ctx_sync(NxgCtx* ctx, NxgStatus* st, NetidxError* err);
/* A connection's backlog of frames (read_task hands decode_task frame after frame over a
 * channel, channel.rs:379-443 / connection.rs:209-242): n device frames, each decoded into its own
 * device columns (outs[j]; the same columns may be passed for several frames, the later frame then
 * overwrites them), in order, as n nxg_decode_updates_async calls would. Every frame must be
 * complete in device memory when the call is made (work still queued on the ctx stream may not
 * produce it). On the homogeneous-f64 path the frames are pipelined: the record-length probe of
 * frame j + 1 runs in the same launch as the column emit of frame j. nxg_ctx_sync completes them
 * (and reruns any frame the fast path rejected); every frame counts as one in-flight call. */
bool nxg_decode_frames_async(NxgCtx* ctx, uint32_t n, const uint8_t* const* dframes,
                             const uint64_t* lens, NxgColumns* const* douts, uint32_t flags,
                             NetidxError* err);

/* ---- encode: replaces handle_updates' queue_send loop (server.rs:610-612) ----------------
 * `heap` holds the bytes that string/bytes/decimal/abstract offsets and ctl spans refer to.
 * It may be NULL for pure fixed-width columns. in/heap/out must all be device memory, or all
 * host memory. An encode that fails (a buffer too small) may leave any bytes inside
 * [out, out + cap); failing or not, it writes nothing outside. */
bool nxg_encoded_len(NxgCtx* ctx, const NxgColumns* in, const uint8_t* heap, uint64_t* len_out,
                     NetidxError* err);
bool nxg_encode_updates(NxgCtx* ctx, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                        uint64_t cap, uint64_t* len_out, NetidxError* err);
/* Async device-resident variant (len_out is written at nxg_ctx_sync time). `din` (the struct and
 * its arrays), like a decode's frame, must stay unchanged until nxg_ctx_sync: a batch the
 * sequential-id encoder declines is encoded again there, after every later call has run, and a
 * later call of the backlog that wrote into the columns makes nxg_ctx_sync fail that encode with
 * an error (it never encodes the overwritten rows), unless an earlier call's completion there
 * rewrote them first (a decode into them that fell back: the relay decode -> encode -> decode ->
 * encode over one set of columns). `dout` may be reused by later calls of the backlog. An encode
 * that fails (the error above, a buffer too small) may leave any bytes inside [dout, dout + cap);
 * it writes nothing outside. */
bool nxg_encode_updates_async(NxgCtx* ctx, const NxgColumns* din, const uint8_t* dheap,
                              uint8_t* dout, uint64_t cap, uint64_t* len_out, NetidxError* err);
/* nxg_encode_updates plus the frame split of WriteChannel::queue_send + try_flush
 * (netidx/src/channel.rs:177-202, 237-257): the payload is cut before the message that would take
 * a frame past MAX_BATCH = 0x3FFFFFFF bytes, so `out` holds the frames' payloads back to back and
 * chunk_len_out[0 .. *n_chunks) their lengths (each goes out behind its own u32 header,
 * nxg_frame_header). The encode kernels record the cut themselves (the message holding byte
 * MAX_BATCH). Batches that would need a second cut (more than MAX_BATCH + the first chunk's
 * length, about 2 GiB) are refused: the reference then cuts before every further message
 * (channel.rs:187 compares against the last chunk's length), which nxg_frame_split reproduces
 * from message lengths. An empty batch gives no frame, as try_flush sends nothing. */
bool nxg_encode_frames(NxgCtx* ctx, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                       uint64_t cap, uint64_t* len_out, uint64_t* chunk_len_out,
                       uint64_t cap_chunks, uint64_t* n_chunks, NetidxError* err);

/* ---- subscriber write batches: publisher::To (netidx-netproto/src/publisher.rs:50-70) ------
 * The other direction of a connection. nxg_decode_writes replaces the publisher's
 * con.receive_batch(batch) loop (netidx/src/publisher/server.rs:660); nxg_encode_writes replaces
 * the subscriber's queue_send(&To::Write(..)) / queue_send(&To::Unsubscribe(..)) loop
 * (netidx/src/subscriber/connection.rs:384-399). Every message is varint(L) variant fields:
 *   0 Subscribe { path, resolver: SocketAddr, timestamp: u64, permissions: u32, token: Bytes }
 *   1 Unsubscribe(Id)
 *   2 Write(Id, bool, Value, #[pack(default)] WriteId)
 * Rows are the Write messages in wire order: id/tag/fixed/aux and the children mean what they
 * mean for an Update, and the two further fields of a Write go to the companion NxgWriteCols
 * (NxgColumns keeps its layout). Subscribe and Unsubscribe messages are validated and kept as raw
 * control spans (ctl_row/ctl_off/ctl_len) with ctl_variant = the To variant (0 or 1).
 * nxg_route_writes (below) then routes the decoded rows: permissions, on_write channels, the
 * WriteResult and Unsubscribed replies. Synchronous calls only: the async ring, the multi-GPU
 * calls and the sessions do not take To frames. */
#define NXG_PATH_WRITES 6 /* NxgStatus.path of a To-frame decode */
enum NxgWriteFlags {
    NXG_WRITE_REPLY = 1, /* Write's bool: the writer wants a WriteResult */
    NXG_WRITE_NO_WID = 2 /* no WriteId on the wire (an old peer, or one cut short by the length
                            prefix): the caller allots one, as WriteId::default() does; wid[i]
                            is 0 */
};
typedef struct NxgWriteCols {
    uint32_t mem; /* NxgMem */
    uint32_t pad;
    uint64_t cap_rows;
    uint8_t* wflags; /* NxgWriteFlags per row */
    uint64_t* wid;   /* WriteId per row */
} NxgWriteCols;
bool nxg_write_cols_alloc(NxgCtx* ctx, uint64_t cap_rows, uint32_t mem, NxgWriteCols* out,
                          NetidxError* err);
void nxg_write_cols_free(NxgCtx* ctx, NxgWriteCols* cols);
/* `frame`: host or device memory (a frame from nxg_session_recv_frame goes straight in). `out`
 * must have the MIXED layout; `out` and `wout` are both device memory or both pinned host memory,
 * and wout->cap_rows >= out->cap_rows. Capacity bounds for W bytes: rows <= W/5 (`05 02 00 00 10`),
 * children <= W, ctl <= W/3 (`03 01 07`). n_heartbeat is 0. A malformed frame returns true with
 * st->err_kind / err_offset of the first failing message and all counts 0, as nxg_decode_updates;
 * false on misuse, a HIP failure or an exceeded capacity (NXG_CAPACITY in the message). */
bool nxg_decode_writes(NxgCtx* ctx, const uint8_t* frame, uint64_t len, NxgColumns* out,
                       NxgWriteCols* wout, NxgStatus* st, NetidxError* err);
/* The same call with options; opts NULL (or fast = 0) is nxg_decode_writes itself: the same
 * launches, path 6, the same errors. fast = 1 tries the tile-parallel fast decoder first, under
 * the argument and capacity contract of nxg_decode_writes word for word (device or pinned-host
 * columns, host or device frame, NXG_CAPACITY with the same message and zeroed counts, nothing at
 * or past any capacity written, a malformed frame true with (err_kind, err_offset) and zero counts,
 * synchronous only). The fast decoder takes a frame whose every message is, with its length
 * filled exactly and a canonical length prefix (L counts its own prefix),
 *   a Write `L 02 varint(id) bool Value [varint(wid)]` of a one-byte L, an id of any width,
 *     bool 0 or 1, a valid Value without child slots (fixed-size and varint scalars,
 *     DateTime, Duration, String, Bytes, Decimal, Error(String)), and then nothing
 *     (NXG_WRITE_NO_WID) or one varint of 1-10 bytes,
 *   an Unsubscribe `L 01 varint(id)`, or
 *   a Subscribe `varint(L) 00 varint(plen) path tag addr u64 u32 varint(tlen) token` with address
 *     tag 0 or 1, canonical plen / tlen, a UTF-8 path, and at most 256 bytes in all (prefix
 *     included).
 * Non-canonical id / wid varints are taken too. It declines everything else -- Subscribes
 * longer than 256 bytes, non-canonical plen / tlen, Array / Map / Error(Value) / Abstract values,
 * bytes left inside a length wrap (a wid cut short by the message end included), every frame the
 * general decoder rejects, frames of 4 GiB or more, and columns too small for the frame -- and
 * the same call then reruns the frame on the general decoder. st->path (and the status
 * nxg_last_status reports) is NXG_PATH_WRITES_FAST when the fast decoder took the frame, which
 * implies err_kind 0 and n_children 0, and NXG_PATH_WRITES after a decline; the columns are
 * identical either way. A frame of the accepted set can still fall back for a geometric reason
 * (bytes inside values or tokens that spell a chain of messages which crosses a 4 KiB tile edge
 * without rejoining the true one, or more than 16 such false chains in front of the first true
 * message start of each of two adjacent tiles). A decline keeps no state: the next call tries the fast decoder again. An
 * empty frame launches nothing and reports path 6. fast > 1 or reserved != 0 is misuse (false,
 * with a message, before any use of the context). */
#define NXG_PATH_WRITES_FAST 8 /* NxgStatus.path: the fast To decoder took the frame */
typedef struct NxgWriteDecodeOpts {
    uint32_t fast;     /* 0: the general decoder only (nxg_decode_writes); 1: try the fast decoder first */
    uint32_t reserved; /* must be 0 */
} NxgWriteDecodeOpts;
bool nxg_decode_writes_opts(NxgCtx* ctx, const uint8_t* frame, uint64_t len, NxgColumns* out,
                            NxgWriteCols* wout, const NxgWriteDecodeOpts* opts /* NULL = defaults */,
                            NxgStatus* st, NetidxError* err);
/* Each row becomes varint(L) 02 varint(id) (wflags & NXG_WRITE_REPLY) Value varint(wid), with
 * L = lw(1 + vl(id) + 1 + |Value| + vl(wid)); NXG_WRITE_NO_WID is ignored (the reference encoder
 * always writes the WriteId). Control spans (pre-encoded Subscribe / Unsubscribe messages) are
 * copied from `heap` before row ctl_row[k]. in/win/heap/out all device memory, or all host memory.
 * out NULL: the length only. A message longer than MAX_BATCH fails with TooBig. A batch whose total exceeds MAX_BATCH
 * (0x3FFFFFFF bytes) is refused before anything is written: size it with nxg_encoded_writes_len
 * and split the rows; the frame cut of nxg_encode_frames is not extended to write batches. A failed
 * encode (a buffer too small) may leave any bytes inside [out, out + cap); failing or not, it
 * writes nothing outside. */
bool nxg_encoded_writes_len(NxgCtx* ctx, const NxgColumns* in, const NxgWriteCols* win,
                            const uint8_t* heap, uint64_t* len_out, NetidxError* err);
bool nxg_encode_writes(NxgCtx* ctx, const NxgColumns* in, const NxgWriteCols* win,
                       const uint8_t* heap, uint8_t* out, uint64_t cap, uint64_t* len_out,
                       NetidxError* err);

/* ---- multi-GPU: one frame decoded in byte ranges, one batch encoded in shards -------------
 * One process per GPU. A frame of W bytes is cut into contiguous byte ranges; each GPU decodes
 * the messages that START in its range, reading past the range end as needed (messages never
 * straddle frames, channel.rs:187-201, but they do straddle ranges). A range's summary says
 * where its chain enters (the first message start >= begin) and leaves (the first start >= end,
 * or the frame end); nxg_range_link checks that consecutive ranges meet and numbers their rows.
 * Any f64 frame (the length-run decoder, or the single-pass decoder when ids come in any order)
 * into f64 or mixed columns, and frames of short Updates / Heartbeats (the fast mixed decoder)
 * into mixed columns; a range those decoders decline (Maps, nested containers, rare control
 * messages, content errors) reports ok = 0 (err_kind NXG_CAPACITY when it was declined because
 * the columns are too small). nxg_decode_sharded then falls back to row shares
 * (nxg_decode_share). */
typedef struct NxgRange {
    uint64_t begin, end; /* the byte range [begin, end) of the frame */
    uint64_t entry;      /* first message start >= begin (absolute byte offset) */
    uint64_t exit;       /* first message start >= end, or the frame end */
    uint64_t n_rows;     /* rows decoded from the range (at dout rows 0 .. n_rows) */
    uint32_t ok;         /* 1: decoded by bytes; 2: decoded as a row share (nxg_decode_sharded's
                            fallback: entry = exit = UINT64_MAX); 0: declined */
    uint32_t err_kind;   /* NxgErrKind: the columns overflowed (ok = 1, or ok = 0 when that is why
                            the range was declined); the frame's error (ok = 2); else 0 */
    uint64_t err_offset; /* ok = 2: the frame's error offset */
} NxgRange;
/* Device frame and device columns; synchronous. */
bool nxg_decode_range(NxgCtx* ctx, const uint8_t* dframe, uint64_t frame_len, uint64_t begin,
                      uint64_t end, NxgColumns* dout, NxgRange* rng, NetidxError* err);
/* One share of a frame's rows: the frame (device) decoded whole, as nxg_decode_updates does
 * (every decoder, every error), then rows [N*share/shares, N*(share+1)/shares) of its N rows, the
 * children of their values and the control spans before them (the last share: also those after
 * the last row) into dout (device columns) from row 0, child indices and ctl_row re-based;
 * *row_off = the share's first row. The frame's error (status->err_kind / err_offset) leaves no
 * rows in any share; a share that does not fit dout reports NXG_CAPACITY (NXG_NOT_F64 for mixed
 * content in f64 columns). The ctx grows its own whole-frame columns on demand (first `shares`
 * times dout's capacities). Synchronous. */
bool nxg_decode_share(NxgCtx* ctx, const uint8_t* dframe, uint64_t frame_len, uint32_t share,
                      uint32_t shares, NxgColumns* dout, uint64_t* row_off, NxgStatus* status,
                      NetidxError* err);
/* Ranges in frame order, contiguous from 0 to frame_len: checks ranges[0].entry == 0,
 * ranges[i].exit == ranges[i+1].entry and the last exit == frame_len; row_off[i] = rows before
 * range i. Returns false (and *bad = the first range whose entry is off the chain) otherwise. */
bool nxg_range_link(const NxgRange* ranges, uint32_t n, uint64_t frame_len, uint64_t* row_off,
                    uint32_t* bad, NetidxError* err);

/* RCCL communicator (librccl, over xGMI) for the sharded calls. nxg_comm_unique_id on one rank,
 * its 128 bytes sent to every rank by the caller (as ncclGetUniqueId's id), nxg_comm_init on
 * every rank (collective). */
typedef struct NxgComm NxgComm;
bool nxg_comm_unique_id(uint8_t id[128], NetidxError* err);
NxgComm* nxg_comm_init(NxgCtx* ctx, int nranks, int rank, const uint8_t id[128],
                       NetidxError* err);
void nxg_comm_destroy(NxgComm* comm);
/* A caller-provided transport for the sharded calls instead of RCCL (the application's own MPI
 * or TCP collectives; the tests' gloo), and optionally a caller-provided local codec instead of
 * the ctx's kernels. Collective functions are called by every rank in the same order and return
 * true on success. The protocol (nxg_encode_allgather, nxg_decode_sharded) is the same code for
 * every transport: every rank's failure is exchanged in the next collective, so all ranks return
 * false together (none is left waiting in a collective). */
typedef struct NxgCommOps {
    void* user;
    /* collective: `bytes` bytes at `mine` (host memory) from every rank, in rank order, into
     * `all` (host memory, nranks * bytes) */
    bool (*allgather)(void* user, const void* mine, void* all, uint64_t bytes);
    /* collective: `buf` (device memory; host memory with the codec hooks below) holds this
     * rank's shard at [off[rank], off[rank + 1]); afterwards every rank's buf holds every shard
     * at its offset (off has nranks + 1 entries) */
    bool (*allgatherv)(void* user, uint8_t* buf, const uint64_t* off, uint32_t nranks,
                       uint32_t rank);
    /* local codec, all three or none (NULL: the ctx's kernels): the contracts of
     * nxg_encoded_len, nxg_encode_updates and nxg_decode_range */
    bool (*encoded_len)(void* user, const NxgColumns* in, const uint8_t* heap, uint64_t* len);
    bool (*encode)(void* user, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                   uint64_t cap, uint64_t* len);
    bool (*decode_range)(void* user, const uint8_t* frame, uint64_t frame_len, uint64_t begin,
                         uint64_t end, NxgColumns* out, NxgRange* rng);
    /* optional with the codec hooks (NULL: a declined range fails nxg_decode_sharded): the
     * contract of nxg_decode_share */
    bool (*decode_share)(void* user, const uint8_t* frame, uint64_t frame_len, uint32_t share,
                         uint32_t shares, NxgColumns* out, uint64_t* row_off, NxgStatus* status);
} NxgCommOps;
/* Not collective. ctx may be NULL when ops carries the local codec. The ops struct is copied. */
NxgComm* nxg_comm_init_ops(NxgCtx* ctx, int nranks, int rank, const NxgCommOps* ops,
                           NetidxError* err);
/* BASELINE configs[4]: every rank encodes its shard of the batch (rows in rank order) straight
 * into its place in the full frame (an 8-byte all-gather of the shard sizes first), then grouped
 * send/recv deliver every shard into the same offsets on every rank: no padding, no compaction.
 * *len_out = the full frame length; shard_off[0 .. nranks) = each shard's byte offset (may be
 * NULL). Device columns and buffers (host ones with an ops comm's local codec). A failure on any
 * rank (its encode, a capacity short of the frame) makes every rank return false. */
bool nxg_encode_allgather(NxgCtx* ctx, NxgComm* comm, const NxgColumns* din, const uint8_t* dheap,
                          uint8_t* dout, uint64_t cap, uint64_t* len_out, uint64_t* shard_off,
                          NetidxError* err);
/* One frame (on every rank's device) decoded in nranks byte ranges: rank r decodes range r,
 * the summaries are all-gathered and linked; a range whose guessed entry is off the chain is
 * decoded again from its predecessor's exit. *row_off = this rank's first global row. When a
 * range is declined (rng->ok 0 on some rank: content the byte-range decoders do not take), every
 * rank sees it in the same exchange and falls back to nxg_decode_share(rank, nranks): the frame
 * decoded whole on every rank (the frame is there already; no data moves), rows in nranks row
 * shares, rng->ok = 2, the frame's error in rng->err_kind / err_offset. Every rank returns the
 * same verdict: a local failure on any rank (a launch, a range declined for capacity), or a frame
 * that does not link makes all of them return false. */
bool nxg_decode_sharded(NxgCtx* ctx, NxgComm* comm, const uint8_t* dframe, uint64_t frame_len,
                        NxgColumns* dout, uint64_t* row_off, NxgRange* rng, NetidxError* err);

/* ---- dispatch: replaces ConnectionCtx::process_updates_batch (connection.rs:546-567) ------
 * The decoded Update rows fanned out to the subscriber's channels. For each row, in batch
 * order: the subscription of its Id, found by a dense table (publisher Ids come from a counter
 * starting at 0, netidx-core/src/utils.rs:130-134); an Id with no subscription, or >= n_ids, is
 * dropped, as `self.subscriptions.get(&i)` returning None. For each stream of the
 * subscription, in stream order, the entry (SubId, row) is appended to that stream's channel
 * batch (by_chan, connection.rs:551-557), so every channel sees its updates in batch order. A
 * subscription that keeps `last` records its last row in the batch (connection.rs:559-561).
 *
 * The table is a CSR built by the host from its subscriptions map; every array is device
 * memory: */
#define NXG_NO_SLOT 0xffffffffu
typedef struct NxgSubTable {
    uint64_t n_ids;                   /* slot_of_id covers Ids [0, n_ids) */
    const uint32_t* slot_of_id;       /* [n_ids]: subscription slot, or NXG_NO_SLOT */
    uint64_t n_slots;                 /* subscriptions */
    const uint64_t* slot_sub_id;      /* [n_slots]: SubId (subscriber/mod.rs:85) */
    const uint32_t* slot_stream_off;  /* [n_slots + 1]: the slot's streams, CSR */
    const uint32_t* stream_chan;      /* [n_streams]: channel of each stream, < n_chans */
    const uint8_t* slot_has_last;     /* [n_slots]: 1 if the subscription keeps `last` */
    uint32_t n_chans;                 /* channels (ChanId) */
} NxgSubTable;
/* A slot may name one channel more than once: each stream gets its own entry, in stream order
 * (the reference dedups streams on subscribe, connection.rs:328-358; the table need not).
 * n_chans == 0 is valid: chan_off[0] = 0 and no entries, last_row and n_unmatched as usual. So
 * are a table with no slots and a batch in which no Id has one.
 *
 * Output (device memory, capacities from the caller):
 *   chan_off[n_chans + 1]  channel c's batch is entries [chan_off[c], chan_off[c+1])
 *   ent_sub[cap], ent_row[cap]  (SubId, index of the update's row in the decoded columns)
 *   last_row[n_slots]      1 + the last row of the slot's subscription in this batch, 0 if none
 *                          (or if the slot keeps no `last`) */
typedef struct NxgDispatch {
    uint64_t cap_entries;
    uint64_t* chan_off;
    uint64_t* ent_sub;
    uint64_t* ent_row;
    uint64_t* last_row;
    uint64_t n_entries;   /* written by the call */
    uint64_t n_unmatched; /* rows whose Id has no subscription */
} NxgDispatch;
/* `id` = the decoded id column (device), n_rows rows. Synchronous. Returns false on API misuse,
 * a HIP failure, or entries > cap_entries (n_entries then holds the required capacity). */
bool nxg_dispatch_updates(NxgCtx* ctx, const NxgSubTable* tab, const uint64_t* id,
                          uint64_t n_rows, NxgDispatch* out, NetidxError* err);

/* ---- write routing: replaces the Write and Unsubscribe arms of ClientCtx::handle_batch_inner
 * (netidx/src/publisher/server.rs:497-576) and write() (server.rs:171-245) ----------------------
 * The rows and control spans of one decoded To frame (nxg_decode_writes, device columns), in
 * message order, with the reference's outcome per message. State is per connection (client).
 * For Write(id, r, v, wid), row i, the checks run in this order:
 *   NXG_WRITE_UNSUBSCRIBED  the client is not subscribed to id, "cannot write to unsubscribed
 *       value" (server.rs:201-202): id >= n_ids, perm_of_id[id] == NXG_NOT_SUBSCRIBED, or an
 *       Unsubscribe(id) came earlier in this batch (server.rs:562-565; unsubscribe() removes
 *       cl.subscribed[id]). A client the publisher does not know gets the same message
 *       (server.rs:201): pass a table with n_ids = 0.
 *   NXG_WRITE_DENIED        the permissions lack WRITE (0x04, resolver_server/auth.rs:26), "write
 *       permission denied" (server.rs:203-205)
 *   NXG_WRITE_NOT_ACCEPTED  no on_write entry for id, or none of its channels is open, "writes
 *       not accepted" (server.rs:206-217). The host builds the table from open channels only (the
 *       retain of server.rs:207-214; it keeps its own gc_on_write), so a slot with an empty channel
 *       list is this outcome.
 *   NXG_WRITE_ROUTED        one request onto each channel of on_write[id], in list order
 *       (server.rs:225-240); with r set, (id, wid) is appended to the wait list (server.rs:218-224).
 *       The table describes published values only: an on_write slot implies that by_id has the Id
 *       (the `if let Some(pbv) = t.by_id.get(&id)` of server.rs:226 always holds).
 * The other three outcomes with r set queue From::WriteResult(id, Error(String(msg)), wid) on the
 * connection (server.rs:191-194); without r they queue nothing. Unsubscribe(id) always queues
 * From::Unsubscribed(id), for any id, subscribed or not (server.rs:562-566).
 * Order: control span k precedes row ctl_row[k]; spans with equal ctl_row are in k order; a write
 * at row i is after an Unsubscribe span k if and only if ctl_row[k] <= i. The reply frame holds
 * the replies of both kinds in message order:
 *   Unsubscribed(id)                        varint(L) 02 varint(id)
 *   WriteResult(id, Error(String(m)), wid)  varint(L) 06 varint(id) 12 varint(|m|) m varint(wid)
 * The effective WriteId: a row with NXG_WRITE_NO_WID has none on the wire and the reference allots
 * a fresh one at decode time (WriteId::default() is WriteId::new(), netidx-netproto/src/
 * publisher.rs:11-15). The caller passes fresh_wid, the first of a block it reserved: among the
 * rows the call processes, the j-th NO_WID row in row order gets fresh_wid + j, and n_fresh says
 * how many were used. Replies and the wait list carry the effective id; the columns are not
 * modified.
 * Subscribe needs a path lookup and is not this call's (the host's, or nxg_route_subscribes',
 * below, which alternates with this call through a mixed frame): the call stops in front of the first
 * Subscribe span at or after ctl_begin and says where (below). Also left to the host: creating
 * the SendResult of each wait-list entry, gc_on_write, its own unsubscribe() bookkeeping from
 * unsub_id[], and building the WriteRequests (path, client, value) from the entries.
 *
 * The table, built by the host for one client; every array is device memory: */
#define NXG_NOT_SUBSCRIBED 0xffffffffu
typedef struct NxgWriteTable {
    uint64_t n_ids;                /* perm_of_id and slot_of_id cover Ids [0, n_ids) */
    const uint32_t* perm_of_id;    /* [n_ids]: the client's Permissions bits for the Id
                                      (cl.subscribed[id]), or NXG_NOT_SUBSCRIBED */
    const uint32_t* slot_of_id;    /* [n_ids]: on_write slot of the Id, or NXG_NO_SLOT */
    uint64_t n_slots;              /* on_write entries */
    const uint32_t* slot_chan_off; /* [n_slots + 1]: the slot's open channels, CSR */
    const uint32_t* chan;          /* open channels in on_write order, each < n_chans */
    uint32_t n_chans;              /* channels (ChanId) */
} NxgWriteTable;
enum NxgWriteOutcome {
    NXG_WRITE_ROUTED = 0,
    NXG_WRITE_UNSUBSCRIBED = 1,
    NXG_WRITE_DENIED = 2,
    NXG_WRITE_NOT_ACCEPTED = 3
};
/* Capacities and device arrays from the caller, counts written by the call. A-priori bounds for
 * R rows and K control spans: entries <= R * the longest channel list, wait <= R, unsub <= K,
 * reply bytes <= 58 * R + 12 * K. */
typedef struct NxgWriteRoute {
    uint64_t cap_rows;  /* outcome[] entries, >= cols->n_rows */
    uint8_t* outcome;   /* [cap_rows]: NxgWriteOutcome of row i, written for the processed rows */
    /* per channel c the requests [chan_off[c], chan_off[c+1]) as (ent_sub = Id, ent_row = row in
     * the columns), in batch order; chan_off has n_chans + 1 entries; last_row is not used (NULL);
     * n_entries is repeated below, n_unmatched is 0 */
    NxgDispatch disp;
    uint64_t cap_wait;  /* wait list: (row, Id, effective WriteId) of routed rows with r set */
    uint64_t* wait_row;
    uint64_t* wait_id;
    uint64_t* wait_wid;
    uint64_t cap_unsub; /* the Ids of the Unsubscribe spans, in order */
    uint64_t* unsub_id;
    uint64_t cap_reply; /* the reply frame's payload */
    uint8_t* reply;
    /* written by the call */
    uint64_t n_entries, n_wait, n_unsub;
    uint64_t n_replies;    /* messages in `reply` (WriteResults + Unsubscribeds) */
    uint64_t reply_len;    /* bytes in `reply` */
    uint64_t n_fresh;      /* WriteIds taken from fresh_wid on */
    uint64_t n_outcome[4]; /* processed rows per NxgWriteOutcome */
    uint64_t next_row, next_ctl; /* where to resume: row_begin / ctl_begin of the next call */
    uint32_t stopped_at_subscribe; /* 1: span next_ctl - 1 is a Subscribe, in front of next_row */
    uint32_t pad;
} NxgWriteRoute;
/* `frame` is the device frame the columns were decoded from (the Unsubscribe spans' Ids are read
 * from it: varint(L) 01 varint(id), validated by the decode; a non-canonical L and trailing bytes
 * inside the wrap are accepted as the decode accepted them). `cols` / `wcols`: the device columns
 * nxg_decode_writes filled. The call processes control spans [ctl_begin, s), s = the first
 * Subscribe span at or after ctl_begin or n_ctl, and rows [row_begin, ctl_row[s]) or to n_rows. On
 * return next_ctl = s + 1 and next_row = ctl_row[s], or both are at the end and
 * stopped_at_subscribe is 0: the host handles the Subscribe, updates the table (the unsub_id[] of
 * this call included) and calls again with (next_row, next_ctl) until next_ctl == n_ctl and
 * next_row == n_rows. A call covers fewer than 2^32 rows. One synchronisation; synchronous.
 * Returns false on misuse (the message names the field: host or F64-layout columns, wcols NULL,
 * row_begin / ctl_begin past the end, a missing array), on a HIP failure, or when a capacity is
 * exceeded; the counts then hold the required values (n_entries, n_wait, n_unsub, reply_len), as
 * nxg_dispatch_updates does, and the arrays hold what fitted. */
bool nxg_route_writes(NxgCtx* ctx, const NxgWriteTable* tab, const uint8_t* frame,
                      const NxgColumns* cols, const NxgWriteCols* wcols, uint64_t row_begin,
                      uint64_t ctl_begin, uint64_t fresh_wid, NxgWriteRoute* out, NetidxError* err);

/* ---- a device-resident by_path: path (its exact bytes) -> publisher::Id ----------------------
 * PublisherInner.by_path (netidx/src/publisher/mod.rs) as a hash table in device memory, built
 * and queried on the device: open addressing with a stored 64-bit hash, a hit confirmed by
 * comparing every byte of the path (a hash match alone is never an answer). The table owns a copy
 * of the inserted bytes. It holds at most cap_paths paths in slots sized so that they stay at or
 * below half full, and cap_bytes bytes of paths; the bytes of a removed path are not reclaimed
 * (cap_bytes bounds what was ever inserted). Keys are canonical paths: the host canonises what it
 * inserts (nxg_path_is_plain says when the bytes already are). One thread at a time per table; a
 * table belongs to the device of the ctx that made it. */
typedef struct NxgPathTable NxgPathTable;
#define NXG_NO_ID UINT64_MAX
NxgPathTable* nxg_path_table_new(NxgCtx* ctx, uint64_t cap_paths, uint64_t cap_bytes,
                                 NetidxError* err);
void nxg_path_table_free(NxgPathTable* t);
uint64_t nxg_path_table_len(const NxgPathTable* t);
/* Host arrays: path i is paths[off[i] .. off[i+1]) and maps to id[i] (never NXG_NO_ID). The
 * result does not depend on scheduling: a path already in the table keeps its Id; among equal
 * paths of one call the lowest index wins; *n_dup (may be NULL) counts the losers of both kinds.
 * len + n > cap_paths, or more bytes than the table has left, is refused (NXG_CAPACITY in the
 * message) before anything changes. Synchronous. */
bool nxg_path_table_insert(NxgCtx* ctx, NxgPathTable* t, const uint8_t* paths, const uint64_t* off,
                           const uint64_t* id, uint64_t n, uint64_t* n_dup, NetidxError* err);
/* Removing leaves a tombstone that lookups probe past and later inserts reuse; a path that is
 * absent (or named a second time in the call) counts in *n_missing (may be NULL). Synchronous. */
bool nxg_path_table_remove(NxgCtx* ctx, NxgPathTable* t, const uint8_t* paths, const uint64_t* off,
                           uint64_t n, uint64_t* n_missing, NetidxError* err);
/* Device arrays: path i is dheap[doff[i] .. doff[i] + dlen[i]); did_out[i] = its Id, or NXG_NO_ID.
 * The paths are read in aligned 8-byte words: dheap must be readable up to the next multiple of 8
 * past its last path (any allocation is). What Publisher::id(path) answers. Synchronous. */
bool nxg_path_table_lookup(NxgCtx* ctx, const NxgPathTable* t, const uint8_t* dheap,
                           const uint64_t* doff, const uint32_t* dlen, uint64_t n,
                           uint64_t* did_out, NetidxError* err);
/* A path is plain if it has no `\` byte, is not empty, has no `//` and no trailing `/` (unless it
 * is exactly `/`). Path::decode canonises (netidx-core/src/path.rs:24-48, 70-72, 131-139) and its
 * splitting honours `\` escapes; a plain path is canonical as it stands, so its wire bytes are
 * the by_path key. Host-side, no ctx. */
bool nxg_path_is_plain(const uint8_t* path, uint64_t len);
/* The 64-bit word the table stores for a path, computed on the host exactly as the kernels compute
 * it: a multiplicative hash over the path's length and its little-endian 8-byte words (the last
 * one zero above the path's end), never 0 or 1 (those mark empty slots and tombstones: a raw 0 or
 * 1 is stored as 2 or 3). A path's probe starts at slot hash & (slots - 1). The seam that tests
 * and tools check their own statement of the hash against; distinct paths can share a hash, and
 * the table then tells them apart by their bytes. Host-side, no ctx. */
uint64_t nxg_path_hash(const uint8_t* path, uint64_t len);

/* ---- Subscribe routing: replaces the Subscribe arm of ClientCtx::handle_batch_inner
 * (netidx/src/publisher/server.rs:506-549) and subscribe() (server.rs:60-137) -----------------
 * One run of consecutive Subscribe spans of a decoded To frame (nxg_decode_writes, device
 * columns; the decode validated each path's UTF-8). The run is spans k = ctl_begin, ctl_begin + 1,
 * ... for as long as ctl_variant[k] == 0, ctl_row[k] == row_begin (no Write row lies in between)
 * and the path is plain (nxg_path_is_plain). On return next_ctl is the span the run ended in
 * front of, and `stopped` says why:
 *   0  the end of the spans
 *   1  span next_ctl is an Unsubscribe, or a Write row comes first: the host continues with
 *      nxg_route_writes(row_begin, next_ctl), which is unchanged and still stops in front of the
 *      next Subscribe (then: next_row / next_ctl - 1 of that call go in here)
 *   2  span next_ctl is a Subscribe whose path is not plain: the host handles that one message
 *      and resumes at next_ctl + 1
 * The two calls alternate through a mixed frame; between them the host updates perm_of_id from
 * sub_id[] / sub_perm[] (and unsub_id[]). A frame of Subscribes only takes one call.
 * Per span, in the reference's order (server.rs:68-135):
 *   NXG_SUB_DENIED         span_perm[k] == NXG_SUB_PERM_DENY (server.rs:520-535), or the path
 *       resolves, by_id has the Id and allow_of_id[id] == 0 (server.rs:98-106): Denied(path)
 *   NXG_SUB_DEFERRED       the path is not in by_path, the greatest default base <= path (byte
 *       order) is a byte prefix of it, and fewer than deferred_room spans of this call were
 *       deferred before it: no reply, the span's index goes to deferred[]. Only that one base is
 *       examined, as the loop of server.rs:74-93 does: with bases /a and /a/b the path /a/c gets
 *       NoSuchValue although /a is a prefix; with base /d the path /dx is deferred (starts_with
 *       is a string prefix). The `continue` on a closed channel (server.rs:81) is the host's: it
 *       lists the bases of open channels only.
 *   NXG_SUB_NO_SUCH_VALUE  the path is not in by_path, otherwise: NoSuchValue(path)
 *   NXG_SUB_IGNORED        the path resolves, but id >= n_ids or slot_of_id[id] == NXG_NO_SLOT
 *       (by_id.get_mut is None, server.rs:97): nothing
 *   NXG_SUB_SUBSCRIBED     otherwise: Subscribed(path, id, current), and (id, permissions) is
 *       appended to sub_id[] / sub_perm[] (cl.subscribed.insert, server.rs:109). The same path
 *       twice gives two replies and two entries, as the reference does.
 * The reply frame holds the replies in span order, L = lw(|body|):
 *   NoSuchValue(path)            varint(L) 00 varint(|p|) p
 *   Denied(path)                 varint(L) 01 varint(|p|) p
 *   Subscribed(path, id, value)  varint(L) 03 varint(|p|) p varint(id) Value
 * with the current value of every tag encoded as nxg_encode_updates encodes it (text, Decimal,
 * Abstract, nested Array / Map / Error(Value) from the table's children).
 * Left to the host: the hc_subscribed interning and the ut.subscribed update from sub_id[]
 * (server.rs:111-124), wait_clients (127-131), Event::Subscribe (132), sending the deferred paths
 * to their default channels (80-85), the gc of hc_subscribed (569-571), check_token (its SHA3)
 * and extended_auth, whose results come in as span_perm[] and allow_of_id[]. */
#define NXG_SUB_PERM_DENY 0xffffffffu
enum NxgSubscribeOutcome {
    NXG_SUB_SUBSCRIBED = 0,
    NXG_SUB_NO_SUCH_VALUE = 1,
    NXG_SUB_DENIED = 2,
    NXG_SUB_DEFERRED = 3,
    NXG_SUB_IGNORED = 4
};
/* Built by the host; every array is device memory (the two structs themselves are host memory) */
typedef struct NxgSubscribeTable {
    const NxgPathTable* paths;     /* by_path */
    const struct NxgPubTable* pub; /* by_id: n_ids, slot_of_id, n_slots and the cur_* columns of
                                      the current values (the client CSR is not read) */
    const uint8_t* allow_of_id;    /* [n_ids]: extended_auth evaluated for this client, 0 denies;
                                      NULL: no extended_auth */
    uint64_t n_defaults;           /* the default publishers' bases (open channels only), sorted */
    const uint8_t* default_heap;   /* ascending in byte order and unique: base b is */
    const uint64_t* default_off;   /* default_heap[default_off[b] .. default_off[b+1]) */
    uint64_t deferred_room;        /* MAX_DEFERRED - deferred_subs.inner().len(), server.rs:56, 78 */
} NxgSubscribeTable;
/* Capacities and device arrays from the caller, counts written by the call. A-priori bounds for
 * K spans: sub <= K, deferred <= min(K, deferred_room), reply bytes <= the spans' bytes + K * (15
 * + the longest current value). */
typedef struct NxgSubscribeRoute {
    uint64_t cap_spans;    /* outcome[] / span_id[] entries, >= cols->n_ctl */
    uint8_t* outcome;      /* [cap_spans]: NxgSubscribeOutcome of span k, for the run's spans */
    uint64_t* span_id;     /* [cap_spans]: the Id the span's path resolves to, or NXG_NO_ID */
    uint64_t cap_sub;      /* the Subscribed spans' (Id, Permissions bits), in order */
    uint64_t* sub_id;
    uint32_t* sub_perm;
    uint64_t cap_deferred; /* the deferred spans' indices, in order */
    uint64_t* deferred;
    uint64_t cap_reply;    /* the reply frame's payload */
    uint8_t* reply;
    /* written by the call */
    uint64_t n_spans;      /* spans of the run: next_ctl - ctl_begin */
    uint64_t n_sub, n_deferred;
    uint64_t n_replies;    /* messages in `reply` */
    uint64_t reply_len;    /* bytes in `reply` */
    uint64_t n_outcome[5]; /* the run's spans per NxgSubscribeOutcome */
    uint64_t next_ctl;
    uint32_t stopped;      /* 0, 1 or 2, above */
    uint32_t pad;
} NxgSubscribeRoute;
/* `frame` is the device frame the columns were decoded from (the paths are read from it, in
 * aligned 8-byte words). span_perm (device memory) is indexed by the absolute span index: NULL is
 * DesiredAuth::Anonymous, every Subscribe gets Permissions::all() = 0x3f (resolver_server/
 * auth.rs:24-29); otherwise the host has looked up the resolver's secret and run check_token
 * (server.rs:244-271) and passes the permission bits, or NXG_SUB_PERM_DENY for "no stored secret"
 * and "token invalid" alike. One synchronisation; synchronous. Returns false on misuse (the
 * message names the field: host or F64-layout columns, a missing array, ctl_begin > n_ctl, a
 * pointer that is not device memory), on a HIP failure, when the current value of a Subscribed
 * span of the run cannot be encoded, or when a capacity is exceeded (NXG_CAPACITY in the message);
 * the counts then hold the required values (n_sub, n_deferred, reply_len) and the arrays hold what
 * fitted, as nxg_route_writes does. A value cannot be encoded when it or an element has an unknown
 * tag, when a container has no child columns or more elements than MAX_VEC allows, or when it
 * nests deeper than nxg_encode_updates accepts: the root is level 0, and a value at a level past
 * NXG_MAX_DEPTH is refused (NXG_MAX_DEPTH containers around a scalar are the deepest). The message
 * names the lowest such span and that span's cause, whatever the scheduling. A value nobody is
 * answered with (behind the stop, or under an Id that is denied, not in by_id or not asked for)
 * is not looked at. */
bool nxg_route_subscribes(NxgCtx* ctx, const NxgSubscribeTable* tab, const uint8_t* frame,
                          const NxgColumns* cols, uint64_t row_begin, uint64_t ctl_begin,
                          const uint32_t* span_perm, NxgSubscribeRoute* out, NetidxError* err);

/* ---- reply routing: replaces ConnectionCtx::process_batch (netidx/src/subscriber/
 * connection.rs:409-541) and unsubscribe() (connection.rs:67-83) ---------------------------------
 * The subscriber's side of a frame that holds a message other than an Update (decode_task,
 * connection.rs:218-226, sends every such frame to process_batch; the publisher's Heartbeat makes
 * one every idle second, and the reply to a Subscribe burst is one): the rows and control spans of
 * one decoded From frame (nxg_decode_updates, device MIXED columns; control variants 0 NoSuchValue,
 * 1 Denied, 2 Unsubscribed, 3 Subscribed, 5 Heartbeat, 6 WriteResult), in message order. Control
 * span k precedes row ctl_row[k]; spans with equal ctl_row are in k order. An all-Update frame
 * (n_ctl == 0) stays with nxg_dispatch_updates; this call has process_batch semantics even then
 * (rows without a subscription are answered).
 *
 * State, built by the host for one connection (arrays in device memory, structs in host memory):
 *   subs       the connection's subscriptions, exactly as nxg_dispatch_updates takes them, plus one
 *              slot per pending request: the slot its subscription will occupy, with the request's
 *              sub_id, its stream list (req.streams deduplicated by channel in order: what the
 *              handle_connect_stream loop of connection.rs:521-528 leaves in sub.streams) and
 *              slot_has_last 0 if one of those streams carries STOP_COLLECTING_LAST
 *              (connection.rs:350-353), else 1. slot_of_id names live subscriptions only.
 *   pending    `pending: HashMap<Path, SubscribeValRequest>` as a path table: the path's exact
 *              bytes -> q, the request's index (the table's id is q)
 *   pend_slot  [n_pending]: the slot of request q, < subs->n_slots
 *   pend_alive [n_pending]: 0 if the request's `finished` receiver is known to be gone
 *              (connection.rs:501-505); NULL: all alive
 * The device decides plain paths only (nxg_path_is_plain), as nxg_route_subscribes does.
 *
 * "Subscribed at that point": slot_of_id[id], unless an earlier span of this call changed it: none
 * after an Unsubscribed(id) that removed it, pend_slot[q] after a Subscribed with outcome
 * NXG_REPLY_SUBSCRIBED. An Id >= n_ids has no subscription. Per message:
 *   Update(id, v), row i, subscribed: one entry (slot_sub_id, i) per stream of the slot, in stream
 *       order, appended to that stream's channel; last_row[slot] = 1 + i when the slot keeps `last`
 *       (connection.rs:419-431)
 *   Update(id, v), row i, not subscribed: To::Unsubscribe(id) is queued (connection.rs:432), once
 *       per such row; counted in disp.n_unmatched
 *   Heartbeat                     NXG_REPLY_NONE
 *   WriteResult                   NXG_REPLY_WRITE_RESULT: reported only. pending_writes reads and
 *       changes nothing else in the batch (connection.rs:435-445): matching (id, wid) is the host's
 *   NoSuchValue / Denied(path)    NXG_REPLY_FAILED if the path is in `pending` and no earlier
 *       variant-0/1/3 span of this call named it (pending.remove, connection.rs:447, 452):
 *       span_q[k] = q, and the host sends the error the variant implies. Else NXG_REPLY_NONE.
 *   Unsubscribed(id)              NXG_REPLY_UNSUBSCRIBED if subscribed at that point: one entry
 *       (slot_sub_id, NXG_ENT_SPAN | k) per stream of the slot (unsubscribe(), connection.rs:74-80),
 *       (id, slot) appended to unsub_id[] / unsub_slot[], and from there on the Id has no
 *       subscription. Else NXG_REPLY_NONE.
 *   Subscribed(path, id, m)       NXG_REPLY_ORPHAN on a pending miss (absent, or named earlier in
 *       this call): To::Unsubscribe(id) (connection.rs:464-467). On a hit with the Id not
 *       subscribed: NXG_REPLY_DROPPED if pend_alive[q] == 0: To::Unsubscribe(id), no subscription
 *       (connection.rs:502-505); else NXG_REPLY_SUBSCRIBED: (k, q, id) appended to sub_span[] /
 *       sub_q[] / sub_id[], and from there on the Id's slot is pend_slot[q] (connection.rs:491-517).
 *       A hit with the Id subscribed at that point (an alias, connection.rs:468-490) or with
 *       id >= n_ids is the host's message (stop 2).
 * span_id[k] is the Id of a variant-2/3 span, else NXG_NO_ID; span_q[k] is q for FAILED, SUBSCRIBED
 * and DROPPED, else NXG_NO_ID. Every To::Unsubscribe(id) goes out as varint(L) 01 varint(id),
 * L = lw(1 + vl(id)), always one byte; the reply frame holds them in message order, rows and spans
 * interleaved.
 *
 * Where a call stops (next_row, next_ctl, stopped):
 *   0  the end: next_ctl == n_ctl and next_row == n_rows
 *   1  span next_ctl is a Subscribed or Unsubscribed whose Id (< n_ids: an Id outside the table
 *      has no state to change) an earlier Subscribed or Unsubscribed span of this call already
 *      named, whatever that span's outcome. The call has processed the spans before it and the rows
 *      before ctl_row[next_ctl] = next_row. The host applies the outputs (slot_of_id from sub_* and
 *      unsub_*, nxg_path_table_remove of the paths with span_q[k] != NXG_NO_ID) and calls again
 *      with (next_row, next_ctl). So inside one call each Id changes state at most once.
 *   2  span next_ctl is the host's: a path that is not plain (variants 0, 1, 3), an alias, or a hit
 *      with an Id outside the table. The host applies the outputs, handles that one message,
 *      updates the tables and resumes at (next_row, next_ctl + 1). A span that is both (a path
 *      that is not plain, an Id named before) stops with 2.
 * The stop is the lowest such span, whatever the scheduling.
 *
 * Left to the host: stream_batch, the BEGIN_WITH_LAST initial values of new subscriptions
 * (connection.rs:341-349, 521-528), which the reference runs after the whole batch (connection.rs:
 * 535-536) through process_updates_batch: the host runs them after the last call, from sub_span[],
 * through nxg_dispatch_updates or by hand; pending_writes; the durable_* and `subscribed`
 * bookkeeping of unsubscribe() (connection.rs:84-117); setting `last` to Event::Unsubscribed from
 * unsub_slot[], after applying last_row; send_updates. */
#define NXG_ENT_SPAN (1ull << 63) /* ent_row: Event::Unsubscribed of span ent_row & ~NXG_ENT_SPAN */
enum NxgReplyOutcome {
    NXG_REPLY_NONE = 0,
    NXG_REPLY_WRITE_RESULT = 1,
    NXG_REPLY_FAILED = 2,
    NXG_REPLY_UNSUBSCRIBED = 3,
    NXG_REPLY_ORPHAN = 4,
    NXG_REPLY_DROPPED = 5,
    NXG_REPLY_SUBSCRIBED = 6
};
typedef struct NxgReplyTable {
    const NxgSubTable* subs;
    const NxgPathTable* pending;
    uint64_t n_pending;
    const uint32_t* pend_slot; /* [n_pending] */
    const uint8_t* pend_alive; /* [n_pending], or NULL */
} NxgReplyTable;
/* Capacities and device arrays from the caller, counts written by the call. A-priori bounds for
 * R rows and K spans: entries <= (R + K) * the longest stream list, reply bytes <= 12 * (R + K),
 * sub <= K, unsub <= K. */
typedef struct NxgReplyRoute {
    uint64_t cap_spans;  /* outcome[] / span_q[] / span_id[] entries, >= cols->n_ctl */
    uint8_t* outcome;    /* [cap_spans]: NxgReplyOutcome of span k, for the processed spans */
    uint64_t* span_q;
    uint64_t* span_id;
    /* per channel c the entries [chan_off[c], chan_off[c+1]) in message order: ent_row is the
     * Update's row, or NXG_ENT_SPAN | k for Event::Unsubscribed; last_row[n_slots]; n_unmatched =
     * the rows answered with Unsubscribe */
    NxgDispatch disp;
    uint64_t cap_sub;    /* the SUBSCRIBED spans, in order: span, request, Id */
    uint64_t* sub_span;
    uint64_t* sub_q;
    uint64_t* sub_id;
    uint64_t cap_unsub;  /* the UNSUBSCRIBED spans, in order: Id and the slot it had */
    uint64_t* unsub_id;
    uint32_t* unsub_slot;
    uint64_t cap_reply;  /* the reply frame's payload */
    uint8_t* reply;
    /* written by the call */
    uint64_t n_entries, n_sub, n_unsub;
    uint64_t n_replies;    /* messages in `reply` */
    uint64_t reply_len;    /* bytes in `reply` */
    uint64_t n_outcome[7]; /* processed spans per NxgReplyOutcome */
    uint64_t next_row, next_ctl;
    uint32_t stopped;      /* 0, 1 or 2, above */
    uint32_t pad;
} NxgReplyRoute;
/* `frame` is the device frame the columns were decoded from. The decode validated every span
 * (path UTF-8, varints, values); the call re-reads only varint(L) variant, then varint(|p|) path
 * [varint(id)] or varint(id), the paths in aligned 8-byte words, and accepts a non-canonical L and
 * trailing bytes inside the wrap as the decode accepted them. A call covers fewer than 2^32 rows
 * and spans. One synchronisation; synchronous; scratch is the ctx's. Returns false on misuse,
 * before any launch, with a message that names the field (host or F64-layout columns, a null
 * array, ctl_begin > n_ctl, row_begin > n_rows, a pointer that is not device memory, async work
 * pending on the ctx); on a HIP failure; when a path of the frame names a request q >= n_pending
 * or with pend_slot[q] >= subs->n_slots (found on the device; the message names the lowest such
 * span); or when a capacity is exceeded (NXG_CAPACITY in the message): the counts then hold the
 * required values (n_entries, n_sub, n_unsub, reply_len) and the arrays hold what fitted, as
 * nxg_route_writes does. */
bool nxg_route_replies(NxgCtx* ctx, const NxgReplyTable* tab, const uint8_t* frame,
                       const NxgColumns* cols, uint64_t row_begin, uint64_t ctl_begin,
                       NxgReplyRoute* out, NetidxError* err);

/* ---- type-partitioned view of decoded mixed columns (optional output) --------
 * Replaces the per-value 28-way `match` on the tag (Value::decode, netidx-value/src/lib.rs:470-506)
 * for a consumer that handles values by type: the rows of `cols` grouped by their tag column, on
 * the device, from a per-tile LDS tag histogram + scan (the mechanism BASELINE configs[2] names).
 * Device memory, capacities >= cols->n_rows (rows < 2^32):
 *   rank[i]      row i's index among the rows of its tag (record -> (tag[i], rank[i]))
 *   row_of[d]    the row at dense index d; tag t's rows are d in [off[t], off[t+1]), in record
 *                order
 *   fixed[d], aux[d]   the rows' fixed / aux columns at their dense index
 * off[] and count[] are filled on the host (off[NXG_TAG_BINS] = n_rows). Children (array
 * elements) and text stay where the decode put them (fixed / aux of a row still point at them).
 * Synchronous. Returns false on API misuse (F64-only columns have no tag column) or a HIP
 * failure. */
#define NXG_TAG_BINS 256
typedef struct NxgTagView {
    uint64_t cap_rows;
    uint32_t* rank;
    uint32_t* row_of;
    uint64_t* fixed;
    uint32_t* aux;
    uint64_t n_rows;                    /* written by the call */
    uint64_t count[NXG_TAG_BINS];       /* rows per tag value */
    uint64_t off[NXG_TAG_BINS + 1];     /* exclusive prefix of count */
} NxgTagView;
bool nxg_partition_by_tag(NxgCtx* ctx, const NxgColumns* cols, NxgTagView* out, NetidxError* err);

/* ---- publisher commit: replaces UpdateBatch::commit (publisher/mod.rs:776-845) ----------
 * A queued batch (its rows in NxgColumns form: id, tag, fixed, aux, text in `heap`; kind[i] per
 * row; to_client[i] for NXG_PUB_UPDATE_CLIENT rows) becomes per-client batches of
 * From::Update(id, v), in batch order:
 *   NXG_PUB_UPDATE          Update(None, id, v)  (Val::update, mod.rs:517-519): to every client
 *                           subscribed to id (pb.by_id[id].subscribed), then current = v;
 *   NXG_PUB_UPDATE_CHANGED  UpdateChanged(id, v) (update_changed): the same, only if
 *                           current != v (Value::eq, netidx-value/src/op.rs:133-172);
 *   NXG_PUB_UPDATE_CLIENT   Update(Some(cl), id, v) (update_subscriber): to client cl only.
 * Ids that are not published are dropped (counted in n_unmatched). The table (device memory):
 * by_id as a dense slot table, each slot's subscribed clients as a CSR, and each slot's current
 * value (cur_tag NULL: all F64; text, Decimal and Abstract bytes at cur_heap + cur_fixed; the
 * elements of Array/Map/Error(Value) current values at cur_ctag/cur_cfixed/cur_caux slots
 * cur_fixed .., as NxgColumns children; the batch's children are the batch's NxgColumns
 * children). Equality is Value::eq on every variant: floats NaN == NaN, Decimal numerically
 * (rust_decimal's PartialEq: scale-independent, every zero equal), containers element by element
 * (Map entries in column order -- the reference's encoder writes them sorted and unique),
 * Abstract by its bytes. Output in NxgDispatch: per client c, entries [chan_off[c], chan_off[c+1])
 * of (ent_sub = Id, ent_row = row); last_row[slot] = 1 + the row that became current (0:
 * unchanged). Synchronous; false on misuse, HIP failure, capacity, or NXG_UNSUPPORTED (a value
 * nested deeper than 32 levels; err->msg says which). */
enum NxgPubKind { NXG_PUB_UPDATE = 0, NXG_PUB_UPDATE_CHANGED = 1, NXG_PUB_UPDATE_CLIENT = 2 };
typedef struct NxgPubTable {
    uint64_t n_ids;                   /* slot_of_id covers Ids [0, n_ids) */
    const uint32_t* slot_of_id;       /* [n_ids]: published-value slot, or NXG_NO_SLOT */
    uint64_t n_slots;
    const uint32_t* slot_client_off;  /* [n_slots + 1]: subscribed clients, CSR */
    const uint32_t* client;           /* [n_subscriptions]: client index, < n_clients */
    uint32_t n_clients;
    const uint8_t* cur_tag;           /* [n_slots] current values, columns as NxgColumns */
    const uint64_t* cur_fixed;
    const uint32_t* cur_aux;          /* NULL: 0 */
    const uint8_t* cur_heap;
    const uint8_t* cur_ctag;          /* children of the current values (NULL: none) */
    const uint64_t* cur_cfixed;
    const uint32_t* cur_caux;
} NxgPubTable;
bool nxg_publish_commit(NxgCtx* ctx, const NxgPubTable* tab, const NxgColumns* batch,
                        const uint8_t* heap, const uint8_t* kind, const uint32_t* to_client,
                        NxgDispatch* out, NetidxError* err);
/* The commit's unsubscribes (publisher/mod.rs:820-832): the queued (client, Id) pairs, in queue
 * order, onto each client's From::Unsubscribed list; clients >= n_clients are dropped
 * (pb.clients.get(&cl) is None). Output: chan_off[n_clients + 1] and ent_sub (the Ids) in `out`;
 * ent_row = the pair's index in the queue; last_row unused (may be NULL). Synchronous. */
bool nxg_publish_unsubscribes(NxgCtx* ctx, const uint64_t* id, const uint32_t* client,
                              uint64_t n, uint32_t n_clients, NxgDispatch* out, NetidxError* err);
/* The commit's per-client batches, encoded: replaces the gather of every column by each client's
 * ent_row segment and one nxg_encode_updates call per client (handle_updates -> queue_send,
 * publisher/server.rs:604-629). `batch`, `heap` and `d` are the arguments and the result of
 * nxg_publish_commit, all device memory; batch may have either layout, must have n_ctl == 0, and
 * its children arrays are used as they are. Entry e < d->n_entries becomes the message
 *   varint(L) 04 varint(batch->id[r]) Value(row r),   r = d->ent_row[e],
 * byte for byte what nxg_encode_updates writes for row r; d->ent_sub is not read. The entries are
 * sorted by client, so the payloads lie back to back in client order: client c's is
 * out[client_off[c], client_off[c+1]), one frame payload that the host sends behind its own
 * nxg_frame_header. Entries may name rows in any order and any row any number of times.
 * d->chan_off[0 .. n_clients] must not decrease and must end at d->n_entries. Any other chan_off
 * fails the call: client_off is preset to all-ones, the tiles store the offsets of the clients
 * they find, and the host requires what it reads back not to decrease and to end at the encoded
 * total (a skipped client stays all-ones; offsets decrease exactly where chan_off does, since no
 * message is empty). Entries before chan_off[0] are encoded in front of client 0's payload. One launch of a tile encoder
 * that reads its rows through ent_row; no per-entry offsets are written.
 * Synchronous; a pending async call on the ctx is refused. out->out NULL sizes only: client_off
 * and n_bytes are filled and nothing else is written. false with err
 *   on misuse (NULLs, host memory, n_ctl != 0);
 *   when ent_row[e] >= batch->n_rows for an entry (checked on the device; the message names the
 *     first such entry). Only rows that an entry names are looked at: an invalid value in a row
 *     that no entry names does not fail the call;
 *   on the content errors nxg_encode_updates reports for a row that an entry names (PackError
 *     kind, TooBig);
 *   when n_bytes > cap_bytes (n_bytes then holds what is needed);
 *   when a client's payload exceeds MAX_BATCH = 0x3FFFFFFF bytes (the message names the first such
 *     client and its length: encode that client's rows with nxg_encode_frames). With
 *     cap_bytes > MAX_BATCH the call sizes first, so that such a call writes nothing; a size-only
 *     call succeeds and reports the lengths.
 * A failed call may leave any bytes inside [out, out + cap_bytes) and any values in client_off;
 * whatever the outcome, no byte outside [out, out + cap_bytes) and no element outside
 * client_off[0 .. n_clients] is written. d->n_entries == 0 gives all-zero client_off. */
typedef struct NxgClientFrames {
    uint64_t cap_bytes;   /* capacity of out */
    uint8_t* out;         /* device; NULL: size only */
    uint64_t* client_off; /* device, [n_clients + 1]: client c's payload is
                             out[client_off[c], client_off[c+1]) */
    uint64_t n_bytes;     /* written by the call: client_off[n_clients] */
} NxgClientFrames;
bool nxg_encode_clients(NxgCtx* ctx, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_clients, NxgClientFrames* out,
                        NetidxError* err);

/* ---- the value table: `pbl.current = v` (publisher/mod.rs:796, 809) and a subscription's `last`
 * The routing calls read the connection's values from const device columns and report which row
 * became current (NxgDispatch.last_row[slot] = 1 + row, 0: unchanged). These calls move the values
 * forward on the device: slot s takes the value of batch row src_row[s] - 1, with its text /
 * Decimal / Abstract bytes copied into the table's heap and its Array / Map / Error(Value) subtree
 * copied into the table's child columns, `fixed` re-based. The arrays are the caller's (device
 * memory); tag NULL is an all-F64 table (NxgPubTable.cur_tag == NULL), of which only `fixed` is
 * used. The table's columns are what NxgPubTable.cur_* and NxgColumns children expect.
 *
 * The table appends: a call writes its payload at heap_used / child_used and advances them. A
 * replaced value's payload stays where it is and leaves heap_live / child_live (sized by walking
 * it). Payloads are packed without padding in slot order, each value's in walk order: a container's
 * elements contiguous, blocks handed out in depth-first preorder, whatever the source layout. The
 * layout depends on the call sequence only. Source rows may share children, lie in any order and be
 * named by several slots.
 *
 * nxg_value_table_init   every slot Value::Null (tag 16, fixed 0, aux 0; an F64 table: fixed 0),
 *                        counters 0.
 * nxg_value_table_apply  in place. src_row: n_slots device words (NxgDispatch.last_row as it is).
 *                        `heap`, `heap_len`: the batch's payload bytes (a decoded frame: the frame).
 *                        An F64-layout batch has tag 9, aux 0. An F64 table takes a MIXED batch
 *                        whose selected rows all have tag 9 (otherwise NXG_NOT_F64 in the message).
 * nxg_value_table_rebuild  writes dst (its own arrays, dst->n_slots >= src->n_slots, the same kind
 *                        as src): selected slots from the batch, the others from src, slots past
 *                        src's Null. Afterwards heap_used == heap_live, child_used == child_live.
 *                        batch and src_row may be NULL (compaction, growth). The same kernels as
 *                        apply, the source chosen per slot.
 * nxg_value_table_set_unsubscribed  the n named slots (device u32) become NXG_TAG_UNSUBSCRIBED,
 *                        fixed 0, aux 0; their old payload leaves the live counts, a slot named
 *                        twice once. Called after apply, as the reference sets `last`.
 *
 * All or nothing: everything is validated in a sizing pass before the first write. Refused, with
 * the lowest refused slot and its cause in the message whatever the scheduling: src_row[s] - 1 >=
 * batch->n_rows; a tag outside 0..27 and NXG_TAG_UNSUBSCRIBED; a payload outside [0, heap_len) (for
 * a value the table holds: heap_used); a child range outside batch->n_children (child_used); a
 * container with elements but no child columns; a value at a level past NXG_MAX_DEPTH
 * (NXG_MAX_DEPTH containers around a scalar are the deepest). If the appended payload does not fit,
 * the call returns false with NXG_CAPACITY in the message and *out holds the exact needs and the
 * live totals the table would have: what a rebuild into other arrays must hold. After any false
 * return the table's arrays and counters are what they were, and no element at or past a capacity
 * is ever written. Synchronous, one read-back per call (a second pass, before any write, only when
 * the slots name more heap-borne values than the batch has rows and children); a ctx with async
 * work pending is refused. The table's arrays must not overlap the batch, its heap, src_row (or,
 * for rebuild, src): checked on the host. */
typedef struct NxgValueTable {
    uint64_t n_slots;
    uint8_t* tag;      /* [n_slots]; NULL: an all-F64 table */
    uint64_t* fixed;   /* [n_slots] */
    uint32_t* aux;     /* [n_slots]; NULL only when tag is NULL */
    uint8_t* heap;     /* text / Decimal / Abstract payloads */
    uint64_t cap_bytes;
    uint8_t* ctag;     /* child columns, [cap_children] each */
    uint64_t* cfixed;
    uint32_t* caux;
    uint64_t cap_children;
    /* kept by the calls, host memory */
    uint64_t heap_used, heap_live, child_used, child_live;
} NxgValueTable;
typedef struct NxgValueApply { /* written by the call */
    uint64_t n_applied;                 /* slots with src_row != 0 */
    uint64_t need_bytes, need_children; /* payload of the new values */
    uint64_t live_bytes, live_children; /* what the table holds after the call */
} NxgValueApply;
bool nxg_value_table_init(NxgCtx* ctx, NxgValueTable* t, NetidxError* err);
bool nxg_value_table_apply(NxgCtx* ctx, NxgValueTable* t, const NxgColumns* batch,
                           const uint8_t* heap, uint64_t heap_len, const uint64_t* src_row,
                           NxgValueApply* out, NetidxError* err);
bool nxg_value_table_rebuild(NxgCtx* ctx, const NxgValueTable* src, const NxgColumns* batch,
                             const uint8_t* heap, uint64_t heap_len, const uint64_t* src_row,
                             NxgValueTable* dst, NxgValueApply* out, NetidxError* err);
bool nxg_value_table_set_unsubscribed(NxgCtx* ctx, NxgValueTable* t, const uint32_t* slot,
                                      uint64_t n, NetidxError* err);

/* ---- archive batches: replaces <GPooled<Vec<BatchItem>> as Pack>::decode ------------------
 * (netidx-archive/src/logfile/reader.rs:449/475 over logfile/mod.rs:150-205 BatchItem and
 * netidx/src/subscriber/mod.rs:154-177 Event). `buf` (device memory, `len` bytes) starts with the
 * batch: varint count, then count items of varint Id (as u32) and an Event that is not
 * length-wrapped (0x40 = Unsubscribed, else a bare Value). `len` is what remains of the buffer
 * (the uncompressed reader decodes from the record to the end of the mmap, reader.rs:449): it
 * bounds the size guard, while the fast path reads only a window of it that grows geometrically
 * until the batch fits, so the cost follows the batch. A batch the fast path declines (an error,
 * Maps, nesting, ...) is decoded by the exact decoder, which walks the whole buffer.
 * Output: MIXED-layout columns (nxg_columns_alloc), one row per item: id = the u32 Id, the
 * Event's Value in tag/fixed/aux (+ children; text offsets index `buf`), Unsubscribed as tag
 * NXG_TAG_UNSUBSCRIBED with fixed 0, aux 0. status: n_rows (= count), n_children, err_kind /
 * err_offset (the failing item's start, 0 for the count and the size guard) with the reference's
 * PackError kinds; path = NXG_PATH_ARCHIVE_FAST (the fast path) or NXG_PATH_ARCHIVE (the exact
 * decoder). *consumed = the batch's length in bytes.
 * Deviation: Event::decode on an empty buffer panics in the reference; here it is
 * NXG_BUFFER_SHORT. Synchronous; false on misuse or a HIP failure. A decode error is reported in
 * `status` (as nxg_decode_updates does), with n_rows = n_children = 0. A batch that needs more
 * rows or children than out->cap_rows / cap_children is NXG_CAPACITY there, and no element at or
 * past a capacity of any array is written, whatever the outcome. */
#define NXG_TAG_UNSUBSCRIBED 0x40
#define NXG_PATH_ARCHIVE 3
#define NXG_PATH_ARCHIVE_FAST 5
bool nxg_decode_archive_batch(NxgCtx* ctx, const uint8_t* buf, uint64_t len, NxgColumns* out,
                              NxgStatus* status, uint64_t* consumed, NetidxError* err);
/* Replaces <GPooled<Vec<BatchItem>> as Pack>::encode (writer.rs:423-428, pack.rs:941-952):
 * device MIXED-layout columns in the same form (id = the u32 Id, tag NXG_TAG_UNSUBSCRIBED for
 * Event::Unsubscribed; text at heap + fixed, device memory; no control messages) to `out`
 * (device memory, `cap` bytes; NULL: *len_out = the length only). Synchronous. TooBig when
 * count * size_of::<BatchItem>() exceeds MAX_VEC or a value violates a size guard. A failed encode
 * (a buffer too small) may leave any bytes inside [out, out + cap); failing or not, it writes
 * nothing outside. */
bool nxg_encode_archive_batch(NxgCtx* ctx, const NxgColumns* in, const uint8_t* heap,
                              uint8_t* out, uint64_t cap, uint64_t* len_out, NetidxError* err);

/* ---- recording: replaces the recorder's batch loop (netidx-archive/src/recorder/record.rs:
 * 307-347): every (SubId, Event) of a channel's batch is translated through by_subid to the
 * archive's Id, entries without one are dropped, and the rest become one archive batch
 * (<Vec<BatchItem> as Pack>::encode, writer.rs:399-428). Here a dispatch's entry list becomes the
 * records of all its channels in one call.
 * `batch` and `heap` are what the dispatch was made from: device columns of either layout (for a
 * decoded frame the heap is the frame); control spans in `batch` are ignored. `d` is the result of
 * nxg_dispatch_updates or nxg_route_replies (disp), or any entry list of that form; d->last_row is
 * not read. Per channel c, over its entries e in [d->chan_off[c], d->chan_off[c+1]), in order:
 *   sub = d->ent_sub[e]; the entry is kept iff sub < tab->n_subs and arch_id_of_sub[sub] !=
 *   NXG_NO_SLOT. Any other entry is dropped and counted in n_dropped, and nothing else of it is
 *   read (its ent_row may be anything).
 *   A kept entry becomes the item varint(arch_id) Event: the byte 0x40 when ent_row[e] has
 *   NXG_ENT_SPAN set (the span index is not read) or when the row's tag is NXG_TAG_UNSUBSCRIBED,
 *   else the bare Value of batch row ent_row[e] as nxg_encode_archive_batch writes it (a row of
 *   F64-layout columns: 09 and the 8 bytes big-endian).
 *   The record is varint(rec_items[c]) and the items: byte for byte what nxg_encode_archive_batch
 *   writes for the kept entries' rows gathered into columns with id = arch_id. A channel without a
 *   kept entry gets no bytes (add_batch writes nothing for an empty batch, writer.rs:405):
 *   rec_off[c] == rec_off[c+1], rec_items[c] == 0.
 * Records lie back to back in channel order: rec_off[0] == 0, rec_off[n_chans] == n_bytes. Entries
 * may name rows in any order and any number of times, and rows may share children. Entries in front
 * of chan_off[0] belong to no channel: they are neither read, kept nor counted.
 * false with a message:
 *   on misuse, before any launch (a null argument, host memory, d->n_entries > d->cap_entries,
 *     2^39 entries or more, async work pending on the ctx);
 *   when chan_off[0 .. n_chans] decreases or does not end at d->n_entries (found on the device;
 *     the message names the lowest channel c with chan_off[c+1] < chan_off[c], or the last channel
 *     when only the end differs);
 *   for a kept entry with ent_row >= batch->n_rows, or whose row has an unknown tag, violates a
 *     size guard (PackError::TooBig), has a child range outside n_children, is a container with
 *     elements but no child columns, or nests past NXG_MAX_DEPTH: the message names the lowest such
 *     entry and its cause, whatever the scheduling;
 *   when rec_items[c] * size_of::<BatchItem>() exceeds MAX_VEC (TooBig; the first such channel);
 *   when n_bytes > cap_bytes: n_bytes, n_items, n_dropped, rec_off and rec_items then hold the
 *     true values.
 * Every check and every size is settled before the first byte of `out` is written: after any false
 * return no byte of `out` has changed. Whatever the outcome, nothing outside [out, out +
 * cap_bytes), rec_off[0 .. n_chans] and rec_items[0 .. n_chans) is written. d->n_entries == 0
 * gives all zeros. Synchronous, one read-back of a small head; out NULL sizes only (the same
 * read-back, no writing kernel). */
typedef struct NxgRecordTable {      /* by_subid: FxHashMap<SubId, Id>, record.rs:196 */
    uint64_t n_subs;                 /* arch_id_of_sub covers SubIds [0, n_subs) (SubIds come from a counter) */
    const uint32_t* arch_id_of_sub;  /* device; the archive Id, or NXG_NO_SLOT: by_subid has no entry */
} NxgRecordTable;
typedef struct NxgRecordBatches {
    uint64_t cap_bytes;   /* capacity of out */
    uint8_t* out;         /* device; NULL: size only */
    uint64_t* rec_off;    /* device [n_chans + 1]: channel c's record is out[rec_off[c], rec_off[c+1]) */
    uint64_t* rec_items;  /* device [n_chans]: items in channel c's record */
    uint64_t n_bytes, n_items, n_dropped;   /* written by the call */
} NxgRecordBatches;
bool nxg_record_entries(NxgCtx* ctx, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_chans, const NxgRecordTable* tab,
                        NxgRecordBatches* out, NetidxError* err);

/* ---- indexed archives: the RecordIndex in front of every batch (netidx-archive/src/logfile/
 * mod.rs:146-149, #[derive(Pack)] struct RecordIndex { index: Vec<Id> }).
 *
 * nxg_archive_index_records replaces the HashSet loop of add_batch (writer.rs:407-429): the indexes
 * of n_recs records in one call. `key` (device, n_keys positions) and `seg_off` (device, n_recs + 1
 * entries, in the form of NxgDispatch.chan_off) give record c the positions [seg_off[c],
 * seg_off[c+1]); positions in front of seg_off[0] or behind seg_off[n_recs] belong to no record and
 * are not read. n_keys is stated so that no launch depends on a read-back.
 *   tab == NULL: key[p] is the archive Id itself (the id column given to nxg_encode_archive_batch,
 *     or a decoded window's). An Id >= 2^32 is refused; the message names the lowest such position,
 *     whatever the scheduling.
 *   tab != NULL: key[p] is a SubId, translated and filtered exactly as nxg_record_entries does: kept
 *     iff key[p] < tab->n_subs and arch_id_of_sub[key[p]] != NXG_NO_SLOT. Called with d->ent_sub,
 *     d->chan_off, d->n_entries and the recorder's table, the call yields the index of exactly the
 *     record nxg_record_entries wrote for each channel; the file's record is index[c] | batch[c].
 * Record c's index is  varint(L) varint(count) varint(id)...  where `inner` is the bytes from the
 * count on and L = inner + varint_len(inner + varint_len(inner)) (len_wrapped_len, pack.rs:522-525):
 * its distinct kept Ids, each once, in order of first occurrence. (The reference drains a
 * FxHashSet, whose order nobody can pin; the reader is order-blind.) A record with no kept position
 * gets no bytes, as add_batch writes nothing for an empty batch (writer.rs:405): idx_off[c] ==
 * idx_off[c+1], idx_ids[c] == 0. Indexes lie back to back in record order: idx_off[0] == 0,
 * idx_off[n_recs] == n_bytes. The index of an *image* record is the constant 02 00 (writer.rs:408
 * inserts nothing): the host writes those two bytes itself, this call is for delta records.
 * false with a message:
 *   on misuse, before any launch (a null argument, host memory, more than 2^28 positions, async
 *     work pending on the ctx);
 *   when seg_off decreases (the message names the lowest record c with seg_off[c+1] < seg_off[c])
 *     or ends behind n_keys (the last record);
 *   for an Id >= 2^32 (tab == NULL);
 *   when idx_ids[c] * 4 exceeds MAX_VEC (PackError::TooBig, pack.rs:943; the first such record);
 *   when n_bytes > cap_bytes: n_bytes, n_ids_total, idx_off and idx_ids then hold the true values.
 * Every check and every size is settled before the first byte of `out` is written: after any false
 * return no byte of `out` has changed. Whatever the outcome, nothing outside [out, out +
 * cap_bytes), idx_off[0 .. n_recs] and idx_ids[0 .. n_recs) is written. n_recs == 0 or n_keys == 0
 * gives all zeros and launches nothing: with no keys seg_off is not examined (its entries are not
 * read, so one that would end behind n_keys is not refused). Synchronous, one read-back of a small
 * head; out NULL sizes only.
 * Memory: the context keeps a table of 12 bytes per slot, a power of two >= 2 * n_keys slots (384
 * MiB at 10^7 positions, 6 GiB at the limit of 2^28), and 9 bytes per position of scratch. Both
 * are grown on demand and stay with the context at the size of its largest call until
 * nxg_ctx_destroy; a caller that cannot afford that splits its records over several calls. */
typedef struct NxgArchiveIndexes {
    uint64_t cap_bytes;  /* capacity of out */
    uint8_t* out;        /* device; NULL: size only */
    uint64_t* idx_off;   /* device [n_recs + 1]: record c's RecordIndex is out[idx_off[c], idx_off[c+1]) */
    uint64_t* idx_ids;   /* device [n_recs]: distinct Ids in record c's index */
    uint64_t n_bytes, n_ids_total;   /* written by the call */
} NxgArchiveIndexes;
bool nxg_archive_index_records(NxgCtx* ctx, const uint64_t* key, uint64_t n_keys,
                               const uint64_t* seg_off, uint32_t n_recs,
                               const NxgRecordTable* tab /* may be NULL */, NxgArchiveIndexes* out,
                               NetidxError* err);

/* nxg_archive_scan_index replaces scan_index_at (reader.rs:394-422), the test matching_idxs
 * (reader.rs:559-581) makes of every record of a filtered read: n records in one call. dbuf is
 * device memory of buf_len bytes; record i's RecordIndex starts at dbuf + idx_off[i] (past the
 * RecordHeader, and past the u32 of a compressed record) and its record ends at idx_end[i]
 * (idx_off, idx_end and verdict are host memory). keep[a] != 0 iff archive Id a is in the filter
 * set: the array nxg_archive_build_image takes (device, n_ids bytes).
 * verdict[i] is scan_index_at, statement by statement:
 *   index_len = decode_varint; a failure is NXG_INDEX_ERR_SHORT or NXG_INDEX_ERR_FORMAT.
 *   The body is the index_len - varint_len(index_len) bytes behind the bytes that varint consumed
 *   (a non-canonical 81 00 consumes two), clipped at idx_end[i] (Buf::take clips, it does not fail).
 *   The body is walked varint by varint; the Vec's count is one of them, because the reference does
 *   not skip it: a record whose count equals a kept Id matches, and 02 00 matches iff keep[0].
 *   Each value is truncated to u32 (Id(id as u32): the varint of 2^32 + 5 tests keep[5]); it hits
 *   when it is < n_ids and kept. The first hit ends the walk with NXG_INDEX_MATCH, so errors behind
 *   a hit are never seen; otherwise the first failing varint gives the verdict, NXG_INDEX_ERR_FORMAT
 *   for ten continuation bytes inside the body, NXG_INDEX_ERR_SHORT when the body ends inside a
 *   varint; otherwise NXG_INDEX_NONE.
 * The reference logs an error and skips the record; whether to skip stays the caller's decision.
 * Deviations: index_len == 0 underflows in the reference, here it is NXG_INDEX_ERR_FORMAT; the
 * reference's slice runs to the end of the mmap, ours to the record's end.
 * *n_match (may be NULL) counts the NXG_INDEX_MATCH verdicts. One launch covers all records, one
 * pinned copy up, one read-back; n == 0 launches nothing. false on misuse: a null argument, a host
 * dbuf or keep, idx_off[i] > idx_end[i], idx_end[i] > buf_len, async work pending on the ctx. */
#define NXG_INDEX_NONE 0
#define NXG_INDEX_MATCH 1
#define NXG_INDEX_ERR_SHORT 2    /* PackError::BufferShort */
#define NXG_INDEX_ERR_FORMAT 3   /* PackError::InvalidFormat */
bool nxg_archive_scan_index(NxgCtx* ctx, const uint8_t* dbuf, uint64_t buf_len,
                            const uint64_t* idx_off, const uint64_t* idx_end /* host [n] each */,
                            uint32_t n, const uint8_t* keep /* device [n_ids] */, uint64_t n_ids,
                            uint8_t* verdict /* host [n] */, uint64_t* n_match, NetidxError* err);

/* ---- compressed archive batches: replaces the compressed branch of ArchiveReader::get_batch_at
 * (netidx-archive/src/logfile/reader.rs:453-477): a record after its RecordHeader is
 * u32 BE uncompressed record length | the RecordIndex (indexed files: a varint that is its own
 * length, then the ids) | one zstd frame of the batch, compressed with the archive's dictionary
 * (reader.rs:243-244, 737-801; zstd 0.13 = libzstd 1.5, RFC 8878). The frames are decompressed on
 * the device, many records per call; nxg_decode_archive_batch then decodes each batch.
 * A dictionary (the archive's, from its header): zstd format (magic EC30A437: entropy tables,
 * repeat offsets, content) or raw content. */
typedef struct NxgZstdDict NxgZstdDict;
NxgZstdDict* nxg_zstd_dict_new(NxgCtx* ctx, const uint8_t* dict, uint64_t len, NetidxError* err);
void nxg_zstd_dict_free(NxgZstdDict* d);
/* one record: in, its bytes [off, off + len) of `src` (after the RecordHeader); out, its batch at
 * [out_off, out_off + out_len) of `dout` (each record has room for its uncompressed length), and
 * err: 0, or 1 not a zstd frame / trailing bytes, 2 corrupt, 3 the batch is longer than the
 * record's uncompressed length, 4 dictionary missing or of another id, 5 checksum mismatch, 6
 * frame content size mismatch, 7 record too short. A record's failure is its own (the
 * reference fails that get_batch); the others are decompressed. */
typedef struct NxgArchiveRecord {
    uint64_t off, len;
    uint64_t out_off, out_len;
    uint32_t err, pad;
} NxgArchiveRecord;
/* src: host memory (the archive's mmap), src_len bytes; dout: device memory of `cap` bytes (NULL:
 * *need = the bytes the records need). dict may be NULL (frames without a dictionary). The host
 * reads the records' lengths and index prefixes; the frames go to the device in one copy.
 * Synchronous. Returns false on misuse, a HIP failure or cap < *need. */
bool nxg_archive_decompress(NxgCtx* ctx, const NxgZstdDict* dict, const uint8_t* src,
                            uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                            uint8_t* dout, uint64_t cap, uint64_t* need, NetidxError* err);

/* replaces compress_task of ArchiveReader::compress (reader.rs:741-769), many records per call:
 * record i is src[recs[i].off, + recs[i].len), the bytes after its RecordHeader of an uncompressed
 * archive: the RecordIndex when `indexed` (its first varint is the index's own length), then the
 * packed batch. Its compressed record -- u32 BE recs[i].len | the index bytes verbatim | one zstd
 * frame of the batch (Single_Segment with the content size, no checksum, the Dictionary_ID in its
 * smallest field for a zstd-format dictionary, none for raw content or dict == NULL) -- is written
 * to out[recs[i].out_off, + recs[i].out_len), the bytes add_batch_raw takes. Slots are disjoint,
 * in record order and not contiguous: each has its record's worst case, 4 + index + 17 + batch +
 * 3 per 128 KiB block. recs[i].err: 0, or 7 when the record is shorter than its index prefix (that
 * record alone fails). The frames are not libzstd's bytes; libzstd and nxg_archive_decompress
 * turn them back into the batch, and the same record and dictionary give the same bytes in every
 * call. src and out are host memory; out == NULL: *need = the bytes of all slots, computed on the
 * host. Synchronous. Returns false on misuse, a HIP failure, cap < *need, or a record of 2^32
 * bytes or more. */
bool nxg_archive_compress(NxgCtx* ctx, const NxgZstdDict* dict, const uint8_t* src,
                          uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                          uint8_t* out, uint64_t cap, uint64_t* need, NetidxError* err);
/* nxg_archive_compress with options (NULL: the defaults, which is nxg_archive_compress itself).
 * literals: how a block's literals may be Huffman-coded.
 *   NXG_ZSTD_LIT_DICT_TREE (0): with the dictionary's tree only (Treeless_Literals_Block); frames
 *     without a zstd-format dictionary have raw literals.
 *   NXG_ZSTD_LIT_BLOCK_TREES (1): a block may also build a tree from its own literals (code
 *     lengths of at most 11 bits) and describe it (Compressed_Literals_Block; direct or
 *     FSE-compressed weights), when that section is smaller than raw, RLE and the treeless form
 *     with the tree the frame's reader has at that block -- the dictionary's, or the last one a
 *     block of the frame described. No dictionary is needed for Huffman-coded literals.
 * Slots, record layout, errors and determinism are those of nxg_archive_compress; a frame of one
 * block, and every frame without a zstd-format dictionary, is never larger than with literals
 * 0. An unknown `literals` value or a non-zero `reserved` word fails the call. */
enum { NXG_ZSTD_LIT_DICT_TREE = 0, NXG_ZSTD_LIT_BLOCK_TREES = 1 };
typedef struct NxgZstdCompressOpts {
    uint32_t literals;
    uint32_t reserved[3];
} NxgZstdCompressOpts;
bool nxg_archive_compress_opts(NxgCtx* ctx, const NxgZstdDict* dict, const uint8_t* src,
                               uint64_t src_len, NxgArchiveRecord* recs, uint32_t n, bool indexed,
                               const NxgZstdCompressOpts* opts /* NULL = defaults */,
                               uint8_t* out, uint64_t cap, uint64_t* need, NetidxError* err);

/* ---- a window of archive records: replaces the get_batch_at loops of ArchiveReader::read_deltas
 * (netidx-archive/src/logfile/reader.rs:590-631, up to n records per call; recorder/oneshot.rs:141
 * asks for 1000) and ArchiveReader::build_image (reader.rs:492-557).
 * Record i's batch is dbuf[recs[i].out_off, + recs[i].out_len); dbuf is device memory of buf_len
 * bytes. The array nxg_archive_decompress fills feeds straight in; for an uncompressed archive the
 * host fills out_off / out_len itself, past the RecordHeader and the index. A record with
 * recs[i].err != 0 is skipped: its info has zero rows and err_kind 0 (the caller has recs[i].err).
 * Bytes after a batch inside its slot are not read; slots need not be contiguous or ordered.
 * Output: MIXED-layout device columns holding the rows of all batches back to back, in record
 * order, then item order. id / tag / fixed / aux mean what they mean for nxg_decode_archive_batch,
 * except that text offsets index dbuf (absolute, not the record) and that container `fixed` and
 * child `cfixed` index out's child arrays (absolute). out->n_rows / n_children are the totals.
 * info[i] (host memory, n entries): the record's rows [row_off, + n_rows) and children
 * [child_off, + n_children) in `out`, consumed = its batch's length in bytes, and the status
 * nxg_decode_archive_batch gives for the same bytes: err_kind / err_offset (relative to the
 * record's batch start) and path -- NXG_PATH_ARCHIVE_WINDOW for a record the window's own kernels
 * decoded, else the path of the single-batch decoder it went through.
 * A record that fails, fails alone: its info carries (err_kind, err_offset), it has no rows
 * (n_rows = n_children = consumed = 0), and the others decode; the reference's `?` on the first
 * failure is the caller's decision.
 * Routes: records shorter than opts->big_record_bytes bytes go to the window's kernels (one wave per
 * record); those decline what the fast single-batch path declines (an Id wider than 5 bytes, Maps,
 * Error(Value), nested or 128+-element Arrays, any parse error, a count the items do not bear
 * out). Records of that length or more, and declined ones, go through nxg_decode_archive_batch, unchanged, into
 * scratch columns of the ctx and are copied to their place. big_record_bytes 0 (or opts NULL) is
 * the default, NXG_ARCHIVE_WINDOW_BIG_DEFAULT; 1 sends every record through the single-batch
 * decoder; UINT64_MAX every record that is not declined through the window's kernels. The result
 * does not depend on the route.
 * Capacity: when out->cap_rows or out->cap_children is too small the call returns false with
 * *need_rows / *need_children set to the exact totals (they are written on success too). A-priori
 * bounds: rows <= sum(out_len) / 2, children <= sum(out_len).
 * Misuse (false): a null argument, columns that are not device MIXED columns, a record outside
 * buf_len, an async operation pending on the ctx. Synchronous. */
#define NXG_PATH_ARCHIVE_WINDOW 7
#define NXG_ARCHIVE_WINDOW_BIG_DEFAULT 131072
typedef struct NxgArchiveBatchInfo { /* one per record, written by the call */
    uint64_t row_off, n_rows;        /* the record's rows in `out`, record order then item order */
    uint64_t child_off, n_children;
    uint64_t consumed;               /* the batch's length in bytes */
    int32_t err_kind;                /* as nxg_decode_archive_batch's status */
    uint32_t path;                   /* which decoder */
    uint64_t err_offset;             /* relative to the record's batch start */
} NxgArchiveBatchInfo;
typedef struct NxgArchiveWindowOpts {
    uint64_t big_record_bytes; /* 0 = default */
} NxgArchiveWindowOpts;
bool nxg_archive_decode_window(NxgCtx* ctx, const uint8_t* dbuf, uint64_t buf_len,
                               const NxgArchiveRecord* recs, uint32_t n,
                               const NxgArchiveWindowOpts* opts /* NULL = defaults */,
                               NxgColumns* out, NxgArchiveBatchInfo* info, uint64_t* need_rows,
                               uint64_t* need_children, NetidxError* err);

/* The image of a decoded window: replaces the image.extend(...) fold of build_image
 * (reader.rs:519-552), a HashMap::extend in record order, then item order. For each Id the value
 * of its last row in `window` (the columns nxg_archive_decode_window wrote). Event::Unsubscribed
 * is a value like any other: it stays in the image as tag NXG_TAG_UNSUBSCRIBED. With `keep`
 * (n_ids bytes of device memory; NULL = every Id) rows whose Id has keep[id] == 0 are dropped, as
 * the reference's filter drops them (reader.rs:519-525, 546-552); n_filtered counts those rows.
 * Archive Ids come from a counter (writer.rs:314-315) and the reader knows max_id
 * (reader.rs:226-237): n_ids = max_id + 1. An Id >= n_ids is a false return whose message names
 * the Id and the row; a well-formed archive has none.
 * Output: the caller's device arrays of cap_rows entries each (cap_rows >= min(n_ids, the window's
 * rows) always suffices; fewer is a false return): id, tag, fixed, aux of each winner and src_row,
 * its row in the window, in ascending Id order (the reference's map has no order; this one is
 * deterministic). n_rows and n_filtered are written by the call.
 * The image borrows the window: children and text stay where the window decode put them. An
 * NxgColumns made of the image's row arrays (n_rows, cap_rows) and the window's child arrays
 * (n_children, cap_children) is accepted as it is by nxg_encode_archive_batch(..., heap = dbuf,
 * ...) -- the encoder reaches children only through `fixed` -- and its bytes are the image record
 * the writer stores. Chaining over windows needs no further call: encode the image and make it
 * record 0 of the next window. Synchronous; false on misuse (null arguments, non-device columns, an
 * async operation pending) or a HIP failure. */
typedef struct NxgArchiveImage {
    uint64_t cap_rows; /* >= min(n_ids, window rows) */
    uint64_t* id;      /* device arrays of cap_rows entries */
    uint8_t* tag;
    uint64_t* fixed;
    uint32_t* aux;
    uint64_t* src_row;           /* the winning row's index in the window columns */
    uint64_t n_rows, n_filtered; /* written by the call */
} NxgArchiveImage;
bool nxg_archive_build_image(NxgCtx* ctx, const NxgColumns* window, uint64_t n_ids,
                             const uint8_t* keep /* [n_ids] device, NULL = every Id */,
                             NxgArchiveImage* out, NetidxError* err);

/* ---- playback: replaces the loop of the recorder's publish session over a batch (netidx-archive/
 * src/recorder/publish/session_shard.rs:196-245, process_batch) and over the pathmap (reimage,
 * session_shard.rs:375-409). For every BatchItem(id, ev) the reference turns Event::Unsubscribed
 * into Value::Null, looks the archive Id up in `published: FxHashMap<Id, Val>` (session_shard.rs:42),
 * calls val.update(&mut pbatch, v) on a hit, publishes the path on a miss when it has one and the
 * session's filter matches it, and drops anything else; then pbatch.commit. Here a decoded window
 * becomes the update rows of all its records in one call, in the form nxg_publish_commit,
 * nxg_encode_clients and nxg_value_table_apply take.
 * `window` and `info` are what nxg_archive_decode_window produced (info: host memory, n_recs
 * entries; only row_off and n_rows are read). Record i's rows are window rows [info[i].row_off, +
 * info[i].n_rows); a sub-range of the infos (info + k, n_recs - k) is as good as all of them.
 * Window rows in front of, between or behind the records belong to none: they are neither read,
 * kept nor counted.
 * The table is `published` with the host's knowledge folded in: pub_id_of_arch[a] is the publisher
 * Id of archive Id a, NXG_REPLAY_DROP when a has no path or the session's filter does not match it
 * (the reference's silent drop), or NXG_REPLAY_MISS when it has a path the filter matches and is
 * not published yet.
 * Row by row in window order, with a = window->id[r]:
 *   miss: a >= tab->n_ids, or the table holds NXG_REPLAY_MISS (the reference would call
 *     path_for_id here, the host's knowledge);
 *   drop: the table holds NXG_REPLAY_DROP; counted in n_dropped;
 *   kept: anything else. The output row is (id = pub_id_of_arch[a], tag, fixed, aux, src_row = r):
 *     tag NXG_TAG_UNSUBSCRIBED becomes Value::Null (tag 16, fixed 0, aux 0), every other value is
 *     copied verbatim -- container `fixed` still indexes the window's child arrays and text `fixed`
 *     still indexes dbuf. An NxgColumns made of the row arrays (n_rows, cap_rows) and the window's
 *     child arrays is a batch for nxg_publish_commit(..., heap = dbuf, ...), as the image's is for
 *     the encoder.
 * The call stops in front of a miss, as nxg_route_writes stops in front of a Subscribe: publishing
 * is the host's job and changes the table for every later item. n_done is the lowest record that
 * holds a miss, or n_recs when none does, whatever the scheduling. Records [0, n_done) are emitted
 * and nothing of later records is: record i's updates are rows [rec_off[i], rec_off[i+1]),
 * rec_off[0] == 0, rec_off[i] == rec_off[n_done] for i > n_done, n_rows == rec_off[n_recs], and
 * n_dropped counts the drops of records [0, n_done) only. miss_row[0 .. min(n_miss, cap_miss))
 * lists the window rows of record n_done that missed, in item order; n_miss is their true count
 * (0 when n_done == n_recs). The caller publishes those Ids (publisher.publish(path, v), the first
 * row per Id), updates its table and calls again from record n_done (info + n_done, n_recs -
 * n_done). On that second call the publishing row comes back as an Update of a value that equals
 * `current` and has no subscriber yet, which changes neither a client's bytes nor `current`: the
 * protocol is observably the reference's. After reimage has published the pathmap, misses happen
 * only when a live recording adds paths, so the stop is rare; it costs a second small launch and
 * read-back.
 * Val::update is NXG_PUB_UPDATE: whether a row is sent does not depend on `current`. One
 * nxg_publish_commit over rows [0, n_rows) therefore gives every client the concatenation, in
 * record order, of what per-record commits give, and its last_row is the last per-record one
 * shifted by rec_off. Speed::Unlimited commits a window at once; Speed::Limited commits
 * per-record views, the same arrays at pointer offset rec_off[i].
 * false with a message:
 *   on misuse, before any launch: a null argument, columns that are not device MIXED columns,
 *     host memory, async work pending on the ctx, an info whose rows leave window->n_rows, whose
 *     row_off decreases or whose rows overlap the record before;
 *   when cap_rows is smaller than the kept rows of [0, n_done): n_rows holds the need (n_dropped,
 *     n_done, n_miss, rec_off and miss_row are written as on success) and no row is written.
 *     cap_rows >= window->n_rows always suffices.
 * Whatever the outcome, nothing is written outside [0, cap_rows) of each row array,
 * rec_off[0 .. n_recs] and miss_row[0 .. cap_miss). n_recs == 0 or no rows gives all zeros and
 * n_done = n_recs. Synchronous, one read-back of a small head on the common path. */
#define NXG_REPLAY_DROP  0xffffffffffffffffull  /* no path, or the session's filter does not match it */
#define NXG_REPLAY_MISS  0xfffffffffffffffeull  /* has a path the filter matches, not yet published */
typedef struct NxgReplayTable {      /* `published`, session_shard.rs:42, with the host's filter folded in */
    uint64_t n_ids;                  /* pub_id_of_arch covers archive Ids [0, n_ids) */
    const uint64_t* pub_id_of_arch;  /* device: the publisher Id, NXG_REPLAY_DROP or NXG_REPLAY_MISS */
} NxgReplayTable;
typedef struct NxgReplayRows {       /* caller's device arrays, cap_rows entries each */
    uint64_t cap_rows;
    uint64_t* id; uint8_t* tag; uint64_t* fixed; uint32_t* aux;
    uint64_t* src_row;               /* the row's index in the window (or image) columns */
    uint64_t* rec_off;               /* device [n_recs + 1]: record i's updates are rows [rec_off[i], rec_off[i+1]) */
    uint64_t* miss_row; uint64_t cap_miss;    /* device: window rows of the stopping record that missed */
    uint64_t n_rows, n_dropped, n_done, n_miss;   /* written by the call */
} NxgReplayRows;
bool nxg_replay_window(NxgCtx* ctx, const NxgColumns* window, const NxgArchiveBatchInfo* info,
                       uint32_t n_recs, const NxgReplayTable* tab, NxgReplayRows* out,
                       NetidxError* err);
/* reimage (session_shard.rs:375-409, on every seek and at session start): every Id of the pathmap
 * gets its image value, or Null when the image has none or has Unsubscribed. `image` is what
 * nxg_archive_build_image produced (ids ascending; only id / tag / fixed / aux and n_rows are
 * read); order[0 .. n_order) are the pathmap's archive Ids in iter_pathmap order, device memory,
 * in any order, duplicates tolerated; `tab` as above. The output is one record (rec_off has 2
 * entries, n_done == 1 always): for each order[j] that is kept, the row (pub id, the image's value,
 * src_row = the image row); when the image has no row for the Id, or has Unsubscribed, the row is
 * Null with src_row = UINT64_MAX. The Id is found by bisection over the image's sorted ids. Drops
 * are counted. Nothing depends on a miss inside one reimage, so misses do not stop the call: every
 * position j that missed is listed in miss_row, in order, and n_miss is exact even past cap_miss.
 * Errors, bounds and synchrony as nxg_replay_window; cap_rows >= n_order always suffices. */
bool nxg_replay_image(NxgCtx* ctx, const NxgArchiveImage* image, const uint32_t* order,
                      uint64_t n_order, const NxgReplayTable* tab, NxgReplayRows* out,
                      NetidxError* err);

/* ---- oneshot queries: replaces do_oneshot's reply (netidx-archive/src/recorder/oneshot.rs:100-157,
 * packed at oneshot.rs:194). OneshotReply(Vec<OneshotReplyShard>) and OneshotReplyShard { pathmap,
 * image, deltas } are #[derive(Pack)] (recorder_client.rs:29-37), so both are length-wrapped
 * (netidx-derive/src/lib.rs:113,137; len_wrapped_len, pack.rs:522-525):
 *   reply   = varint(Lr) varint(n_shards) shard...
 *   shard   = varint(Ls) pathmap image deltas
 *   pathmap = varint(n) { varint(id) varint(len) path bytes }...    FxHashMap<Id, Path> (pack.rs:
 *             1113-1124; Id: logfile/mod.rs:154-166; Path: path.rs:61-68 over ArcStr, pack.rs:444-455)
 *   image   = varint(n) { varint(id) Event }...                     FxHashMap<Id, Event>
 *   deltas  = varint(n) { i64 BE secs, u32 BE subsec nanos, varint(count) { varint(id) Event }... }...
 *             VecDeque<(DateTime<Utc>, Vec<BatchItem>)> (pack.rs:1064-1074, 1416-1424, 1555-1567,
 *             941-952)
 * A HashMap has no order anybody can pin and the decoder inserts into a map, so every map is
 * written in ascending Id order, as nxg_archive_build_image's image is. The image section is
 * exactly what nxg_encode_archive_batch writes for the columns of nxg_archive_build_image(keep =
 * sel).
 *
 * nxg_oneshot_pack_pathmap replaces oneshot.rs:111-120: the filter set and the pathmap section of
 * one shard. `paths` is the shard's path index in Id order (pathindex.index().iter_pathmap()), keep
 * is filter.is_match(path) per Id, computed by the host (glob matching stays there).
 *   sel[a] = 1 iff keep[a] != 0 and Id a has a path (a non-empty range), else 0. It is the
 *     reference's `filterset` and equally `pathmap.contains_key`: the `keep` array to hand to
 *     nxg_archive_scan_index and nxg_archive_build_image.
 *   out = varint(n_sel), then for every selected Id a in ascending order varint(a) varint(len) and
 *     the len bytes path_bytes[path_off[a], path_off[a+1]).
 * false with a message:
 *   on misuse, before any launch (a null argument by name, host memory, more than 2^32 Ids, async
 *     work pending on the ctx);
 *   when path_off decreases (the message names the lowest Id a with path_off[a+1] < path_off[a],
 *     whatever the scheduling);
 *   when n_sel * 12 exceeds MAX_VEC (PackError::TooBig, pack.rs:1115: size_of::<Id>() +
 *     size_of::<Path>(), an ArcStr being one pointer);
 *   when n_bytes > cap_bytes. In the last two cases n_bytes and n_sel hold the true values.
 * Every check and every size is settled before the first byte of `out` is written: after any false
 * return no byte of `out` has changed (sel may have been written). Whatever the outcome, nothing
 * outside [out, out + cap_bytes) and sel[0 .. n_ids) is written. n_ids == 0 gives the single byte
 * 00 and launches nothing. Synchronous, one read-back of a small head; out NULL sizes only (sel is
 * written all the same). */
typedef struct NxgOneshotPaths {      /* pathindex.index().iter_pathmap(), oneshot.rs:113 */
    uint64_t n_ids;                   /* archive Ids [0, n_ids) */
    const uint64_t* path_off;         /* device [n_ids + 1], non-decreasing; Id a's path is path_bytes[path_off[a], path_off[a+1]) */
    const uint8_t* path_bytes;        /* device, not NULL when n_ids > 0; an empty range: Id a has no path */
} NxgOneshotPaths;
typedef struct NxgOneshotPathmap {
    uint64_t cap_bytes; uint8_t* out; /* device; NULL: size only */
    uint8_t* sel;                     /* device [n_ids], written by the call: 1 iff keep[a] != 0 and a has a path */
    uint64_t n_bytes, n_sel;          /* written by the call */
} NxgOneshotPathmap;
bool nxg_oneshot_pack_pathmap(NxgCtx* ctx, const NxgOneshotPaths* paths,
                              const uint8_t* keep /* device [n_ids] */, NxgOneshotPathmap* out,
                              NetidxError* err);

/* nxg_oneshot_pack_deltas replaces oneshot.rs:146-149 for one window of read_deltas:
 * batch.retain(|BatchItem(id, _)| pathmap.contains_key(id)), the drop of the records that end up
 * empty, and the deltas elements of the records that remain. `window`, `info` and `dbuf` are what
 * nxg_archive_decode_window produced and read (device MIXED columns; text at dbuf + fixed); only
 * row_off and n_rows of info are read, and window rows outside the records belong to none: they
 * are neither read, kept nor counted. ts_secs / ts_nanos are the DateTime<Utc> read_deltas pairs
 * with each record (reader.rs:617-627), written verbatim as put_i64(secs) put_u32(nanos)
 * (pack.rs:1555-1567): a leap second's nanos of 1 999 999 999 included, nothing is validated.
 * `sel` is nxg_oneshot_pack_pathmap's (any keep array of that form).
 *   Window row r of record i is kept iff window->id[r] < n_ids and sel[id] != 0. Any other row is
 *   dropped and counted in n_dropped, and nothing else of it is read (a dropped row with a bad tag
 *   is not an error): the rule nxg_record_entries has.
 *   A record with a kept row becomes the element  secs nanos varint(rec_items[i]) item...,  each
 *   item varint(id) Event, byte for byte what nxg_encode_archive_batch(..., heap = dbuf, ...) writes
 *   for those rows. A record that keeps nothing gets no bytes (oneshot.rs:148): rec_off[i] ==
 *   rec_off[i+1], rec_items[i] == 0, and it is not counted in n_kept_recs.
 * Elements lie back to back in record order: rec_off[0] == 0, rec_off[n_recs] == n_bytes. The
 * output is the deltas section without its leading count: the fragments of successive windows
 * concatenate into one section (the reference's loop accumulates windows, oneshot.rs:139-156), and
 * nxg_oneshot_shard_layout takes their summed n_bytes and n_kept_recs.
 * false with a message:
 *   on misuse, before any launch (a null argument by name, columns that are not device MIXED
 *     columns, host memory, more than 2^32 Ids, 2^39 rows or more, async work pending on the ctx, an
 *     info whose rows leave window->n_rows, whose row_off decreases or whose rows overlap the record
 *     before, as nxg_replay_window);
 *   for a kept row with an unknown tag, that violates a size guard (PackError::TooBig), has a child
 *     range outside n_children, is a container with elements but no child columns, or nests past
 *     NXG_MAX_DEPTH: the message names the lowest such window row and its cause, whatever the
 *     scheduling;
 *   when rec_items[i] * size_of::<BatchItem>() (24) exceeds MAX_VEC (TooBig; the first such record);
 *   when n_bytes > cap_bytes: n_bytes, n_items, n_dropped, n_kept_recs, rec_off and rec_items then
 *     hold the true values.
 * Every check and every size is settled before the first byte of `out` is written: after any false
 * return no byte of `out` has changed. Whatever the outcome, nothing outside [out, out +
 * cap_bytes), rec_off[0 .. n_recs] and rec_items[0 .. n_recs) is written. n_recs == 0, or records
 * without rows, gives all zeros and launches nothing. Synchronous, one copy up of the records' rows
 * and timestamps, one read-back of a small head; out NULL sizes only. */
typedef struct NxgOneshotDeltas {
    uint64_t cap_bytes; uint8_t* out;   /* device; NULL: size only */
    uint64_t* rec_off;                  /* device [n_recs + 1]: record i's element is out[rec_off[i], rec_off[i+1]) */
    uint64_t* rec_items;                /* device [n_recs]: items kept in record i */
    uint64_t n_bytes, n_items, n_dropped, n_kept_recs;   /* written by the call */
} NxgOneshotDeltas;
bool nxg_oneshot_pack_deltas(NxgCtx* ctx, const NxgColumns* window, const uint8_t* dbuf,
                             const NxgArchiveBatchInfo* info /* host [n_recs] */, uint32_t n_recs,
                             const int64_t* ts_secs, const uint32_t* ts_nanos /* host [n_recs] each */,
                             const uint8_t* sel /* device [n_ids] */, uint64_t n_ids,
                             NxgOneshotDeltas* out, NetidxError* err);

/* The framing of a shard and of the reply: host arithmetic, no ctx.
 * nxg_oneshot_shard_layout: from the lengths of the shard's pathmap and image sections, the summed
 * bytes of its deltas fragments (deltas_len) and the number of delta records in them (n_deltas),
 * the two small heads and where everything lies. With inner = pathmap_len + image_len +
 * varint_len(n_deltas) + deltas_len, Ls = len_wrapped_len(inner) = inner + varint_len(inner +
 * varint_len(inner)); the shard is len_head | pathmap | image | count_head | fragments.
 * nxg_oneshot_reply_head: from the shards' lengths, head = varint(Lr) varint(n_shards) (at most 20
 * bytes) with Lr = len_wrapped_len(varint_len(n_shards) + the shards' bytes); *reply_len (may be
 * NULL) = the head and the shards. The reply is head | shard | shard ... .
 * VecDeque::encode and Vec::encode guard count * size_of::<T>() against MAX_VEC (pack.rs:1066,
 * 943); the element sizes involve GPooled<..> and are not pinned by the reference tree, so both
 * calls refuse a count above MAX_VEC / 64 (n_deltas; n_shards). Besides that: a null argument, a
 * section of 2^60 bytes or more, shards that sum to 2^60 bytes or more. */
typedef struct NxgOneshotShardLayout {
    uint64_t pathmap_len, image_len, deltas_len, n_deltas;   /* as given */
    uint64_t pathmap_off, image_off, count_off, deltas_off;  /* where each part starts in the shard */
    uint64_t shard_len;                                      /* all of the shard, len_head included */
    uint32_t len_head_len, count_head_len;
    uint8_t len_head[10];                                    /* varint(Ls), at offset 0 */
    uint8_t count_head[10];                                  /* varint(n_deltas), at count_off */
    uint8_t pad[4];
} NxgOneshotShardLayout;
bool nxg_oneshot_shard_layout(uint64_t pathmap_len, uint64_t image_len, uint64_t deltas_len,
                              uint64_t n_deltas, NxgOneshotShardLayout* out, NetidxError* err);
bool nxg_oneshot_reply_head(const uint64_t* shard_len, uint64_t n_shards, uint8_t* head /* [20] */,
                            uint32_t* head_len, uint64_t* reply_len, NetidxError* err);
/* A shard put together in device memory: `layout` as nxg_oneshot_shard_layout made it, pathmap and
 * image the sections (device, layout->pathmap_len and ->image_len bytes), frags the deltas
 * fragments in order (device; a fragment of length 0 is skipped). Device-to-device copies to the
 * layout's offsets on the ctx's stream, the two heads from pinned staging; *len_out (may be NULL) =
 * layout->shard_len. Synchronous. false, before anything is copied: a null argument by name, a
 * layout that is not nxg_oneshot_shard_layout's, fragments whose lengths do not sum to
 * layout->deltas_len, cap < layout->shard_len, host memory, async work pending on the ctx. Nothing
 * outside [out, out + cap) is written. */
typedef struct NxgOneshotFrag {
    const uint8_t* ptr;   /* device */
    uint64_t len;
} NxgOneshotFrag;
bool nxg_oneshot_assemble_shard(NxgCtx* ctx, const NxgOneshotShardLayout* layout,
                                const uint8_t* pathmap, const uint8_t* image,
                                const NxgOneshotFrag* frags, uint32_t n_frags, uint8_t* out,
                                uint64_t cap, uint64_t* len_out, NetidxError* err);

/* ---- the publisher <-> subscriber connection (BASELINE configs[0]) ------------------------
 * Replaces hello_publisher (netidx/src/subscriber/connection.rs:120-140), ClientCtx::hello
 * (publisher/server.rs:367-381), read_task / flush_buf (channel.rs:107-126, 379-443) and the
 * To::Subscribe -> From::Subscribed exchange (publisher/server.rs:60-137, 506-516), anonymous
 * authentication only. Raw handshake messages are a u32 big-endian length + the packed value
 * (channel.rs:63-105): u64 3 both ways, then Hello::Anonymous both ways. After the handshake
 * the connection is a Channel of frames (nxg_frame_header) holding len-wrapped messages.
 * Sessions are blocking sockets; one thread per session. */
typedef struct NxgSession NxgSession;
/* subscriber side: connect and run the handshake */
NxgSession* nxg_session_connect(const char* ipv4, uint16_t port, NetidxError* err);
/* publisher side: a listening socket (port 0: any; *bound_port receives it), then one accepted,
 * handshaken connection per nxg_session_accept */
NxgSession* nxg_session_listen(const char* ipv4, uint16_t port, uint16_t* bound_port,
                               NetidxError* err);
NxgSession* nxg_session_accept(NxgSession* listener, NetidxError* err);
void nxg_session_close(NxgSession* s);
/* frames_in, bytes_in, frames_out, bytes_out */
void nxg_session_stats(const NxgSession* s, uint64_t out[4]);
/* one frame out: u32 header (channel.rs:107-126) + payload (<= MAX_BATCH) */
bool nxg_session_send(NxgSession* s, const uint8_t* payload, uint64_t len, NetidxError* err);
/* the next complete frame in (read_task, channel.rs:379-443): *payload stays valid until the
 * next receive on this session; encrypted frames are refused */
bool nxg_session_recv_frame(NxgSession* s, const uint8_t** payload, uint64_t* len,
                            NetidxError* err);
/* the data path, subscriber side: the next frame, read into page-locked memory, decoded on the
 * device into `out` as nxg_decode_updates does (status, flags likewise) */
bool nxg_session_recv_decode(NxgSession* s, NxgCtx* ctx, NxgColumns* out, uint32_t flags,
                             NxgStatus* status, uint64_t* frame_len, NetidxError* err);
/* the data path, publisher side: device columns encoded on the GPU (nxg_encode_frames: the
 * MAX_BATCH cuts), copied to page-locked memory and written as frames */
bool nxg_session_publish(NxgSession* s, NxgCtx* ctx, const NxgColumns* cols, const uint8_t* heap,
                         uint64_t* bytes_sent, NetidxError* err);
/* Control messages (len-wrapped derived enums, netidx-derive lib.rs:289-381). Builders return
 * the message length (out NULL: the length only) or -NXG_CAPACITY / -NXG_UNKNOWN_TAG. */
/* To::Subscribe { path, resolver: SocketAddr::V4, timestamp, permissions, token }
 * (netproto publisher.rs:57-63) */
int64_t nxg_msg_subscribe(const char* path, uint64_t path_len, uint32_t resolver_ipv4,
                          uint16_t resolver_port, uint64_t timestamp, uint32_t permissions,
                          const uint8_t* token, uint64_t token_len, uint8_t* out, uint64_t cap);
/* From::Subscribed(path, id, value) with a scalar value (tag/fixed/aux as NxgColumns; String and
 * Bytes bytes at `text`) */
int64_t nxg_msg_subscribed(const char* path, uint64_t path_len, uint64_t id, uint8_t tag,
                           uint64_t fixed, uint32_t aux, const uint8_t* text, uint8_t* out,
                           uint64_t cap);
/* From::Heartbeat (2 bytes) */
int64_t nxg_msg_heartbeat(uint8_t* out, uint64_t cap);
/* From::Update(id, value) with a scalar value (tag/fixed/aux as NxgColumns; String and Bytes
 * bytes at `text`): one message as Val::update + commit queue it (publisher/mod.rs:517-519,
 * 776-845) and handle_updates encodes it (server.rs:604-629) -- the host path of a publisher
 * that updates one value at a time (BASELINE configs[0]). */
int64_t nxg_msg_update(uint64_t id, uint8_t tag, uint64_t fixed, uint32_t aux,
                       const uint8_t* text, uint8_t* out, uint64_t cap);
/* One control message parsed: to = 0 a publisher::From, 1 a publisher::To. Offsets index `buf`.
 * value_fixed holds scalar payloads as read (big-endian integers, varints as decoded, zigzag
 * not undone); other values are reported by tag and span. */
typedef struct NxgCtlMsg {
    uint64_t msg_len; /* the message's bytes (len-wrapped region) */
    uint32_t variant;
    uint32_t permissions;
    uint64_t id;
    uint64_t path_off, path_len;
    uint64_t timestamp;
    uint64_t token_off, token_len;
    uint64_t value_off, value_len; /* the value's bytes, tag included */
    uint64_t value_fixed;
    uint32_t value_tag, value_aux;
} NxgCtlMsg;
bool nxg_msg_parse(const uint8_t* buf, uint64_t len, int to, NxgCtlMsg* m, NetidxError* err);

/* ---- a machine-local anonymous resolver (BASELINE configs[0]) ------------------------------
 * The control plane the examples need to find each other, host only: the resolver server's
 * anonymous read and write paths (netidx/src/resolver_server/mod.rs:458-480, 771-860), the write
 * client's hello and ToWrite::Publish (resolver_client/write_client.rs:194-221), the read client's
 * hello and ToRead::Resolve -> FromRead::Publisher + FromRead::Resolved (read_client.rs:84-99,
 * resolver_server/shard_store.rs:160-193, 600-640). Blocking sockets; the server runs a thread per
 * client. Authentication other than anonymous, referrals and clustering are out of scope. */
typedef struct NxgResolver NxgResolver;
typedef struct NxgResolverClient NxgResolverClient;
NxgResolver* nxg_resolver_start(const char* ipv4, uint16_t port, uint16_t* bound_port,
                                uint64_t writer_ttl_secs, NetidxError* err);
void nxg_resolver_stop(NxgResolver* r);
uint64_t nxg_resolver_n_published(NxgResolver* r);
/* a publisher's resolver connection: ClientHello::WriteOnly { write_addr, Anonymous, Normal } */
NxgResolverClient* nxg_resolver_connect_write(const char* ipv4, uint16_t port,
                                              uint32_t write_ipv4, uint16_t write_port,
                                              uint64_t* ttl_out, NetidxError* err);
/* a subscriber's: ClientHello::ReadOnly(Anonymous) */
NxgResolverClient* nxg_resolver_connect_read(const char* ipv4, uint16_t port, NetidxError* err);
void nxg_resolver_client_close(NxgResolverClient* c);
/* ToWrite::Publish(path), true once FromWrite::Published is back */
bool nxg_resolver_publish(NxgResolverClient* c, const char* path, uint64_t path_len,
                          NetidxError* err);
/* ToRead::Resolve(path): the Resolved reply; its first publisher's address from the
 * FromRead::Publisher that precedes it (n_publishers = 0: nobody publishes the path) */
typedef struct NxgResolved {
    uint32_t n_publishers;
    uint32_t publisher_ipv4; /* host byte order */
    uint64_t publisher_id;
    uint16_t publisher_port, resolver_port;
    uint32_t resolver_ipv4;
    uint64_t timestamp;
    uint32_t flags, permissions;
} NxgResolved;
bool nxg_resolver_resolve(NxgResolverClient* c, const char* path, uint64_t path_len,
                          NxgResolved* out, NetidxError* err);

/* ---- host framing (netidx/src/channel.rs) ------------------------------------------------
 * Frame boundaries exactly as WriteChannel::queue_send/try_flush split the buffer. The split
 * happens at MAX_BATCH = 0x3FFFFFFF (channel.rs:34, 187-191) and is recorded between messages.
 * `msg_len` holds the encoded length of each message, in order. `chunk_len_out` receives the
 * length of each frame payload. Returns the number of frames, or -1 if cap_chunks is too small
 * or a message exceeds MAX_BATCH. */
int64_t nxg_frame_split(const uint64_t* msg_len, uint64_t n_msgs, uint64_t* chunk_len_out,
                        uint64_t cap_chunks);
/* flush_buf (channel.rs:107-126): the u32 big-endian header, with bit 31 set when the frame is
 * encrypted. */
void nxg_frame_header(uint32_t payload_len, bool encrypted, uint8_t out[4]);
/* read_task (channel.rs:379-443): parse one header from `buf`. Returns the header size (4), or
 * 0 if fewer than 4 bytes are present. */
uint32_t nxg_frame_parse_header(const uint8_t* buf, uint64_t avail, uint32_t* payload_len,
                                bool* encrypted);
/* read_task's frame assembly (channel.rs:379-443), incremental: push the bytes read from the
 * socket in any pieces; _next hands out each complete frame payload, in order (the pointer stays
 * valid until the next _push or _free). _next returns 1 with a frame, 0 when the next frame is not
 * complete yet ("reading more"), -1 on an encrypted frame: this layer has no security context
 * ("encryption is not supported", channel.rs:420-422; krb5 is out of scope). */
typedef struct NxgFrameReader NxgFrameReader;
NxgFrameReader* nxg_frame_reader_new(NetidxError* err);
void nxg_frame_reader_free(NxgFrameReader* r);
bool nxg_frame_reader_push(NxgFrameReader* r, const uint8_t* data, uint64_t len, NetidxError* err);
int nxg_frame_reader_next(NxgFrameReader* r, const uint8_t** payload, uint64_t* len,
                          NetidxError* err);
uint64_t nxg_frame_reader_buffered(const NxgFrameReader* r);

#ifdef __cplusplus
}
#endif
#endif
