// nxg_api_oneshot.cpp -- the oneshot calls of the C ABI (include/nxg_codec.h): the pathmap section
// of a reply shard and its filter set, and the framing of a shard and of the reply
// (netidx-archive/src/recorder/oneshot.rs:100-157, recorder_client.rs:29-37).
#include "nxg_host.h"
#include "nxg_oneshot.h"

using namespace nxg_host;

namespace {

uint32_t varint_len(uint64_t v) {  // pack.rs:472-474
    uint32_t n = 1;
    for (; v >= 0x80; v >>= 7) n++;
    return n;
}

uint32_t put_varint(uint8_t* o, uint64_t v) {  // pack.rs:476-486
    uint32_t n = 0;
    for (; v >= 0x80; v >>= 7) o[n++] = (uint8_t)((v & 0x7f) | 0x80);
    o[n++] = (uint8_t)v;
    return n;
}

uint64_t len_wrapped_len(uint64_t n) { return n + varint_len(n + varint_len(n)); }  // pack.rs:522-525

// Vec / VecDeque::encode's guard with an element of 64 bytes (the element sizes involve
// GPooled<..> and cannot be pinned)
constexpr uint64_t kOsMaxElems = kMaxVecBytes / 64;

bool shard_layout(uint64_t pathmap_len, uint64_t image_len, uint64_t deltas_len, uint64_t n_deltas,
                  NxgOneshotShardLayout* o, NetidxError* err) {
    if (n_deltas > kOsMaxElems) {
        set_err(err, "encode failed: %llu delta records exceed MAX_VEC (PackError::TooBig)",
                (unsigned long long)n_deltas);
        return false;
    }
    if ((pathmap_len | image_len | deltas_len) >> 60)
        return refuse(err, "a section of 2^60 bytes or more");
    memset(o, 0, sizeof *o);
    o->pathmap_len = pathmap_len, o->image_len = image_len;
    o->deltas_len = deltas_len, o->n_deltas = n_deltas;
    o->count_head_len = put_varint(o->count_head, n_deltas);
    const uint64_t inner = pathmap_len + image_len + o->count_head_len + deltas_len;
    o->len_head_len = put_varint(o->len_head, len_wrapped_len(inner));
    o->pathmap_off = o->len_head_len;
    o->image_off = o->pathmap_off + pathmap_len;
    o->count_off = o->image_off + image_len;
    o->deltas_off = o->count_off + o->count_head_len;
    o->shard_len = o->deltas_off + deltas_len;
    return true;
}

}  // namespace

extern "C" {

// ---- the pathmap section and the filter set (nxg_oneshot.hip). Argument checks on the host, the
// launches, one read-back of the call's head.
bool nxg_oneshot_pack_pathmap(NxgCtx* c, const NxgOneshotPaths* paths, const uint8_t* keep,
                              NxgOneshotPathmap* out, NetidxError* err) {
    // (every argument is looked at before the ctx, so that each refusal is reached without one)
    if (!paths) return refuse(err, "null argument (paths)");
    if (!out) return refuse(err, "null argument (out)");
    const uint64_t n = paths->n_ids;
    if (n && !paths->path_off) return refuse(err, "null argument (paths->path_off)");
    if (n && !paths->path_bytes) return refuse(err, "null argument (paths->path_bytes)");
    if (n && !keep) return refuse(err, "null argument (keep)");
    if (n && !out->sel) return refuse(err, "null argument (out->sel)");
    if (n > (1ull << 32)) {
        set_err(err, "too many Ids for one path index (%llu): an archive Id has 32 bits",
                (unsigned long long)n);
        return false;
    }
    if (!c) return refuse(err, "null argument (ctx)");
    if (!all_device({n ? paths->path_off : nullptr, n ? paths->path_bytes : nullptr,
                     n ? keep : nullptr, n ? out->sel : nullptr, out->out})) {
        set_err(err, "nxg_oneshot_pack_pathmap takes device memory only (paths->path_off, "
                     "paths->path_bytes, keep, out->sel and out->out)");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    out->n_bytes = out->n_sel = 0;
    if (n == 0) {  // an empty map is its count, and no kernel runs
        out->n_bytes = 1;
        if (!out->out) return true;
        if (out->cap_bytes < 1) {
            set_err(err, "output buffer too small: need 1 bytes, have 0");
            return false;
        }
        HIPCHK(hipMemsetAsync(out->out, 0, 1, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgOsPmArgs a{};
    a.path_off = paths->path_off;
    a.path_bytes = paths->path_bytes;
    a.keep = keep;
    a.n_ids = n;
    a.sel = out->sel;
    a.out = out->out;
    a.cap = out->out ? out->cap_bytes : 0;
    if (!ensure_dscratch(c, nxg_os_pm_scratch_bytes(n), err)) return false;
    NxgOsPmHead h;
    HIPCHK(nxg_launch_os_pathmap(a, c->dscratch, c->stream));
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.bad_inv) {
        const uint64_t id = ~h.bad_inv;
        set_err(err, "paths->path_off decreases at Id %llu: path_off[%llu] lies in front of "
                     "path_off[%llu]", (unsigned long long)id, (unsigned long long)(id + 1),
                (unsigned long long)id);
        return false;
    }
    out->n_bytes = h.n_bytes;
    out->n_sel = h.n_sel;
    if (h.vec_bad) {
        set_err(err, "encode failed: %llu selected paths exceed MAX_VEC (PackError::TooBig)",
                (unsigned long long)h.n_sel);
        return false;
    }
    if (out->out && h.n_bytes > out->cap_bytes) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)h.n_bytes, (unsigned long long)out->cap_bytes);
        return false;
    }
    return true;
}

// ---- batch.retain, the empty-record drop and the deltas elements of one window (oneshot.rs:
// 146-149; nxg_oneshot.hip). Argument checks on the host, one copy up of the records' rows and
// timestamps, the launches, one read-back of the call's head.
bool nxg_oneshot_pack_deltas(NxgCtx* c, const NxgColumns* window, const uint8_t* dbuf,
                             const NxgArchiveBatchInfo* info, uint32_t n_recs,
                             const int64_t* ts_secs, const uint32_t* ts_nanos, const uint8_t* sel,
                             uint64_t n_ids, NxgOneshotDeltas* out, NetidxError* err) {
    // (every argument is looked at before the ctx, so that each refusal is reached without one)
    if (!window) return refuse(err, "null argument (window)");
    if (n_recs && !info) return refuse(err, "null argument (info)");
    if (n_recs && !ts_secs) return refuse(err, "null argument (ts_secs)");
    if (n_recs && !ts_nanos) return refuse(err, "null argument (ts_nanos)");
    if (n_ids && !sel) return refuse(err, "null argument (sel)");
    if (!out) return refuse(err, "null argument (out)");
    if (!out->rec_off) return refuse(err, "null argument (out->rec_off)");
    if (n_recs && !out->rec_items) return refuse(err, "null argument (out->rec_items)");
    if (window->mem != NXG_MEM_DEVICE || window->layout != NXG_LAYOUT_MIXED ||
        (window->n_rows && (!window->id || !window->tag || !window->fixed || !window->aux)))
        return refuse(err, "a window is packed from device MIXED-layout columns");
    if (n_ids > (1ull << 32)) {
        set_err(err, "too many Ids (%llu): an archive Id has 32 bits", (unsigned long long)n_ids);
        return false;
    }
    std::vector<uint64_t> hbeg, hend;
    if (!window_records(window, info, n_recs, &hbeg, &hend, err)) return false;
    const uint64_t first = hbeg[0], n = hbeg[n_recs] - first;
    if (n >= (1ull << 39)) {
        set_err(err, "too many rows for one call (%llu)", (unsigned long long)n);
        return false;
    }
    if (!c) return refuse(err, "null argument (ctx)");
    const bool kids = window->n_children && window->ctag && window->cfixed && window->caux;
    if (!all_device({out->rec_off, n_recs ? out->rec_items : nullptr, out->out, dbuf,
                     n_ids ? sel : nullptr, n ? window->id : nullptr, n ? window->tag : nullptr,
                     n ? window->fixed : nullptr, n ? window->aux : nullptr,
                     kids ? window->ctag : nullptr, kids ? window->cfixed : nullptr,
                     kids ? window->caux : nullptr})) {
        set_err(err, "nxg_oneshot_pack_deltas takes device memory only (window, dbuf, sel, "
                     "out->out, out->rec_off and out->rec_items)");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    out->n_bytes = out->n_items = out->n_dropped = out->n_kept_recs = 0;
    if (n == 0) {  // no rows: no element, and no kernel runs
        HIPCHK(hipMemsetAsync(out->rec_off, 0, ((uint64_t)n_recs + 1) * 8, c->stream));
        if (n_recs) HIPCHK(hipMemsetAsync(out->rec_items, 0, (uint64_t)n_recs * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgOsDlArgs a{};
    a.cols = desc_of(window);
    a.cols.n_ctl = 0;
    if (!kids) {
        a.cols.ctag = nullptr, a.cols.cfixed = nullptr, a.cols.caux = nullptr;
        a.cols.n_children = 0;
    }
    a.heap = dbuf;
    a.sel = sel;
    a.n_ids = n_ids;
    a.first = first;
    a.n = n;
    a.n_recs = n_recs;
    a.out = out->out;
    a.cap = out->out ? out->cap_bytes : 0;
    a.rec_off = out->rec_off;
    a.rec_items = out->rec_items;
    // rbeg[n_recs + 1] and rend[n_recs] relative to `first`, the seconds, the nanoseconds
    std::vector<uint64_t> up(4 * (size_t)n_recs + 1);
    uint64_t rows = 0;
    for (uint32_t i = 0; i < n_recs; i++) {
        up[i] = hbeg[i] - first;
        up[(size_t)n_recs + 1 + i] = hend[i] - first;
        up[2 * (size_t)n_recs + 1 + i] = (uint64_t)ts_secs[i];
        up[3 * (size_t)n_recs + 1 + i] = ts_nanos[i];
        rows += hend[i] - hbeg[i];
    }
    up[n_recs] = n;
    if (!ensure_dscratch(c, nxg_os_dl_scratch_bytes(n, n_recs), err)) return false;
    NxgOsDlHead h;
    HIPCHK(nxg_launch_os_deltas(a, c->dscratch, up.data(), c->stream));
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.err_inv) {
        const uint64_t row = ~(h.err_inv >> 8 | 0xffull << 56);
        set_err(err, "window row %llu: %s", (unsigned long long)row,
                rec_cause((uint32_t)(h.err_inv & 0xff)));
        return false;
    }
    if (h.vec_bad) {
        set_err(err, "encode failed: record %u's items exceed MAX_VEC (PackError::TooBig)",
                h.vec_bad - 1);
        return false;
    }
    out->n_bytes = h.n_bytes;
    out->n_items = h.n_items;
    out->n_dropped = rows - h.n_items;
    out->n_kept_recs = h.n_kept_recs;
    if (out->out && h.n_bytes > out->cap_bytes) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)h.n_bytes, (unsigned long long)out->cap_bytes);
        return false;
    }
    return true;
}

// ---- the framing: #[derive(Pack)] OneshotReplyShard and OneshotReply (recorder_client.rs:29-37),
// both length-wrapped (netidx-derive/src/lib.rs:113,137; len_wrapped_len, pack.rs:522-525). Host
// arithmetic; the assembly is copies on the ctx's stream.
bool nxg_oneshot_shard_layout(uint64_t pathmap_len, uint64_t image_len, uint64_t deltas_len,
                              uint64_t n_deltas, NxgOneshotShardLayout* out, NetidxError* err) {
    if (!out) return refuse(err, "null argument (out)");
    return shard_layout(pathmap_len, image_len, deltas_len, n_deltas, out, err);
}

bool nxg_oneshot_reply_head(const uint64_t* shard_len, uint64_t n_shards, uint8_t* head,
                            uint32_t* head_len, uint64_t* reply_len, NetidxError* err) {
    if (n_shards && !shard_len) return refuse(err, "null argument (shard_len)");
    if (!head) return refuse(err, "null argument (head)");
    if (!head_len) return refuse(err, "null argument (head_len)");
    if (n_shards > kOsMaxElems) {
        set_err(err, "encode failed: %llu shards exceed MAX_VEC (PackError::TooBig)",
                (unsigned long long)n_shards);
        return false;
    }
    uint64_t inner = varint_len(n_shards);
    for (uint64_t i = 0; i < n_shards; i++) {
        if (shard_len[i] >> 60 || (inner += shard_len[i]) >> 60)
            return refuse(err, "shards of 2^60 bytes or more");
    }
    uint32_t n = put_varint(head, len_wrapped_len(inner));
    const uint32_t wrap = n;
    n += put_varint(head + n, n_shards);
    *head_len = n;
    if (reply_len) *reply_len = wrap + inner;
    return true;
}

bool nxg_oneshot_assemble_shard(NxgCtx* c, const NxgOneshotShardLayout* layout,
                                const uint8_t* pathmap, const uint8_t* image,
                                const NxgOneshotFrag* frags, uint32_t n_frags, uint8_t* out,
                                uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!layout) return refuse(err, "null argument (layout)");
    if (layout->pathmap_len && !pathmap) return refuse(err, "null argument (pathmap)");
    if (layout->image_len && !image) return refuse(err, "null argument (image)");
    if (n_frags && !frags) return refuse(err, "null argument (frags)");
    if (!out) return refuse(err, "null argument (out)");
    NxgOneshotShardLayout want;
    if (!shard_layout(layout->pathmap_len, layout->image_len, layout->deltas_len, layout->n_deltas,
                      &want, err))
        return false;
    if (memcmp(&want, layout, sizeof want) != 0)
        return refuse(err, "layout is not what nxg_oneshot_shard_layout made of its four inputs");
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_frags; i++) {
        if (frags[i].len && !frags[i].ptr) {
            set_err(err, "null argument (frags[%u].ptr)", i);
            return false;
        }
        if (frags[i].len > layout->deltas_len - sum) {
            sum = ~0ull;
            break;
        }
        sum += frags[i].len;
    }
    if (sum != layout->deltas_len) {
        set_err(err, "the fragments' lengths do not sum to the layout's deltas_len (%llu)",
                (unsigned long long)layout->deltas_len);
        return false;
    }
    if (layout->shard_len > cap) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)layout->shard_len, (unsigned long long)cap);
        return false;
    }
    if (!c) return refuse(err, "null argument (ctx)");
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    bool dev = is_device_ptr(out) && (!layout->pathmap_len || is_device_ptr(pathmap)) &&
               (!layout->image_len || is_device_ptr(image));
    for (uint32_t i = 0; dev && i < n_frags; i++) dev = !frags[i].len || is_device_ptr(frags[i].ptr);
    if (!dev) {
        set_err(err, "nxg_oneshot_assemble_shard takes device memory only (pathmap, image, every "
                     "fragment and out)");
        return false;
    }
    // the two heads from pinned staging (the call ends with a synchronize: the staging is free again)
    if (!grow(c, c->os_host, 32, kGrowDouble, err)) return false;
    uint8_t* hp = c->os_host.get();
    memcpy(hp, layout->len_head, layout->len_head_len);
    memcpy(hp + 16, layout->count_head, layout->count_head_len);
    HIPCHK(hipMemcpyAsync(out, hp, layout->len_head_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(out + layout->count_off, hp + 16, layout->count_head_len,
                          hipMemcpyHostToDevice, c->stream));
    if (layout->pathmap_len)
        HIPCHK(hipMemcpyAsync(out + layout->pathmap_off, pathmap, layout->pathmap_len,
                              hipMemcpyDeviceToDevice, c->stream));
    if (layout->image_len)
        HIPCHK(hipMemcpyAsync(out + layout->image_off, image, layout->image_len,
                              hipMemcpyDeviceToDevice, c->stream));
    uint64_t at = layout->deltas_off;
    for (uint32_t i = 0; i < n_frags; i++) {
        if (!frags[i].len) continue;
        HIPCHK(hipMemcpyAsync(out + at, frags[i].ptr, frags[i].len, hipMemcpyDeviceToDevice,
                              c->stream));
        at += frags[i].len;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (len_out) *len_out = layout->shard_len;
    return true;
}

}  // extern "C"
