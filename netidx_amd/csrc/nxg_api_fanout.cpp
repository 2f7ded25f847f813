// nxg_api_fanout.cpp -- the fan-out calls of the C ABI (include/nxg_codec.h): the type-partitioned
// view, dispatch, publisher commit and unsubscribes, per-client frames, the value table.
#include "nxg_host.h"

using namespace nxg_host;

namespace {

// The tail of the three dispatch calls: the fan-out of nxg_dispatch.hip over `n` rows into `out`
// (`ds`: 64 bytes for the unmatched counter, then nxg_disp_scratch_bytes), the total and (where
// rows can go unmatched) the unmatched count read back in one wait, the capacity check. `needs`
// opens the capacity message ("dispatch needs", "unsubscribes need").
bool dispatch_tail(NxgCtx* c, const NxgSubTable& tab, const uint64_t* id, uint64_t n, uint8_t* ds,
                   NxgDispatch* out, uint64_t* last_row, const uint8_t* mode,
                   const uint32_t* to_client, bool unmatched, const char* needs,
                   NetidxError* err) {
    uint64_t* um = reinterpret_cast<uint64_t*>(ds);
    HIPCHK(nxg_launch_dispatch(tab, id, n, ds + 64, out->chan_off, out->ent_sub, out->ent_row,
                               out->cap_entries, last_row, um, c->ncu, c->stream, mode,
                               to_client));
    uint64_t res[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&res[0], out->chan_off + tab.n_chans, 8, hipMemcpyDeviceToHost,
                          c->stream));
    if (unmatched) HIPCHK(hipMemcpyAsync(&res[1], um, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_entries = res[0];
    out->n_unmatched = res[1];
    if (res[0] > out->cap_entries) {
        set_err(err, "%s %llu entries, capacity is %llu", needs, (unsigned long long)res[0],
                (unsigned long long)out->cap_entries);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

// ---- type-partitioned view ------------------------------------------------------
bool nxg_partition_by_tag(NxgCtx* c, const NxgColumns* cols, NxgTagView* out, NetidxError* err) {
    if (!c || !cols || !out) return refuse(err, "null argument");
    const uint64_t n = cols->n_rows;
    if (cols->layout != NXG_LAYOUT_MIXED || !cols->tag || !cols->fixed || !cols->aux)
        return refuse(err, "the type-partitioned view needs mixed-layout columns (a tag column)");
    if (n && (!out->rank || !out->row_of || !out->fixed || !out->aux))
        return refuse(err, "null output array");
    if (n > out->cap_rows || n > 0xffffffffull) {
        set_err(err, "%llu rows: the view's capacity is %llu (and rows must be < 2^32)",
                (unsigned long long)n, (unsigned long long)out->cap_rows);
        return false;
    }
    if (n && (!is_device_ptr(cols->tag) || !is_device_ptr(out->rank)))
        return refuse(err, "the type-partitioned view needs device columns and device outputs");
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
    if (!c || !tab || !out || (n_rows && !id) || !out->chan_off)
        return refuse(err, "null argument");
    if ((tab->n_ids && !tab->slot_of_id) ||
        (tab->n_slots && (!tab->slot_sub_id || !tab->slot_stream_off || !tab->slot_has_last ||
                          !out->last_row)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row)))
        return refuse(err, "null table or output array");
    if (n_rows && tab->n_slots && !tab->stream_chan && tab->n_chans)
        return refuse(err, "null stream_chan");
    HIPCHK(hipSetDevice(c->device));
    const size_t need = 64 + nxg_disp_scratch_bytes(n_rows, tab->n_chans);
    if (!ensure_dscratch(c, need, err)) return false;
    return dispatch_tail(c, *tab, id, n_rows, c->dscratch, out, out->last_row, nullptr, nullptr,
                         true, "dispatch needs", err);
}

// ---- publisher commit (publisher/mod.rs:776-845) -----------------------------------------------
bool nxg_publish_commit(NxgCtx* c, const NxgPubTable* tab, const NxgColumns* batch,
                        const uint8_t* heap, const uint8_t* kind, const uint32_t* to_client,
                        NxgDispatch* out, NetidxError* err) {
    if (!c || !tab || !batch || !out || !out->chan_off) return refuse(err, "null argument");
    const uint64_t n = batch->n_rows;
    if (n && (!batch->id || !batch->fixed || !kind || !to_client))
        return refuse(err, "null batch column, kind or to_client");
    if ((tab->n_ids && !tab->slot_of_id) ||
        (tab->n_slots && (!tab->slot_client_off || !tab->cur_fixed || !out->last_row)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row)))
        return refuse(err, "null table or output array");
    if (n >= 0xffffffffull) return refuse(err, "publish batches are limited to 2^32 - 1 rows");
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
    return dispatch_tail(c, st, batch->id, n, c->dscratch + pub, out, out->last_row, mode, to_client,
                         true, "publish needs", err);
}

// the commit's unsubscribes (publisher/mod.rs:820-832): every pair routes to its client (row
// mode 2 of the dispatch), so each client's list keeps queue order
bool nxg_publish_unsubscribes(NxgCtx* c, const uint64_t* id, const uint32_t* client, uint64_t n,
                              uint32_t n_clients, NxgDispatch* out, NetidxError* err) {
    if (!c || !out || !out->chan_off || (n && (!id || !client)) ||
        (out->cap_entries && (!out->ent_sub || !out->ent_row)))
        return refuse(err, "null argument");
    if (n >= 0xffffffffull) return refuse(err, "unsubscribe lists are limited to 2^32 - 1 pairs");
    HIPCHK(hipSetDevice(c->device));
    const size_t mode_bytes = (n + 255) & ~uint64_t(255);
    const size_t need = mode_bytes + 64 + nxg_disp_scratch_bytes(n, n_clients);
    if (!ensure_dscratch(c, need, err)) return false;
    uint8_t* mode = c->dscratch;
    if (n) HIPCHK(hipMemsetAsync(mode, 2, n, c->stream));
    const NxgSubTable st{0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, n_clients};
    return dispatch_tail(c, st, id, n, c->dscratch + mode_bytes, out, nullptr, mode, client, false,
                         "unsubscribes need", err);
}

// ---- the commit's per-client batches, encoded (handle_updates -> queue_send per client) -------
// One gathered encode of the entry list (nxg_encode_clients.hip). pass(dout, cap) runs the tile
// kernel and reads the status and client_off back; a buffer that could take more than MAX_BATCH
// bytes is sized first, so that a client too long for one frame fails before anything is written.
bool nxg_encode_clients(NxgCtx* c, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_clients, NxgClientFrames* out,
                        NetidxError* err) {
    if (!c || !batch || !d || !out || !out->client_off || !d->chan_off)
        return refuse(err, "null argument");
    const uint64_t ne = d->n_entries;
    const bool f64 = batch->layout == NXG_LAYOUT_F64;
    if (batch->n_ctl) {
        set_err(err, "per-client batches encode from columns without control messages (n_ctl = "
                     "%llu)", (unsigned long long)batch->n_ctl);
        return false;
    }
    if (ne && (!d->ent_row || !batch->id || !batch->fixed ||
               (!f64 && (!batch->tag || !batch->aux))))
        return refuse(err, "null entry array or batch column");
    // (the arrays that must be there were found non-null above)
    if (batch->mem != NXG_MEM_DEVICE ||
        !all_device({d->chan_off, out->client_off, out->out, ne ? d->ent_row : nullptr,
                     ne ? batch->id : nullptr, heap})) {
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
        if (!with_call(c, &st, &slot, err, [&](DevStatus* s) {
                const hipError_t le = nxg_launch_enc_clients(f64, cd, heap, g, dout, cap, c->tstat,
                                                             c->epoch, s, c->grid_enc_f64,
                                                             c->grid_enc_gen, c->stream);
                HIPCHK(le);
                return true;
            }))
            return false;
        DevStatus h;
        if (!fetch_status(c, st, slot, &h, err, [&] {
                HIPCHK(hipMemcpyAsync(off.data(), out->client_off, cnt * 8, hipMemcpyDeviceToHost,
                                      c->stream));
                return true;
            }))
            return false;
        if (!h.timeout && h.err_key) {  // (the watchdog first: encode_status_ok below)
            set_err(err, "entry %llu names a row at or past the batch's %llu rows",
                    (unsigned long long)~h.err_key, (unsigned long long)batch->n_rows);
            return false;
        }
        if (!encode_status_ok(h, err)) return false;
        bool sorted = !(h.irregular & 1u) && off[n_clients] == h.total_bytes;
        for (uint64_t i = 0; sorted && i < n_clients; i++) sorted = off[i] <= off[i + 1];
        if (!sorted) {
            set_err(err, "d->chan_off is not a dispatch's: it must not decrease and must end at "
                         "d->n_entries (%llu)", (unsigned long long)ne);
            return false;
        }
        total = h.total_bytes;
        out->n_bytes = total;
        return !dout || encode_fits(h.capacity, total, cap, err);
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
        if (!encode_fits(false, total, out->cap_bytes, err)) return false;
    }
    return pass(out->out, out->cap_bytes) && frames_ok();
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
    if (!all_device({t->tag, t->fixed, t->aux, mixed ? t->heap : nullptr, mixed ? t->ctag : nullptr,
                     mixed ? t->cfixed : nullptr, mixed ? t->caux : nullptr})) {
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
        if (b->mem != NXG_MEM_DEVICE)
            return refuse(err, "batch->mem: the value table takes device columns");
        if (b->n_rows && (!b->fixed || (!f64 && (!b->tag || !b->aux))))
            return refuse(err, "batch: null column");
        if (!f64 && b->n_children && (!b->ctag || !b->cfixed || !b->caux))
            return refuse(err, "batch: n_children without child columns");
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
    if (!all_device({s.tag, s.fixed, s.aux, s.ctag, s.cfixed, s.caux, s.heap, src_row}))
        return refuse(err, "batch, heap or src_row: not device memory");
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
    if (!c || !t) return refuse(err, "null argument");
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
    if (!c || !t || !batch || !out || (t->n_slots && !src_row)) return refuse(err, "null argument");
    *out = NxgValueApply{};
    if (!vt_table_ok(t, "t", err)) return false;
    NxgVtArgs a{};
    std::vector<Span> tb, in;
    if (!vt_batch(batch, heap, heap_len, src_row, t->n_slots, &a.batch, &in, err)) return false;
    vt_spans(t, &tb);
    if (overlaps(tb, in))
        return refuse(err, "the batch, its heap or src_row overlaps the table's arrays");
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
    if (!c || !src || !dst || !out) return refuse(err, "null argument");
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
    if (overlaps(db, in)) return refuse(err, "dst overlaps src, the batch, its heap or src_row");
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
    if (!c || !t || (n && !slot)) return refuse(err, "null argument");
    if (!vt_table_ok(t, "t", err)) return false;
    if (!t->tag)
        return refuse(err, "t: a table without a tag column cannot hold Event::Unsubscribed");
    if (n >= 0xffffffffull || (n && !is_device_ptr(slot)))
        return refuse(err, "slot: device memory, fewer than 2^32 - 1 entries");
    std::vector<Span> tb;
    vt_spans(t, &tb);
    if (n && overlaps(tb, {span_of(slot, n * 4)}))
        return refuse(err, "slot overlaps the table's arrays");
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

}  // extern "C"
