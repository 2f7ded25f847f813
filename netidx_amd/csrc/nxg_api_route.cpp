// nxg_api_route.cpp -- the routing calls of the C ABI (include/nxg_codec.h): write routing, the
// path table, Subscribe routing, reply routing.
#include "nxg_host.h"
#include "nxg_path_hash.h"

using namespace nxg_host;

extern "C" {

// ---- write routing (publisher/server.rs:171-245, 497-576) ---------------------------------------
// Replaces handle_batch_inner's Write and Unsubscribe arms: nxg_route_writes.hip's passes, the
// dispatch of nxg_dispatch.hip for the channel fan-out, one copy of the head, one synchronisation.
bool nxg_route_writes(NxgCtx* c, const NxgWriteTable* tab, const uint8_t* frame,
                      const NxgColumns* cols, const NxgWriteCols* wcols, uint64_t row_begin,
                      uint64_t ctl_begin, uint64_t fresh_wid, NxgWriteRoute* out, NetidxError* err) {
    // (the argument checks come before any use of the context)
    if (!c || !tab || !cols || !out) return refuse(err, "null argument");
    if (!wcols)
        return refuse(err, "wcols is null: the rows' wflags / wid come from nxg_decode_writes");
    if (cols->mem != NXG_MEM_DEVICE || wcols->mem != NXG_MEM_DEVICE)
        return refuse(err, "cols->mem / wcols->mem: write routing takes device columns");
    if (cols->layout != NXG_LAYOUT_MIXED || !mixed_capable(cols) || !cols->id)
        return refuse(err, "cols->layout: write batches are MIXED-layout columns");
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
    if (rows >= 0xffffffffull) return refuse(err, "row_begin: a call covers fewer than 2^32 rows");
    if (n_rows && (!wcols->wflags || !wcols->wid || wcols->cap_rows < n_rows)) {
        set_err(err, "wcols holds %llu rows, the batch %llu", (unsigned long long)wcols->cap_rows,
                (unsigned long long)n_rows);
        return false;
    }
    if (spans && !frame)
        return refuse(err, "frame is null: the Unsubscribe spans' Ids are read from it");
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
        (out->cap_unsub && !out->unsub_id) || (out->cap_reply && !out->reply))
        return refuse(err, "out: null output array");
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
    if (!c || !t) return refuse(err, "null argument");
    if (t->device != c->device) {
        set_err(err, "the path table belongs to device %d, the ctx to %d", t->device, c->device);
        return false;
    }
    return no_pending(c, err);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

// Subscribe and reply routing: every listed pointer is device memory; one that is null may be so
// only where `need` is false. The first offender is named.
struct NamedPtr {
    const void* p;
    bool need;
    const char* name;
};
bool named_device(std::initializer_list<NamedPtr> ptrs, NetidxError* err) {
    for (const NamedPtr& q : ptrs) {
        if ((q.p || q.need) && !is_device_ptr(q.p)) {
            set_err(err, "%s: %s", q.name, q.p ? "not device memory" : "null");
            return false;
        }
    }
    return true;
}

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
    if (!off || !id) return refuse(err, "off / id is null");
    if (!pt_offsets_ok(off, n, err)) return false;
    const uint64_t total = off[n] - off[0];
    if (total && !paths) return refuse(err, "paths is null");
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
    if (!off) return refuse(err, "off is null");
    if (!pt_offsets_ok(off, n, err)) return false;
    const uint64_t total = off[n] - off[0];
    if (total && !paths) return refuse(err, "paths is null");
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
    if (!is_device_ptr(doff) || !is_device_ptr(dlen) || !is_device_ptr(did_out))
        return refuse(err, "doff / dlen / did_out: a path lookup takes device arrays");
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
    if (!c || !cols || !out) return refuse(err, "null argument");
    if (!tab || !tab->paths || !tab->pub)
        return refuse(err, "tab: the table, tab->paths or tab->pub is null");
    if (cols->mem != NXG_MEM_DEVICE)
        return refuse(err, "cols->mem: subscribe routing takes device columns");
    if (cols->layout != NXG_LAYOUT_MIXED || !mixed_capable(cols))
        return refuse(err, "cols->layout: To frames are decoded into MIXED-layout columns");
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
    if (spans >= 0xffffffffull)
        return refuse(err, "ctl_begin: a call covers fewer than 2^32 spans");
    const NxgPubTable* pub = tab->pub;
    if (out->cap_spans < n_ctl || (n_ctl && (!out->outcome || !out->span_id))) {
        set_err(err, "out->cap_spans: outcome[] / span_id[] hold %llu spans, the batch %llu",
                (unsigned long long)out->cap_spans, (unsigned long long)n_ctl);
        return false;
    }
    if ((out->cap_sub && (!out->sub_id || !out->sub_perm)) || (out->cap_deferred && !out->deferred) ||
        (out->cap_reply && !out->reply))
        return refuse(err, "out: null output array");
    if ((pub->n_ids && !pub->slot_of_id) || (pub->n_slots && !pub->cur_fixed) ||
        (tab->n_defaults && (!tab->default_off || !tab->default_heap)))
        return refuse(err, "tab: null table array");
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
    if (!named_device({
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
        }, err))
        return false;
    if (pub->cur_ctag && (!pub->cur_cfixed || !pub->cur_caux))
        return refuse(err, "tab->pub: cur_ctag without cur_cfixed / cur_caux");
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
    if (!c || !cols || !out) return refuse(err, "null argument");
    if (!tab || !tab->subs || !tab->pending)
        return refuse(err, "tab: the table, tab->subs or tab->pending is null");
    if (cols->mem != NXG_MEM_DEVICE)
        return refuse(err, "cols->mem: reply routing takes device columns");
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
    if (rows + spans >= 0xffffffffull)
        return refuse(err, "row_begin / ctl_begin: a call covers fewer than 2^32 rows and spans");
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
    if (!named_device({
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
        }, err))
        return false;
    if (st->n_slots && st->n_chans && !st->stream_chan) {
        // (a table whose every stream list is empty may leave it null: no entry is ever read)
        uint32_t last = 0;
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpy(&last, st->slot_stream_off + st->n_slots, 4, hipMemcpyDeviceToHost));
        if (last) return refuse(err, "tab->subs->stream_chan: null");
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

}  // extern "C"
