// nxg_ctx.cpp -- contexts and what every entry point of the C ABI (include/nxg_codec.h) leans on:
// the error convention, the status ring, buffer growth, column allocation, host staging of
// host-resident frames and columns; the debug entries; host framing.
#include <cstdarg>
#include <cstdio>

#include "nxg_host.h"

using namespace nxg_host;

thread_local uint32_t nxg_patience = 128;  // the calling ctx's, set by begin_call
thread_local DevStatus* nxg_zero_slot = nullptr;
thread_local bool nxg_zero_used = false;

namespace nxg_host {

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

bool refuse(NetidxError* err, const char* msg) {
    set_err(err, "%s", msg);
    return false;
}

bool launch_ok(hipError_t e, const char* what, NetidxError* err) {
    if (e != hipSuccess) set_err(err, "%s: %s", what, hipGetErrorString(e));
    return e == hipSuccess;
}

bool set_device(NxgCtx* c, NetidxError* err) {
    HIPCHK(hipSetDevice(c->device));
    return true;
}

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

bool end_call(NxgCtx* c, NetidxError* err) {
    if (nxg_zero_used) return true;
    nxg_zero_used = true;
    HIPCHK(hipMemsetAsync(nxg_zero_slot, 0, sizeof(DevStatus), c->stream));
    return true;
}

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

void gather_forget(NxgCtx* c) {
    c->gathered_to = c->pending.empty() ? c->calls : c->pending.front().seq;
}

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

bool all_device(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (p && !is_device_ptr(p)) return false;
    return true;
}

ColsDesc desc_of(const NxgColumns* c, const NxgWriteCols* w) {
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

// the column arrays of nr rows, nc children and nk control spans, `s` to `d` (mixed: all of them)
static bool copy_cols(NxgCtx* c, const NxgColumns* s, NxgColumns* d, uint64_t nr, uint64_t nc,
                      uint64_t nk, bool mixed, hipMemcpyKind dir, NetidxError* err) {
    HIPCHK(hipMemcpyAsync(d->id, s->id, nr * 8, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->fixed, s->fixed, nr * 8, dir, c->stream));
    if (!mixed) return true;
    HIPCHK(hipMemcpyAsync(d->tag, s->tag, nr, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->aux, s->aux, nr * 4, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->ctag, s->ctag, nc, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->cfixed, s->cfixed, nc * 8, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->caux, s->caux, nc * 4, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->ctl_row, s->ctl_row, nk * 8, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->ctl_off, s->ctl_off, nk * 8, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->ctl_len, s->ctl_len, nk * 4, dir, c->stream));
    HIPCHK(hipMemcpyAsync(d->ctl_variant, s->ctl_variant, nk, dir, c->stream));
    return true;
}

bool copy_cols_d2h(NxgCtx* c, const NxgColumns* d, NxgColumns* h, NetidxError* err) {
    if (!copy_cols(c, d, h, std::min(d->n_rows, h->cap_rows),
                   std::min(d->n_children, h->cap_children), std::min(d->n_ctl, h->cap_ctl),
                   mixed_capable(h) && d->tag, hipMemcpyDeviceToHost, err))
        return false;
    HIPCHK(hipStreamSynchronize(c->stream));
    return true;
}

bool copy_cols_h2d(NxgCtx* c, const NxgColumns* h, NxgColumns* d, NetidxError* err) {
    if (!copy_cols(c, h, d, h->n_rows, h->n_children, h->n_ctl, h->layout == NXG_LAYOUT_MIXED,
                   hipMemcpyHostToDevice, err))
        return false;
    d->n_rows = h->n_rows;
    d->n_children = h->n_children;
    d->n_ctl = h->n_ctl;
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

}  // namespace nxg_host

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
    if (policy >= sizeof rows / sizeof rows[0]) return refuse(err, "policy: no such row");
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
    if ((e = hipStreamCreateWithFlags(&c->own.s, hipStreamNonBlocking)) != hipSuccess)
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

NxgCtx::~NxgCtx() {
    (void)hipSetDevice(device);
    if (dcols_valid) cols_free_impl(&dcols);
    for (void* p : {(void*)gruns, zdefs, (void*)zlit, zc_tables, (void*)zc_slab, (void*)dst})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : zc_ev)
        if (e) (void)hipEventDestroy(e);
    if (hst) (void)hipHostFree(hst);
}

void nxg_ctx_destroy(NxgCtx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

bool nxg_ctx_set_stream(NxgCtx* c, void* s, NetidxError* err) {
    if (!c) return refuse(err, "null ctx");
    if (!set_device(c, err)) return false;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own.s;
    return true;
}

void* nxg_ctx_stream(NxgCtx* c) { return c ? (void*)c->stream : nullptr; }

bool nxg_columns_alloc(NxgCtx* c, uint32_t layout, uint64_t cap_rows, uint64_t cap_children,
                       uint64_t cap_ctl, uint32_t mem, NxgColumns* out, NetidxError* err) {
    if (!c || !out) return refuse(err, "null argument");
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
    if (!r || (len && !data)) return refuse(err, "null argument");
    // drop what was handed out before growing (payload pointers from _next end here)
    if (r->head) {
        r->buf.erase(r->buf.begin(), r->buf.begin() + (ptrdiff_t)r->head);
        r->head = 0;
    }
    try {
        r->buf.insert(r->buf.end(), data, data + len);
    } catch (...) {
        return refuse(err, "out of memory");
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
