// nxg_api.cpp -- the update calls of the C ABI (include/nxg_codec.h): decode and encode of
// publisher::From batches, the async backlog and nxg_ctx_sync, frames, and publisher::To batches.
#include <cstdio>
#include <string>

#include "nxg_host.h"

using namespace nxg_host;

namespace {

constexpr uint32_t kIrregularCalls = 64;
constexpr uint32_t kMixFailCalls = 16;
constexpr uint32_t kSeqSkipCalls = 64;

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

}  // namespace

namespace nxg_host {

bool enqueue_dec_fast(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, DevStatus* st,
                      int* path, NetidxError* err, bool try_seq) {
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

}  // namespace nxg_host

namespace {

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

// a frame's first attempt: the f64 decoders, or with NXG_DECODE_HINT_MIXED the mixed ones
bool enqueue_dec_first(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, uint32_t flags,
                       DevStatus* st, int* path, NetidxError* err) {
    return !(flags & NXG_DECODE_HINT_MIXED) ? enqueue_dec_fast(c, f, len, out, st, path, err)
                                            : enqueue_dec_mixed(c, f, len, out, st, path, err);
}

}  // namespace

namespace nxg_host {

bool finish_decode(NxgCtx* c, const uint8_t* f, uint64_t len, NxgColumns* out, int tried_fast,
                   DevStatus* st, uint32_t slot, NxgStatus* ust, NetidxError* err,
                   bool fetched, bool* redone) {
    if (redone) *redone = false;
    DevStatus h;
    if (fetched) h = c->hst[slot];
    else if (!fetch_status(c, st, slot, &h, err)) return false;
    // a rerun on another decoder: a call slot of its own, its status into `h`
    auto rerun = [&](auto&& enqueue) {
        DevStatus* st2;
        uint32_t slot2;
        if (!with_call(c, &st2, &slot2, err, enqueue)) return false;
        if (redone) *redone = true;
        return fetch_status(c, st2, slot2, &h, err);
    };
    if (tried_fast == FAST_SEQ && len > 0 && h.fast_fail) {
        if (h.irregular & 2u) {
            // not an f64 frame at all: on to the mixed decoders (as after the length-run probe)
            tried_fast = FAST_RUN;
        } else {
            // an f64 frame whose ids do not count up by one: the length-run (or single-pass)
            // decoder, and this one skipped for the next kSeqSkipCalls calls
            c->seq_left = kSeqSkipCalls;
            if (!rerun([&](DevStatus* st2) {
                    return enqueue_dec_fast(c, f, len, out, st2, &tried_fast, err, false);
                }))
                return false;
        }
    }
    // (irregular bit 1: not an f64 frame at all -- straight on to the mixed decoders)
    if (tried_fast == FAST_RUN && len > 0 && h.fast_fail && (h.irregular & 3u) == 1u) {
        // record lengths vary record to record: the single-pass decoder of any f64 frame, for
        // this frame and the next kIrregularCalls ones
        c->irregular_left = kIrregularCalls;
        if (!rerun([&](DevStatus* st2) { return enqueue_dec_x(c, f, len, out, st2, err); }))
            return false;
        tried_fast = FAST_X;
    }
    // a rejected frame: after the f64 decoders the mixed fast path (mixed columns), after that
    // the general decoder
    while (tried_fast && len > 0 && h.fast_fail) {
        if (tried_fast == FAST_MIX) {
            c->mix_left = kMixFailCalls;
            c->fmx_full = true;  // its next attempt with every candidate kind
        }
        int next = FAST_NONE;
        if (!rerun([&](DevStatus* st2) {
                return tried_fast == FAST_MIX ? enqueue_dec_general(c, f, len, out, st2, err)
                                              : enqueue_dec_mixed(c, f, len, out, st2, &next, err);
            }))
            return false;
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
    if (h.timeout || h.err_kind == NXG_TIMEOUT)
        return refuse(err, "device look-back watchdog expired");
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

}  // namespace nxg_host

namespace {

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

}  // namespace

namespace nxg_host {

bool encode_status_ok(const DevStatus& h, NetidxError* err) {
    if (h.timeout) return refuse(err, "device look-back watchdog expired");
    if (h.err_kind) {
        if (h.err_kind == NXG_TOO_BIG)
            set_err(err, "encode failed: a message exceeds MAX_BATCH (%llu bytes) or a size "
                         "guard (PackError::TooBig)", (unsigned long long)kMaxBatch);
        else
            set_err(err, "encode failed: PackError kind %u", h.err_kind);
        return false;
    }
    return true;
}

bool encode_fits(bool capacity, uint64_t total, uint64_t cap, NetidxError* err) {
    if (!capacity && total <= cap) return true;
    set_err(err, "output buffer too small: need %llu bytes, have %llu", (unsigned long long)total,
            (unsigned long long)cap);
    return false;
}

bool finish_encode(NxgCtx* c, const NxgColumns* in, DevStatus* st, uint32_t slot,
                   uint64_t* len_out, uint64_t cap, bool wrote, NetidxError* err, bool fetched,
                   int fast, const uint8_t* heap, uint8_t* out, bool* redone) {
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
        if (!with_call(c, &st2, &slot2, err, [&](DevStatus* s) {
                return enqueue_encode(c, in, heap, out, cap, s, err, nullptr, false);
            }))
            return false;
        if (redone) *redone = true;
        if (!fetch_status(c, st2, slot2, &h, err)) return false;
        fast = 0;  // (the tiled encoder's status from here on: last_enc_kernel reports it)
    }
    c->last_split = h.split_start;
    if (in->layout == NXG_LAYOUT_F64) c->last_enc_kernel = fast && !h.fast_fail ? 1u : 2u;
    if (!encode_status_ok(h, err)) return false;
    const uint64_t total = h.total_bytes + ctl_total;
    if (len_out) *len_out = total;
    return !wrote || encode_fits(h.capacity, total, cap, err);
}

Span span_of(const void* p, uint64_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    return Span{a, p ? a + bytes : a};
}

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

}  // namespace nxg_host

namespace {

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
    int fast = FAST_NONE;
    return with_call(c, &st, &slot, err, [&](DevStatus* s1) {
               return enqueue_dec_first(c, p.frame, p.len, p.cols, p.flags, s1, &fast, err);
           }) &&
           finish_decode(c, p.frame, p.len, p.cols, fast, st, slot, s, err);
}

// a pending encode done again, synchronously (its input columns or its output buffer were
// rewritten after it ran)
bool redo_encode(NxgCtx* c, const NxgCtx::Pending& p, const NxgColumns* in, NetidxError* err) {
    DevStatus* st;
    uint32_t slot;
    int fast = 0;
    return with_call(c, &st, &slot, err, [&](DevStatus* s1) {
               return enqueue_encode(c, in, p.heap, p.out, p.cap, s1, err, &fast);
           }) &&
           finish_encode(c, in, st, slot, p.len_out, p.cap, true, err, false, fast, p.heap, p.out);
}

}  // namespace

extern "C" {

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

bool nxg_decode_updates(NxgCtx* c, const uint8_t* frame, uint64_t len, NxgColumns* out,
                        uint32_t flags, NxgStatus* ust, NetidxError* err) {
    if (!c || !out || (!frame && len)) return refuse(err, "null argument");
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
    int fast = FAST_NONE;
    if (!with_call(c, &st, &slot, err, [&](DevStatus* s1) {
            return enqueue_dec_first(c, df, len, target, flags, s1, &fast, err);
        }))
        return false;
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
    if (!c || !dout || (!dframe && len)) return refuse(err, "null argument");
    if (c->pending.size() >= kStatusRing / 2) {
        set_err(err, "too many in-flight async calls (max %d); call nxg_ctx_sync", kStatusRing / 2);
        return false;
    }
    if (dout->mem != NXG_MEM_DEVICE || ((uintptr_t)dframe & 15))
        return refuse(err, "async decode needs device columns and a 16-byte aligned device frame");
    DevStatus* st;
    uint32_t slot;
    int fast = FAST_NONE;
    if (!with_call(c, &st, &slot, err, [&](DevStatus* s1) {
            return enqueue_dec_first(c, dframe, len, dout, flags, s1, &fast, err);
        }))
        return false;
    c->pending.push_back({1, fast, dframe, len, dout, nullptr, 0, st, slot, flags});
    c->pending.back().seq = c->calls - 1;
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
        if (!begin_call(c, &st, &slot, err)) return false;  // (no with_call: nxg_host.h)
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
        if (!begin_call(c, &st, &slot, err)) return false;  // (no with_call: nxg_host.h)
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
    if (!c || (n && (!dframes || !lens || !douts))) return refuse(err, "null argument");
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
    if (!c) return refuse(err, "null ctx");
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
    if (!c || !in) return refuse(err, "null argument");
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
    uint64_t total = 0;
    // one encode of the batch into `o` (null: sizing only), then the bound on a write batch
    auto pass = [&](uint8_t* o, uint64_t enc_cap, uint64_t fin_cap) -> bool {
        DevStatus* st;
        uint32_t slot;
        int fast = 0;
        if (!with_call(c, &st, &slot, err, [&](DevStatus* s) {
                return enqueue_encode(c, din, dheap, o, enc_cap, s, err, &fast, true, dwin);
            }))
            return false;
        if (!finish_encode(c, din, st, slot, &total, fin_cap, o != nullptr, err, false, fast, dheap,
                           o))
            return false;
        if (win && total > kMaxBatch) {
            set_err(err, "write batch of %llu bytes exceeds MAX_BATCH (%llu): split the rows",
                    (unsigned long long)total, (unsigned long long)kMaxBatch);
            return false;
        }
        return true;
    };
    // pass 1 (sizing) when writing to a host buffer; a device buffer is written directly. A
    // write batch is also sized first when its buffer could take more than MAX_BATCH bytes, so
    // that such a batch is refused before anything is written (a smaller buffer bounds the
    // writes itself, and the call fails below).
    const bool size_first = win && out && cap > kMaxBatch;
    if ((host && out) || size_first) {
        if (!pass(nullptr, 0, 0) || !encode_fits(false, total, cap, err)) return false;
        if (host && !grow(c, c->dframe, total + 16, kGrowFrame, err)) return false;
        if (host) dout = c->dframe;
        cap = total;
    }
    if (!pass(dout, out ? cap : 0, cap)) return false;
    if (host && out && total) {
        HIPCHK(hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (len_out) *len_out = total;
    return true;
}

bool nxg_encoded_len(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint64_t* len_out,
                     NetidxError* err) {
    return encode_impl(c, in, heap, nullptr, 0, len_out, err);
}

bool nxg_encode_updates(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                        uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!out) return refuse(err, "null output buffer");
    return encode_impl(c, in, heap, out, cap, len_out, err);
}

// ---- subscriber write batches: publisher::To (publisher.rs:50-70) ------------------------------
bool nxg_write_cols_alloc(NxgCtx* c, uint64_t cap_rows, uint32_t mem, NxgWriteCols* out,
                          NetidxError* err) {
    if (!c || !out) return refuse(err, "null argument");
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
    if (!c || !out || !wout || !ust || (!frame && len)) return refuse(err, "null argument");
    if (opts && (opts->fast > 1u || opts->reserved != 0u)) {
        set_err(err, "NxgWriteDecodeOpts: fast = %u (0 or 1), reserved = %u (must be 0)",
                opts->fast, opts->reserved);
        return false;
    }
    const bool try_fast = opts && opts->fast == 1u && nxg_wfast_takes(len);
    // (the argument checks come before any use of the context)
    if (!mixed_capable(out) || !out->id || !out->fixed)
        return refuse(err, "write batches decode into MIXED-layout columns");
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
        // (none is null: the checks above)
        if (!all_device({out->id, out->tag, out->fixed, out->aux, out->ctag, out->cfixed, out->caux,
                         out->ctl_row, out->ctl_off, out->ctl_len, out->ctl_variant, wout->wflags,
                         wout->wid}))
            return refuse(err, "a column array is not device memory");
    }
    const uint8_t* df;
    if (!frame_to_device(c, frame, len, &df, err)) return false;
    DevStatus* st;
    uint32_t slot;
    const ColsDesc d = desc_of(target, &wtarget);
    bool took = false;  // the fast decoder took the frame
    if (try_fast) {
        DevStatus h;
        // one buffer for both decoders, so that a fallback does not reallocate
        const size_t need = std::max(nxg_wfast_scratch_bytes(len), nxg_dec_gen_scratch_bytes(len));
        if (!with_call(c, &st, &slot, err, [&](DevStatus* s) {
                return ensure_glws(c, need, err) &&
                       launch_ok(nxg_launch_dec_wfast(df, len, d, c->glws, s, c->stream),
                                 "fast To decode launch failed", err);
            }) ||
            !fetch_status(c, st, slot, &h, err))
            return false;
        took = !h.fast_fail;
    }
    if (!took &&
        !with_call(c, &st, &slot, err, [&](DevStatus* s) {
            return ensure_glws(c, nxg_dec_gen_scratch_bytes(len), err) &&
                   launch_ok(nxg_launch_dec_gen(
                                 df, len, d, reinterpret_cast<uint32_t*>(c->glws.get()), c->gruns,
                                 c->gruns + (size_t)gdec2::MAX_RUNS * gdec2::RUN_WORDS,
                                 c->wgs_dec_gen, s, c->stream, true),
                             "To decode launch failed", err);
        }))
        return false;
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
    if (!c || !in || !win) return refuse(err, "null argument");
    if (in->layout != NXG_LAYOUT_MIXED || !mixed_capable(in))
        return refuse(err, "write batches encode from MIXED-layout columns");
    if (in->n_rows && (!win->wflags || !win->wid || win->cap_rows < in->n_rows)) {
        set_err(err, "write columns hold %llu rows, the batch %llu",
                (unsigned long long)win->cap_rows, (unsigned long long)in->n_rows);
        return false;
    }
    if (in->n_rows && (in->mem != win->mem || is_device_ptr(in->id) != is_device_ptr(win->wid)))
        return refuse(err, "columns and write columns must both be device or both host memory");
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

bool nxg_encode_updates_async(NxgCtx* c, const NxgColumns* din, const uint8_t* dheap,
                              uint8_t* dout, uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!c || !din || !dout) return refuse(err, "null argument");
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
    int fast = 0;
    if (!with_call(c, &st, &slot, err, [&](DevStatus* s) {
            return enqueue_encode(c, din, dheap, dout, cap, s, err, &fast);
        }))
        return false;
    c->pending.push_back({2, fast, nullptr, 0, const_cast<NxgColumns*>(din), len_out, cap, st,
                          slot, 0, dheap, dout, c->calls - 1});
    return true;
}

bool nxg_encode_frames(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                       uint64_t cap, uint64_t* len_out, uint64_t* chunk_len_out,
                       uint64_t cap_chunks, uint64_t* n_chunks, NetidxError* err) {
    if (!out || !n_chunks || (cap_chunks && !chunk_len_out)) return refuse(err, "null argument");
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

}  // extern "C"
