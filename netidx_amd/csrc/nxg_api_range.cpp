// nxg_api_range.cpp -- the multi-GPU decode calls of the C ABI (include/nxg_codec.h): one byte
// range of a frame, the link of the ranges, one share of a frame's rows.
#include "nxg_host.h"

using namespace nxg_host;

extern "C" {

// ---- byte-range decode (multi-GPU) ---------------------------------------------------------------
bool nxg_decode_range(NxgCtx* c, const uint8_t* dframe, uint64_t W, uint64_t begin, uint64_t end,
                      NxgColumns* out, NxgRange* rng, NetidxError* err) {
    if (!c || !out || !rng || (!dframe && W)) return refuse(err, "null argument");
    if (begin > end || end > W) {
        set_err(err, "bad range [%llu, %llu) of a %llu-byte frame", (unsigned long long)begin,
                (unsigned long long)end, (unsigned long long)W);
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (out->mem != NXG_MEM_DEVICE || !is_device_ptr(dframe))
        return refuse(err, "range decode needs a device frame and device columns");
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
    const char* const launch = "range decode launch";
    // one decoder's attempt: a call slot of its own, its status into *hs (with the copies `also`
    // enqueues in front of the same wait)
    auto attempt = [&](DevStatus* hs, auto&& enqueue, auto&& also) {
        DevStatus* st;
        uint32_t slot;
        return with_call(c, &st, &slot, err, enqueue) && fetch_status(c, st, slot, hs, err, also);
    };
    const auto nothing = [] { return true; };
    const uint64_t nt = nxg_dec_f64r_tiles(R);
    uint8_t d0[16], dl[16];
    DevStatus h, h2;
    if (!attempt(
            &h,
            [&](DevStatus* st) {
                return ensure_tstat(c, nxg_dec_f64r_groups(R), err) &&
                       ensure_rdesc(c, 16 * nt, err) &&
                       launch_ok(nxg_launch_dec_f64r(dframe, W, begin, end, out->id, out->fixed,
                                                     out->cap_rows, c->rdesc, c->tstat, c->epoch,
                                                     c->f64r_flags, st, c->stream),
                                 launch, err);
            },
            [&] {  // the first and the last tile descriptor
                HIPCHK(hipMemcpyAsync(d0, c->rdesc, 16, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipMemcpyAsync(dl, c->rdesc + 16 * (nt - 1), 16, hipMemcpyDeviceToHost,
                                      c->stream));
                return true;
            }))
        return false;
    if (h.timeout) return refuse(err, "device look-back watchdog expired");
    c->last = h;
    bool declined = h.fast_fail != 0;
    if (declined && (h.irregular & 3u) == 1u) {
        // record lengths that vary record to record (ids in any order: a batch updating an
        // arbitrary subset of a publisher's values): the single-pass decoder in range mode
        if (!attempt(
                &h2,
                [&](DevStatus* st) {
                    return ensure_tstat(c, nxg_dec_f64x_groups(R), err) &&
                           launch_ok(nxg_launch_dec_f64x_range(dframe, W, begin, end, out->id,
                                                               out->fixed, out->cap_rows, c->tstat,
                                                               c->epoch, st, c->stream),
                                     launch, err);
                },
                nothing))
            return false;
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
        if (!attempt(
                &h2,
                [&](DevStatus* st) {
                    return ensure_glws(c, nxg_fmx_scratch_bytes(R), err) &&
                           launch_ok(nxg_launch_dec_fmx_range(dframe, W, begin, end, desc_of(out),
                                                              c->glws, c->wgs_fmx, st, c->stream),
                                     launch, err);
                },
                nothing))
            return false;
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
    if (!r || (n && !row_off)) return refuse(err, "null argument");
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
    if (out->mem != NXG_MEM_DEVICE || (W && !is_device_ptr(dframe)))
        return refuse(err, "share decode needs a device frame and device columns");
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
        int fast = FAST_NONE;
        if (!with_call(c, &st, &slot, err, [&](DevStatus* s1) {
                return enqueue_dec_fast(c, dframe, W, &v, s1, &fast, err);
            }))
            return false;
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

}  // extern "C"
