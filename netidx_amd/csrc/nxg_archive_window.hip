// nxg_archive_window.hip -- a window of archive records decoded in one call, and its image, for
// gfx950: the get_batch_at loops of ArchiveReader::read_deltas / build_image
// (netidx-archive/src/logfile/reader.rs:590-631, 492-557) and build_image's image.extend fold.
//
// Archive batches come in two sizes: one large image record, then many deltas of tens of items.
// The fast single-batch decoder (nxg_archive_fast.hip: 4 KiB tiles, count / fix / resolve / emit)
// is built for the large kind; here the small kind gets one launch set for the whole window:
//
//   count   one wave per record, over a persistent grid-stride loop; records are independent, so
//           no wave waits on another. The wave stages the record in LDS 4 KiB at a time (an image
//           of SIMG bytes whose first item starts in its first 16), walks item boundaries
//           uniformly -- the Id varint, then 0x40 or the value's size from its tag, text length or
//           element count -- collecting up to 64 item starts, and decodes those 64 one per lane
//           with the LDS-image helpers of nxg_fmx_common.h (val_decode, the utf8 checks,
//           round_elements). It writes rows, child slots and bytes consumed per record, or
//           declines the record: an Id wider than 5 bytes, a Map, Error(Value) of a non-String, a
//           nested or 128+-element Array, an Array larger than the image, any parse error, a
//           count the items do not bear out.
//   scan    one block: exclusive sums of (rows, child slots) over the records, the declined and
//           large ones with the counts the host learned from the single-batch decoder.
//   emit    the count pass again, writing rows at row_off and children at child_off.
//   rebase  a record decoded by nxg_decode_archive_batch into the ctx's scratch columns, copied to
//           its place: out_off added to text offsets, child_off to child indices (children too).
//
// The image (last row per Id): a mark pass (atomicMax of row + 1 into a dense table of n_ids
// entries, the last_row mechanism of nxg_dispatch.hip), a flag scan (nxg_scan_u32), a gather.
#include "nxg_fmx_common.h"

namespace aw {
constexpr uint32_t UNSUB = 0x40;           // Event::Unsubscribed (subscriber/mod.rs:168)
constexpr uint32_t SIMG = fmx::IMG + 16;   // stage image: the first item starts in bytes 0..15
constexpr uint32_t SIL = SIMG - 24;        // items end before this (text aside)
constexpr uint32_t NCHUNK = (SIMG + 15) / 16;
}  // namespace aw

namespace {
using namespace fmx;
using namespace aw;

struct AwLds {
    uint8_t img[SIMG + 48];  // (the text checks read up to 36 bytes past a text's last byte)
    uint32_t el[MAXC];       // text checks / a round's array elements
    uint8_t mark[256];       // utf8_packed, round_elements
};

constexpr uint32_t kTextTags = B(12) | B(13) | B(18);

// The end (image offset) of a non-Array value with tag t at q (structure only, as dleaf sizes
// it), or FAIL; wl: the record's end. Fixed-size, varint and Decimal values must end before il;
// text, Bytes and Abstract payloads may run past the image (their bytes are not read here).
NXG_DEV uint32_t leaf_end(lds_bytes img, uint32_t q, uint32_t t, uint32_t wl, uint32_t il) {
    if (t >= 28u) return FAIL;
    const uint32_t bit = 1u << t;
    const uint32_t lim = min(wl, il);
    const uint32_t f1 = fixed_size1(t);
    if (f1) return q + f1 <= lim ? q + f1 : FAIL;
    if (bit & B(20)) return q + 17u <= lim ? q + 17u : FAIL;  // Decimal: 16 bytes
    uint32_t u = q + 1;
    if (bit & B(22)) {  // Error(String) only
        if (img[u] != 12u) return FAIL;
        u++;
    }
    const Win16 v = win16(img, u);
    uint64_t x;
    const uint32_t nb = wvar(v.lo, v.hi, x);
    if (nb == 0) return FAIL;
    const uint32_t s = u + nb;
    if (bit & kVarTags) return s <= lim ? s : FAIL;
    if (s > wl || s > il || !(bit & (kTextTags | B(22) | B(27)))) return FAIL;  // Map, Array
    uint64_t take = x;
    if (bit & B(27)) {  // Abstract: len-wrapped, at least 16 bytes (dleaf case 27)
        if (x < 1) return FAIL;
        take = x - vl64(x);
        if (take < 16) return FAIL;
    }
    return take < (uint64_t)(wl - s) || (take == (uint64_t)(wl - s) && !(bit & B(27)))
               ? s + (uint32_t)take
               : FAIL;
}

// The end of the item at image offset p (p + 24 <= il): Id varint (at most 5 bytes), then 0x40 or
// a value; an Array's elements are walked (fewer than 128, non-containers, ending before il).
NXG_DEV uint32_t item_end(lds_bytes img, uint32_t p, uint32_t wl, uint32_t il) {
    const Win16 w = win16(img, p);
    const uint64_t stop = ~w.lo & 0x8080808080808080ull;
    const uint32_t k = stop ? (uint32_t)__builtin_ctzll(stop) >> 3 : 8u;
    if (k >= 5u) return FAIL;
    const uint32_t q = p + k + 1;  // the Event's first byte
    if (q >= wl) return FAIL;
    const uint32_t t = (uint32_t)(w.lo >> (8 * (k + 1))) & 0xffu;
    if (t == UNSUB) return q + 1;
    if (t != 19u) return leaf_end(img, q, t, wl, il);
    if (q + 2 > wl) return FAIL;
    const uint32_t c = img[q + 1];
    if (c >= 0x80u) return FAIL;
    uint32_t e = q + 2;
#pragma unroll 1
    for (uint32_t i = 0; i < c && e != FAIL; i++) {
        if (e >= il || e >= wl) return FAIL;
        const uint32_t et = img[e];
        e = et == 19u ? FAIL : leaf_end(img, e, et, wl, il);
    }
    return e != FAIL && e <= min(wl, il) ? e : FAIL;
}

// the stage image: record bytes [s0 - d, s0 - d + SIMG) with d = the low 4 bits of the address of
// record byte s0, so that every 16-byte load is aligned; zeros outside the record
NXG_DEV uint32_t stage_load(uint8_t* img, const uint8_t* __restrict__ rec, uint64_t W, uint64_t s0,
                            uint32_t lane) {
    const uint32_t d = (uint32_t)((uintptr_t)(rec + s0) & 15u);
    wave_lds_order();  // the previous stage's reads are issued
#pragma unroll
    for (uint32_t i = 0; i < (NCHUNK + 63) / 64; i++) {
        const uint32_t c = i * 64 + lane;
        if (c < NCHUNK) {
            const int64_t rel = (int64_t)s0 - (int64_t)d + (int64_t)c * 16;
            uint4 v;
            if (rel >= 0 && (uint64_t)rel + 16 <= W) {
                v = *reinterpret_cast<const uint4*>(rec + rel);
            } else {
                uint32_t q[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; k++) {
                    const int64_t b = rel + k;
                    if (b >= 0 && (uint64_t)b < W) q[k >> 2] |= (uint32_t)rec[b] << (8 * (k & 3));
                }
                v = make_uint4(q[0], q[1], q[2], q[3]);
            }
            *reinterpret_cast<uint4*>(img + c * 16) = v;
        }
    }
    wave_lds_order();
    return d;
}

struct AwOut {
    uint64_t rows, kids, consumed;
    bool ok;
};

// One record by one wave: the count pass (EMIT false: nothing is written, cols.cap_children is 0)
// or the emit pass (rows from row0, children from child0). Uniform result.
template <bool EMIT>
NXG_DEV AwOut wave_record(const uint8_t* __restrict__ dbuf, uint64_t off, uint64_t W,
                          uint64_t row0, uint64_t child0, const ColsDesc& cols, AwLds& L,
                          uint32_t lane) {
    AwOut r{0, 0, 0, false};
    if (W == 0 || W >= 0xfff00000ull) return r;
    const uint8_t* rec = dbuf + off;
    uint8_t* img = L.img;
    const lds_bytes limg = (lds_bytes)img;
    uint64_t s0 = 0;
    uint32_t d = stage_load(img, rec, W, 0, lane);
    uint32_t wl = d + (uint32_t)W;  // the record's end as an image offset (may lie past the image)
    // the count (decode_varint, pack.rs:504-520) and Vec::decode's guard (pack.rs:919-925)
    uint64_t count;
    uint32_t x;
    {
        const Win16 v = win16(limg, d);
        const uint32_t nb = wvar(v.lo, v.hi, count);
        if (nb == 0 || nb > W) return r;
        const uint64_t sz = count > ~0ull / 24 ? ~0ull : count * 24;
        if (sz > kMaxVecBytes || sz > ((W - nb) << 8)) return r;
        x = d + nb;
    }
    uint64_t done = 0, cnext = child0;
    uint32_t first = x;  // the stage's first item: one that does not parse here does not parse
#pragma unroll 1
    while (done < count) {
        // up to 64 item starts, one per lane
        uint32_t n = 0, p = d;
        bool restage = false;
#pragma unroll 1
        while (n < 64u && done + n < count) {
            if (x >= wl) return r;  // fewer items than the count
            if (x + 24u > SIL) {
                restage = true;
                break;
            }
            const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)item_end(limg, x, wl, SIL));
            if (e == FAIL) {
                if (x == first) return r;
                restage = true;
                break;
            }
            if (lane == n) p = x;
            n++;
            x = e;
            if (x > SIL) break;  // text that leaves the image
        }
        if (n) {
            const uint64_t t0 = off + s0 - d;  // dbuf offset of image byte 0
            const uint32_t elim = min(wl, SIL);
            const bool has = lane < n;
            // Id varint (at most 5 bytes: item_end), the Event's first byte, then 12 bytes
            uint32_t h[5];
            win_words<5>(limg, p, h);
            const uint32_t a = h[0], b = h[1];
            const uint32_t sa = ~a & 0x80808080u;
            const uint32_t nb = sa ? ((uint32_t)__builtin_ctz(sa) >> 3) + 1 : 5u;
            const uint64_t id = (uint64_t)compress7_32(nb >= 4u ? a : (a & ((1u << (8u * nb)) - 1u))) |
                                (nb == 5u ? (uint64_t)(b & 0x7fu) << 28 : 0ull);
            const uint32_t tg = (uint32_t)(((((uint64_t)b << 32) | a) >> (8u * nb)) & 0xffu);
            const uint32_t u = nb + 1u;  // the payload, relative to p: 2..6
            const bool up = u >= 4u;
            const uint32_t g0 = up ? h[1] : h[0], g1 = up ? h[2] : h[1], g2 = up ? h[3] : h[2],
                           g3 = up ? h[4] : h[3];
            const uint32_t su = u & 3u;
            const bool un = tg == UNSUB;
            FV o = val_decode(un ? 1u : tg, alignbyte(g1, g0, su), alignbyte(g2, g1, su),
                              alignbyte(g3, g2, su), p + u, wl, true, t0);
            if (un) o = FV{0ull, UNSUB, 0u, p + u, 0u, 0u, 0u, true};
            // text past the image: checked from global memory; everything else ends in it
            const bool far = has && o.ok && o.end > SIL;
            const bool arr = o.tag == 19u;
            bool ok = !has || ((sa != 0u || !(b & 0x80u)) && o.ok && (!far || !arr) &&
                               (!arr || o.end <= elim));
            {
                const bool fw = far && ok && o.slen;
                const bool fo = far_text_ok(dbuf, fw, t0 + o.soff, o.slen, lane);
                if (fw) ok = fo;
            }
            if (__any(!ok)) return r;
            {  // text inside the image
                const bool tx = has && !far && o.slen;
                const uint64_t tm = __ballot(tx);
                if (tx)
                    L.el[__builtin_amdgcn_mbcnt_hi((uint32_t)(tm >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)tm, 0u))] =
                        o.soff | (o.slen << 16);
                wave_lds_order();
                if (tm && !text_flush(limg, L.el, (uint32_t)__popcll(tm), L.mark, lane, nullptr))
                    return r;
                wave_lds_order();
            }
            const uint32_t kd = has ? o.kids : 0u;
            const uint32_t kinc = wave_incl_scan<uint32_t>(kd);
            const uint32_t kpre = kinc - kd;
            const uint32_t rk = wave_last<uint32_t>(kinc);
            if (EMIT && has) {
                const uint64_t row = row0 + done + lane;
                col_st(&cols.id[row], (uint64_t)(uint32_t)id);  // Id(decode_varint as u32)
                col_st(&cols.tag[row], (uint8_t)o.tag);
                col_st(&cols.fixed[row], (uint64_t)(arr ? cnext + kpre : o.fixed));
                col_st(&cols.aux[row], (uint32_t)o.aux);
            }
            if (rk) {
                uint32_t ntxt = 0;
                if (round_elements(img, L.mark, L.el, kd, kpre, rk, o.end, elim, cnext, cols, t0,
                                   lane, ntxt, nullptr))
                    return r;
            }
            cnext += rk;
            done += n;
        }
        if (done < count && (restage || x + 24u > SIL)) {
            s0 += x - d;
            if (s0 >= W) return r;
            d = stage_load(img, rec, W, s0, lane);
            wl = d + (uint32_t)(W - s0);
            x = d;
            first = x;
        }
    }
    r.rows = count;
    r.kids = cnext - child0;
    r.consumed = s0 + (x - d);
    r.ok = true;
    return r;
}

}  // namespace

// count pass: one wave per wave-route record, grid-stride
__global__ __launch_bounds__(TPB) void nxg_aw_count_kernel(const uint8_t* __restrict__ dbuf,
                                                           AwRec* __restrict__ recs, uint32_t n) {
    __shared__ __attribute__((aligned(16))) AwLds lds[TPB / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t nw = gridDim.x * (TPB / 64);
    ColsDesc none{};  // capacity 0: round_elements writes nothing
#pragma unroll 1
    for (uint32_t i = blockIdx.x * (TPB / 64) + w; i < n; i += nw) {
        const uint32_t route = __builtin_amdgcn_readfirstlane((int)recs[i].route);
        if (route != 1u) continue;
        const uint64_t off = recs[i].off, len = recs[i].len;
        const AwOut o = wave_record<false>(dbuf, off, len, 0, 0, none, lds[w], lane);
        if (lane == 0) {
            recs[i].rows = o.ok ? o.rows : 0;
            recs[i].kids = o.ok ? o.kids : 0;
            recs[i].consumed = o.ok ? o.consumed : 0;
            recs[i].declined = o.ok ? 0u : 1u;
        }
    }
}

// scan: row_off / child_off of every record, the totals into the head (one block)
__global__ __launch_bounds__(TPB) void nxg_aw_scan_kernel(AwRec* __restrict__ recs, uint32_t n,
                                                          AwHead* __restrict__ hp) {
    __shared__ uint64_t tmp[TPB / 64];
    uint64_t rrun = 0, krun = 0;
#pragma unroll 1
    for (uint32_t b = 0; b < n; b += TPB) {
        const uint32_t i = b + threadIdx.x;
        const uint64_t rv = i < n ? recs[i].rows : 0ull, kv = i < n ? recs[i].kids : 0ull;
        uint64_t rt, kt;
        const uint64_t re = block_excl_scan<uint64_t, TPB>(rv, tmp, &rt);
        const uint64_t ke = block_excl_scan<uint64_t, TPB>(kv, tmp, &kt);
        if (i < n) {
            recs[i].row_off = rrun + re;
            recs[i].child_off = krun + ke;
        }
        rrun += rt;
        krun += kt;
    }
    if (threadIdx.x == 0) {
        hp->rows = rrun;
        hp->kids = krun;
    }
}

// emit pass: the wave-route records the count pass took
__global__ __launch_bounds__(TPB) void nxg_aw_emit_kernel(const uint8_t* __restrict__ dbuf,
                                                          const AwRec* __restrict__ recs,
                                                          uint32_t n, ColsDesc cols,
                                                          AwHead* __restrict__ hp) {
    __shared__ __attribute__((aligned(16))) AwLds lds[TPB / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t nw = gridDim.x * (TPB / 64);
#pragma unroll 1
    for (uint32_t i = blockIdx.x * (TPB / 64) + w; i < n; i += nw) {
        const uint32_t route = __builtin_amdgcn_readfirstlane((int)recs[i].route);
        const uint32_t dec = __builtin_amdgcn_readfirstlane((int)recs[i].declined);
        if (route != 1u || dec) continue;
        const AwRec r = recs[i];
        // (the host checked the totals against the capacities: every row and child fits)
        const AwOut o = wave_record<true>(dbuf, r.off, r.len, r.row_off, r.child_off, cols, lds[w],
                                          lane);
        if (lane == 0 && !(o.ok && o.rows == r.rows && o.kids == r.kids)) atomicOr(&hp->emit_fail, 1u);
    }
}

namespace {
// Array, Map, Error(Value): `fixed` is the first child slot; String, Bytes, Error(String), Decimal,
// Abstract: `fixed` is the payload's offset in the heap (include/nxg_codec.h)
NXG_DEV bool container(uint32_t t) { return t == 19 || t == 21 || t == 22; }
NXG_DEV bool in_heap(uint32_t t) { return t == 12 || t == 13 || t == 18 || t == 20 || t == 27; }
NXG_DEV uint64_t rebase(uint32_t t, uint64_t f, uint64_t child_off, uint64_t text_off) {
    return container(t) ? f + child_off : (in_heap(t) ? f + text_off : f);
}
}  // namespace

// rows [0, nr) and children [0, nc) of src to dst at row_off / child_off, re-based
__global__ __launch_bounds__(TPB) void nxg_aw_rebase_kernel(ColsDesc src, ColsDesc dst, uint64_t nr,
                                                            uint64_t nc, uint64_t row_off,
                                                            uint64_t child_off, uint64_t text_off) {
    const uint64_t n = nr > nc ? nr : nc;
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
#pragma unroll 1
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        if (i < nr && row_off + i < dst.cap_rows) {
            const uint32_t t = src.tag[i];
            dst.id[row_off + i] = src.id[i];
            dst.tag[row_off + i] = (uint8_t)t;
            dst.fixed[row_off + i] = rebase(t, src.fixed[i], child_off, text_off);
            dst.aux[row_off + i] = src.aux[i];
        }
        if (i < nc && child_off + i < dst.cap_children) {
            const uint32_t t = src.ctag[i];
            dst.ctag[child_off + i] = (uint8_t)t;
            dst.cfixed[child_off + i] = rebase(t, src.cfixed[i], child_off, text_off);
            dst.caux[child_off + i] = src.caux[i];
        }
    }
}

// ---- the image --------------------------------------------------------------------------------
// mark: table[id] = max(row + 1) over the kept rows
__global__ __launch_bounds__(TPB) void nxg_aw_mark_kernel(const uint64_t* __restrict__ id,
                                                          uint64_t n, uint64_t n_ids,
                                                          const uint8_t* __restrict__ keep,
                                                          unsigned long long* __restrict__ table,
                                                          AwHead* __restrict__ hp) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    uint32_t dropped = 0;
    // (whole waves: the trip count is the same for every lane of a block)
    const uint64_t trips = (n + stride - 1) / stride;
#pragma unroll 1
    for (uint64_t k = 0; k < trips; k++) {
        const uint64_t r = k * stride + (uint64_t)blockIdx.x * TPB + threadIdx.x;
        if (r >= n) continue;
        const uint64_t v = id[r];
        if (v >= n_ids) {
            atomicMin((unsigned long long*)&hp->bad_row, (unsigned long long)r);
        } else if (keep && !keep[v]) {
            dropped++;
        } else {
            atomicMax(&table[v], (unsigned long long)(r + 1));
        }
    }
    const uint32_t ws = wave_sum<uint32_t>(dropped);
    if ((threadIdx.x & 63) == 0 && ws)
        atomicAdd((unsigned long long*)&hp->n_filtered, (unsigned long long)ws);
}

__global__ __launch_bounds__(TPB) void nxg_aw_flag_kernel(const unsigned long long* __restrict__ table,
                                                          uint64_t n_ids,
                                                          uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n_ids) flag[i] = table[i] != 0ull;
}

// gather: Id i's winning row to image row pos[i] (ascending Id order)
__global__ __launch_bounds__(TPB) void nxg_aw_gather_kernel(
    const unsigned long long* __restrict__ table, const uint64_t* __restrict__ pos, uint64_t n_ids,
    ColsDesc win, uint64_t cap, uint64_t* __restrict__ oid, uint8_t* __restrict__ otag,
    uint64_t* __restrict__ ofixed, uint32_t* __restrict__ oaux, uint64_t* __restrict__ osrc,
    AwHead* __restrict__ hp) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_ids) return;
    const uint64_t t = table[i], p = pos[i];
    if (i + 1 == n_ids) hp->n_image = p + (t != 0);
    if (!t || p >= cap) return;
    const uint64_t r = t - 1;
    oid[p] = i;
    otag[p] = win.tag[r];
    ofixed[p] = win.fixed[r];
    oaux[p] = win.aux[r];
    osrc[p] = r;
}

// ---- launch (host) ------------------------------------------------------------------------------
static uint32_t aw_grid(uint32_t n, int ncu) {
    const uint32_t want = (n + TPB / 64 - 1) / (TPB / 64);
    const uint32_t most = (uint32_t)(ncu > 0 ? ncu : 256) * 6u;  // LDS: 7 workgroups per CU
    return want < 1 ? 1 : (want < most ? want : most);
}

hipError_t nxg_launch_aw_count(const uint8_t* dbuf, void* drecs, uint32_t n, int ncu,
                               hipStream_t s) {
    hipLaunchKernelGGL(nxg_aw_count_kernel, dim3(aw_grid(n, ncu)), dim3(TPB), 0, s, dbuf,
                       reinterpret_cast<AwRec*>(drecs), n);
    return hipGetLastError();
}

hipError_t nxg_launch_aw_scan(void* drecs, uint32_t n, void* dhead, hipStream_t s) {
    hipLaunchKernelGGL(nxg_aw_scan_kernel, dim3(1), dim3(TPB), 0, s, reinterpret_cast<AwRec*>(drecs),
                       n, reinterpret_cast<AwHead*>(dhead));
    return hipGetLastError();
}

hipError_t nxg_launch_aw_emit(const uint8_t* dbuf, const void* drecs, uint32_t n,
                              const ColsDesc& cols, void* dhead, int ncu, hipStream_t s) {
    hipLaunchKernelGGL(nxg_aw_emit_kernel, dim3(aw_grid(n, ncu)), dim3(TPB), 0, s, dbuf,
                       reinterpret_cast<const AwRec*>(drecs), n, cols,
                       reinterpret_cast<AwHead*>(dhead));
    return hipGetLastError();
}

hipError_t nxg_launch_aw_rebase(const ColsDesc& src, const ColsDesc& dst, uint64_t nr, uint64_t nc,
                                uint64_t row_off, uint64_t child_off, uint64_t text_off,
                                hipStream_t s) {
    const uint64_t n = nr > nc ? nr : nc;
    if (n == 0) return hipSuccess;
    const uint64_t g = (n + TPB - 1) / TPB;
    hipLaunchKernelGGL(nxg_aw_rebase_kernel, dim3((uint32_t)(g > 4096 ? 4096 : g)), dim3(TPB), 0, s,
                       src, dst, nr, nc, row_off, child_off, text_off);
    return hipGetLastError();
}

uint64_t nxg_aw_image_scratch_bytes(uint64_t n_ids) {
    // table 8, flags 4, positions 8 per Id; nxg_scan_u32's block sums
    return 20 * n_ids + 8 * (n_ids / 4096 + 2) + 64;
}

// `scratch`: nxg_aw_image_scratch_bytes(n_ids) bytes; dhead: an AwHead (bad_row, n_filtered and
// n_image are set here). The rows land in ascending Id order.
hipError_t nxg_launch_aw_image(const ColsDesc& win, uint64_t n_rows, uint64_t n_ids,
                               const uint8_t* keep, uint8_t* scratch, uint64_t cap, uint64_t* oid,
                               uint8_t* otag, uint64_t* ofixed, uint32_t* oaux, uint64_t* osrc,
                               void* dhead, hipStream_t s) {
    AwHead* hp = reinterpret_cast<AwHead*>(dhead);
    AwHead h0{};
    h0.bad_row = ~0ull;
    hipError_t e;
    if ((e = hipMemcpyAsync(hp, &h0, sizeof h0, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if (n_ids == 0) return hipSuccess;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(scratch);
    uint64_t* pos = reinterpret_cast<uint64_t*>(scratch + 8 * n_ids);
    uint64_t* bsum = pos + n_ids;
    uint32_t* flag = reinterpret_cast<uint32_t*>(bsum + (n_ids / 4096 + 2));
    if ((e = hipMemsetAsync(table, 0, 8 * n_ids, s)) != hipSuccess) return e;
    if (n_rows) {
        const uint64_t g = (n_rows + TPB - 1) / TPB;
        hipLaunchKernelGGL(nxg_aw_mark_kernel, dim3((uint32_t)(g > 4096 ? 4096 : g)), dim3(TPB), 0,
                           s, win.id, n_rows, n_ids, keep, table, hp);
    }
    const uint32_t gi = (uint32_t)((n_ids + TPB - 1) / TPB);
    hipLaunchKernelGGL(nxg_aw_flag_kernel, dim3(gi), dim3(TPB), 0, s, table, n_ids, flag);
    if ((e = nxg_scan_u32(flag, n_ids, pos, bsum, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(nxg_aw_gather_kernel, dim3(gi), dim3(TPB), 0, s, table, pos, n_ids, win, cap,
                       oid, otag, ofixed, oaux, osrc, hp);
    return hipGetLastError();
}
