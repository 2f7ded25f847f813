// nxg_api_archive.cpp -- the archive calls of the C ABI (include/nxg_codec.h): archive batches,
// zstd dictionaries, decompression and compression, a window of records and its image, recording
// a dispatch's entries, the RecordIndex of an indexed archive (written and scanned), replay.
#include <mutex>

#include "nxg_host.h"
#include "nxg_archive_index.h"
#include "nxg_record.h"
#include "nxg_replay.h"

using namespace nxg_host;

// ---- what other archive-side files share (nxg_host.h) ------------------------------------------
const char* nxg_host::rec_cause(uint32_t cause) {
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

bool nxg_host::window_records(const NxgColumns* window, const NxgArchiveBatchInfo* info,
                              uint32_t n_recs, std::vector<uint64_t>* hbeg,
                              std::vector<uint64_t>* hend, NetidxError* err) {
    hbeg->assign((size_t)n_recs + 1, 0);
    hend->assign(n_recs, 0);
    for (uint32_t i = 0; i < n_recs; i++) {
        const uint64_t lo = info[i].row_off, cnt = info[i].n_rows;
        if (lo > window->n_rows || cnt > window->n_rows - lo) {
            set_err(err, "info[%u]: rows [%llu, + %llu) leave the window's %llu rows", i,
                    (unsigned long long)lo, (unsigned long long)cnt,
                    (unsigned long long)window->n_rows);
            return false;
        }
        if (i && lo < (*hend)[i - 1]) {
            set_err(err, "info[%u].row_off (%llu) lies in front of the end of record %u (%llu): "
                         "row_off must not decrease and records must not overlap", i,
                    (unsigned long long)lo, i - 1, (unsigned long long)(*hend)[i - 1]);
            return false;
        }
        (*hbeg)[i] = lo;
        (*hend)[i] = lo + cnt;
    }
    (*hbeg)[n_recs] = n_recs ? (*hend)[n_recs - 1] : 0;
    return true;
}

extern "C" {

// ---- archive batches (netidx-archive logfile/mod.rs:150-205) ---------------------------------
// <Vec<BatchItem> as Pack>::encode (pack.rs:941-952): the count varint here, the items by the
// general encoder's rows kernel in archive mode
bool nxg_encode_archive_batch(NxgCtx* c, const NxgColumns* in, const uint8_t* heap, uint8_t* out,
                              uint64_t cap, uint64_t* len_out, NetidxError* err) {
    if (!c || !in) return refuse(err, "null argument");
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
    if (!with_call(c, &st, &slot, err, [&](DevStatus* s) {
            const hipError_t le =
                nxg_launch_enc_general(desc_of(in), heap, out, out ? cap : 0, c->escratch, c->tstat,
                                       c->epoch, s, c->grid_enc_gen, c->stream, hl);
            HIPCHK(le);
            return true;
        }))
        return false;
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
    if (!c || (n && (!recs || !src))) return refuse(err, "null argument");
    if (!no_pending(c, err)) return false;
    if (is_device_ptr(src))
        return refuse(err, "the records must be in host memory (the archive's mmap)");
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
        if (!nxg_zstd_build_defaults(reinterpret_cast<NxzDefaults*>(h.data())))
            return refuse(err, "predefined zstd tables");
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
    if (d->device != c->device) return refuse(err, "the dictionary belongs to another device");
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
    if (!c || (n && (!recs || !src))) return refuse(err, "null argument");
    const uint32_t literals = opts ? opts->literals : (uint32_t)NXG_ZSTD_LIT_DICT_TREE;
    if (literals > NXG_ZSTD_LIT_BLOCK_TREES) {
        set_err(err, "NxgZstdCompressOpts.literals: unknown value %u", literals);
        return false;
    }
    if (opts && (opts->reserved[0] | opts->reserved[1] | opts->reserved[2]))
        return refuse(err, "NxgZstdCompressOpts.reserved must be zero");
    if (!no_pending(c, err)) return false;
    if (is_device_ptr(src) || (out && is_device_ptr(out)))
        return refuse(err, "the records and the output must be in host memory");
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
        if (!nxg_zstd_build_enc_tables(h.data()))
            return refuse(err, "predefined zstd encoding tables");
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
    if (!c || !out || (!buf && len)) return refuse(err, "null argument");
    if (!no_pending(c, err)) return false;
    if (len >= (1ull << 40)) {
        set_err(err, "batch too large (%llu bytes)", (unsigned long long)len);
        return false;
    }
    if (out->mem != NXG_MEM_DEVICE || !mixed_capable(out) || !out->id)
        return refuse(err, "archive batches decode into device MIXED-layout columns");
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
    if (!out || !need_rows || !need_children || (n && (!recs || !info)) || (!dbuf && buf_len))
        return refuse(err, "null argument");
    if (out->mem != NXG_MEM_DEVICE || !mixed_capable(out) || !out->id || !out->fixed)
        return refuse(err, "a window of archive records decodes into device MIXED-layout columns");
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
    if (!c) return refuse(err, "null argument");
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if (buf_len && !is_device_ptr(dbuf))
        return refuse(err, "the window's buffer must be device memory");
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
    if (!window || !out) return refuse(err, "null argument");
    if (window->mem != NXG_MEM_DEVICE || window->layout != NXG_LAYOUT_MIXED || !window->id ||
        !window->tag || !window->fixed || !window->aux)
        return refuse(err, "the image is built from device MIXED-layout columns");
    const uint64_t rows = window->n_rows;
    if (out->cap_rows < std::min(n_ids, rows)) {
        set_err(err, "the image's capacity is %llu rows; min(n_ids, window rows) = %llu",
                (unsigned long long)out->cap_rows, (unsigned long long)std::min(n_ids, rows));
        return false;
    }
    if (out->cap_rows && (!out->id || !out->tag || !out->fixed || !out->aux || !out->src_row))
        return refuse(err, "null output array");
    if (!c) return refuse(err, "null argument");
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

// ---- a dispatch's entries as archive batch records (the recorder's batch loop, record.rs:307-347)
// (nxg_record.hip). Argument checks on the host, the launches, one read-back of the call's head.
bool nxg_record_entries(NxgCtx* c, const NxgColumns* batch, const uint8_t* heap,
                        const NxgDispatch* d, uint32_t n_chans, const NxgRecordTable* tab,
                        NxgRecordBatches* out, NetidxError* err) {
    if (!c || !batch || !d || !tab || !out || !d->chan_off || !out->rec_off ||
        (n_chans && !out->rec_items) || (tab->n_subs && !tab->arch_id_of_sub))
        return refuse(err, "null argument");
    const uint64_t ne = d->n_entries;
    const bool f64 = batch->layout == NXG_LAYOUT_F64;
    if (ne && (!d->ent_sub || !d->ent_row)) return refuse(err, "null entry array");
    if (batch->n_rows && (!batch->fixed || (!f64 && (!batch->tag || !batch->aux))))
        return refuse(err, "null batch column");
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
    if (batch->mem != NXG_MEM_DEVICE ||
        !all_device({d->chan_off, out->rec_off, n_chans ? out->rec_items : nullptr, out->out, heap,
                     tab->n_subs ? tab->arch_id_of_sub : nullptr, ne ? d->ent_sub : nullptr,
                     ne ? d->ent_row : nullptr, batch->n_rows ? batch->fixed : nullptr,
                     batch->n_rows && !f64 ? batch->tag : nullptr,
                     batch->n_rows && !f64 ? batch->aux : nullptr, kids ? batch->ctag : nullptr,
                     kids ? batch->cfixed : nullptr, kids ? batch->caux : nullptr})) {
        set_err(err, "nxg_record_entries takes device memory only (batch, heap, the dispatch's "
                     "arrays, tab->arch_id_of_sub, out->out, out->rec_off and out->rec_items)");
        return false;
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

// ---- the RecordIndex of an indexed archive (nxg_archive_index.hip): written per record
// (add_batch, writer.rs:407-429) and scanned by Id set (scan_index_at, reader.rs:394-422).
bool nxg_archive_index_records(NxgCtx* c, const uint64_t* key, uint64_t n_keys,
                               const uint64_t* seg_off, uint32_t n_recs, const NxgRecordTable* tab,
                               NxgArchiveIndexes* out, NetidxError* err) {
    // (every argument is looked at before the ctx, so that each refusal is reached without one)
    if (!seg_off) return refuse(err, "null argument (seg_off)");
    if (!out) return refuse(err, "null argument (out)");
    if (!out->idx_off) return refuse(err, "null argument (out->idx_off)");
    if (n_recs && !out->idx_ids) return refuse(err, "null argument (out->idx_ids)");
    if (n_keys && !key) return refuse(err, "null argument (key)");
    if (tab && tab->n_subs && !tab->arch_id_of_sub)
        return refuse(err, "null argument (tab->arch_id_of_sub)");
    if (n_keys > kAixMaxKeys) {
        set_err(err, "too many positions for one call (%llu)", (unsigned long long)n_keys);
        return false;
    }
    if (!c) return refuse(err, "null argument (ctx)");
    if (!all_device({seg_off, out->idx_off, n_recs ? out->idx_ids : nullptr, out->out,
                     n_keys ? key : nullptr,
                     tab && tab->n_subs ? tab->arch_id_of_sub : nullptr})) {
        set_err(err, "nxg_archive_index_records takes device memory only (key, seg_off, "
                     "tab->arch_id_of_sub, out->out, out->idx_off and out->idx_ids)");
        return false;
    }
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    out->n_bytes = out->n_ids_total = 0;
    if (n_keys == 0 || n_recs == 0) {  // no positions: no index, and no kernel runs
        HIPCHK(hipMemsetAsync(out->idx_off, 0, ((uint64_t)n_recs + 1) * 8, c->stream));
        if (n_recs) HIPCHK(hipMemsetAsync(out->idx_ids, 0, (uint64_t)n_recs * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return true;
    }
    NxgAixArgs a{};
    a.key = key;
    a.seg_off = seg_off;
    a.n_keys = n_keys;
    a.n_recs = n_recs;
    a.arch_id_of_sub = tab ? tab->arch_id_of_sub : nullptr;
    a.n_subs = tab ? tab->n_subs : 0;
    a.out = out->out;
    a.cap = out->out ? out->cap_bytes : 0;
    a.idx_off = out->idx_off;
    a.idx_ids = out->idx_ids;
    a.translate = tab != nullptr;  // (a table without entries drops every position)
    if (!ensure_dscratch(c, nxg_aix_scratch_bytes(n_keys, n_recs), err) ||
        !grow(c, c->aix_table, nxg_aix_table_bytes(nxg_aix_slot_bits(n_keys)), kGrowDouble, err))
        return false;
    NxgAixHead h;
    HIPCHK(nxg_launch_aix_index(a, c->dscratch, c->aix_table, c->stream));
    HIPCHK(hipMemcpyAsync(&h, c->dscratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.seg_bad) {
        set_err(err, "seg_off is not a list of records at record %u: it must not decrease and "
                     "must not end behind n_keys (%llu)", h.seg_bad - 1,
                (unsigned long long)n_keys);
        return false;
    }
    if (h.wide_inv) {
        const uint64_t p = ~h.wide_inv;
        uint64_t v = 0;
        HIPCHK(hipMemcpy(&v, key + p, 8, hipMemcpyDeviceToHost));
        set_err(err, "position %llu: Id %llu is not below 2^32", (unsigned long long)p,
                (unsigned long long)v);
        return false;
    }
    if (h.vec_bad) {
        set_err(err, "encode failed: record %u's Ids exceed MAX_VEC (PackError::TooBig)",
                h.vec_bad - 1);
        return false;
    }
    out->n_bytes = h.n_bytes;
    out->n_ids_total = h.n_ids;
    if (out->out && h.n_bytes > out->cap_bytes) {
        set_err(err, "output buffer too small: need %llu bytes, have %llu",
                (unsigned long long)h.n_bytes, (unsigned long long)out->cap_bytes);
        return false;
    }
    return true;
}

bool nxg_archive_scan_index(NxgCtx* c, const uint8_t* dbuf, uint64_t buf_len,
                            const uint64_t* idx_off, const uint64_t* idx_end, uint32_t n,
                            const uint8_t* keep, uint64_t n_ids, uint8_t* verdict,
                            uint64_t* n_match, NetidxError* err) {
    if (n && !dbuf) return refuse(err, "null argument (dbuf)");
    if (n && !idx_off) return refuse(err, "null argument (idx_off)");
    if (n && !idx_end) return refuse(err, "null argument (idx_end)");
    if (n && !verdict) return refuse(err, "null argument (verdict)");
    if (n_ids && !keep) return refuse(err, "null argument (keep)");
    for (uint32_t i = 0; i < n; i++)
        if (idx_off[i] > idx_end[i] || idx_end[i] > buf_len) {
            set_err(err, "record %u: [%llu, %llu) is not a range of the buffer's %llu bytes", i,
                    (unsigned long long)idx_off[i], (unsigned long long)idx_end[i],
                    (unsigned long long)buf_len);
            return false;
        }
    if (!c) return refuse(err, "null argument (ctx)");
    if (!no_pending(c, err)) return false;
    if (!set_device(c, err)) return false;
    if ((n && !is_device_ptr(dbuf)) || (n_ids && !is_device_ptr(keep))) {
        set_err(err, "nxg_archive_scan_index takes a device buffer and a device keep array");
        return false;
    }
    if (n_match) *n_match = 0;
    if (n == 0) return true;
    // one staging copy up: off[n], end[n], pbase[n + 1], res[n] (all ones)
    const size_t words = 4 * (size_t)n + 1;
    if (!grow(c, c->aix_dev, words * 8, kGrowDouble, err) ||
        !grow(c, c->aix_host, words * 8, kGrowDouble, err))
        return false;
    uint64_t* h = reinterpret_cast<uint64_t*>(c->aix_host.get());
    uint64_t* d = reinterpret_cast<uint64_t*>(c->aix_dev.get());
    uint64_t pieces = 0;
    for (uint32_t i = 0; i < n; i++) {
        h[i] = idx_off[i];
        h[n + i] = idx_end[i];
        h[2 * (size_t)n + i] = pieces;
        pieces += nxg_aix_scan_pieces((uintptr_t)dbuf, idx_off[i], idx_end[i]);
        h[3 * (size_t)n + 1 + i] = ~0ull;
    }
    h[3 * (size_t)n] = pieces;
    HIPCHK(hipMemcpyAsync(d, h, words * 8, hipMemcpyHostToDevice, c->stream));
    unsigned long long* res = reinterpret_cast<unsigned long long*>(d + 3 * (size_t)n + 1);
    HIPCHK(nxg_launch_aix_scan(dbuf, d, d + n, d + 2 * (size_t)n, n, pieces, keep, n_ids, res,
                               c->stream));
    HIPCHK(hipMemcpyAsync(h, res, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint64_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        verdict[i] = h[i] == ~0ull ? NXG_INDEX_NONE : (uint8_t)(h[i] & 3);
        m += verdict[i] == NXG_INDEX_MATCH;
    }
    if (n_match) *n_match = m;
    return true;
}

// ---- playback: a decoded window (process_batch, session_shard.rs:196-245) or its image (reimage,
// session_shard.rs:375-409) as publisher update rows (nxg_replay.hip). Argument checks on the host,
// the launches, one read-back of the call's head; a second small launch and read-back only when a
// record missed.
static bool replay_out_ok(const NxgReplayRows* out, const char* what, NetidxError* err) {
    if (!out->rec_off || (out->cap_miss && !out->miss_row) ||
        (out->cap_rows && (!out->id || !out->tag || !out->fixed || !out->aux || !out->src_row)))
        return refuse(err, "null output array");
    if (!all_device({out->rec_off, out->cap_miss ? out->miss_row : nullptr,
                     out->cap_rows ? out->id : nullptr, out->cap_rows ? out->tag : nullptr,
                     out->cap_rows ? out->fixed : nullptr, out->cap_rows ? out->aux : nullptr,
                     out->cap_rows ? out->src_row : nullptr})) {
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
    if (!c || !window || !tab || !out || (n_recs && !info) || (tab->n_ids && !tab->pub_id_of_arch))
        return refuse(err, "null argument");
    if (window->mem != NXG_MEM_DEVICE || window->layout != NXG_LAYOUT_MIXED ||
        (window->n_rows && (!window->id || !window->tag || !window->fixed || !window->aux)))
        return refuse(err, "a window is replayed from device MIXED-layout columns");
    std::vector<uint64_t> hbeg, hend;
    if (!window_records(window, info, n_recs, &hbeg, &hend, err)) return false;
    const uint64_t first = hbeg[0], n = hbeg[n_recs] - first;
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
        (tab->n_ids && !tab->pub_id_of_arch))
        return refuse(err, "null argument");
    if (image->n_rows > image->cap_rows ||
        (image->n_rows && (!image->id || !image->tag || !image->fixed || !image->aux)))
        return refuse(err, "the image's arrays are null or n_rows exceeds cap_rows");
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

}  // extern "C"
