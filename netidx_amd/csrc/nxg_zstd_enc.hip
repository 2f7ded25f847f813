// nxg_zstd_enc.hip -- zstd compression of archive batch records on gfx950.
//
// Replaces compress_task of ArchiveReader::compress (netidx-archive/src/logfile/reader.rs:741-769):
// every record of an archive file compressed independently with the archive's dictionary. The
// reference runs ncpus * window libzstd jobs on host cores; here a wave compresses one record and
// a persistent grid takes many records per call (nxg_archive_compress), mirroring nxg_zstd_kernel;
// the waves draw records by a ticket, longest first, since records differ in length by orders of
// magnitude and each record's bytes do not depend on which wave compresses it.
//
// Per block (at most 128 KiB, RFC 8878 3.1.1.2):
//   a block of one repeated byte is an RLE block;
//   matches: the wave takes 64 positions per step. Each lane hashes the 4 bytes at its position,
//     reads the candidate of the record's own table (LDS, the record so far) and of the
//     dictionary content's table (global, built once per dictionary, read-only), and checks its 4
//     bytes. A ballot picks the earliest lane with a match; the wave extends it 64 bytes per
//     round. The positions the step covered are then inserted with an LDS atomic max, so the
//     greatest position wins a slot whatever the order the hardware serves the lanes in: the
//     table, and with it the output, is a function of the record and the dictionary alone;
//   literals go to the wave's literal buffer, sequences (offset, literals length, match length)
//     to its sequence buffer (a per-wave slab in global memory, read back with loads that bypass
//     the CU's L1, after the wave's stores are drained);
//   literals section: RLE, Huffman with the dictionary's tree (Treeless_Literals_Block; one
//     stream by lane 0 up to 1023 literals, else four streams by lanes 0..3, from literals the
//     wave stages in LDS) when every literal has a code and that is smaller, else raw. The streams' sizes follow from the code lengths'
//     sums, counted by the whole wave, so every stream's place is known before it is written;
//     With block trees (NxgZstdCompressOpts.literals = 1, the kernel's second instantiation) the
//     same pass takes the literals' histogram (LDS atomics); the wave sorts the counts, lane 0
//     builds code lengths of at most 11 bits, the codes and the tree's description
//     (nxg_zstd_enc.h), a second pass sums the streams' bits under them, and the block's own tree
//     (Compressed_Literals_Block) is one more candidate after raw, RLE and the treeless form with
//     the frame's live tree -- the dictionary's until a block of the frame writes its own;
//   sequences section: predefined distributions, FSE-encoded by lane 0 (nxg_zstd_enc.h);
//   a block whose compressed form is not smaller than its bytes is a raw block.
// Every store is bounded by the record's slot: the compressed form is written under a byte limit
// of the block's length - 1 and dropped for the raw block when it does not fit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "nxg_device.h"
#include "nxg_zstd_enc.h"

using namespace nxz;

// device-resident encode-side state of a dictionary
struct NxzEncDict {
    uint32_t id, content_len, has_tables, pad;
    const uint8_t* content;
    const uint32_t* table;  // hash of 4 content bytes -> the greatest index + 1 with that hash
    HufCode codes[256];
};
// one record: its batch in the staged source, its frame's slot; the result
struct NxzEncRec {
    uint64_t src_off, src_len, out_off, out_cap;
};
struct NxzEncRes {
    uint64_t out_len;
    uint32_t err, pad;
};

namespace {

constexpr uint32_t HBITS = 13;         // the record's table: 32 KiB of LDS
constexpr uint32_t DBITS = 15;         // the dictionary content's table: 128 KiB, L2-resident
constexpr uint32_t NSEQ_MAX = 32768;   // a block's most: 128 KiB of 4-byte matches
constexpr uint64_t SLAB = (uint64_t)kBlockMax + (uint64_t)NSEQ_MAX * 8;  // per wave

constexpr uint32_t HCH = 512;          // literals staged in LDS per Huffman stream and round

struct ELds {
    uint32_t ht[1u << HBITS];
    HufCode codes[256];
    uint8_t stage[4][HCH];
    EncTables enc;  // the predefined distributions' encoding tables, next to the lane that codes
};
// with block trees (kLitBlockTrees): `codes` is the frame's live tree; the tree build's working
// memory lies over the literal stage, which is idle until the streams are written; the block's
// own codes and weights take 1280 of the 2064 bytes ELds leaves of a quarter of the CU's LDS
struct ELdsTrees {
    uint32_t ht[1u << HBITS];
    HufCode codes[256];
    union {
        uint8_t stage[4][HCH];
        HufWork work;
    };
    EncTables enc;
    HufCode fresh[256];
    uint8_t w[256];
};
static_assert(sizeof(ELdsTrees) == sizeof(ELds) + 1280, "the stage and the tree build share");
template <uint32_t MODE>
struct LdsOf {
    using T = ELds;
};
template <>
struct LdsOf<kLitBlockTrees> {
    using T = ELdsTrees;
};

NXG_DEV uint32_t bcast(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
NXG_DEV uint8_t ldnt(const uint8_t* p) { return __builtin_nontemporal_load(p); }
NXG_DEV void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
NXG_DEV uint32_t rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the record being compressed and what lies before it
struct Src {
    const uint8_t* s;
    uint64_t n;
    const uint8_t* dc;  // dictionary content (null: none)
    uint32_t dl;
    const uint32_t* dt;
};
// the byte `off` before position k (a position before 0 is in the dictionary's content)
NXG_DEV uint32_t hist(const Src& S, uint64_t k, uint32_t off) {
    return k >= off ? S.s[k - off] : S.dc[S.dl - (uint32_t)(off - k)];
}

struct LdsB {
    NXG_DEV uint8_t operator()(const uint8_t* p) const { return *p; }
};
struct NtQ {
    NXG_DEV uint64_t operator()(const uint64_t* p) const { return __builtin_nontemporal_load(p); }
};

// src[0, len) -> dst, one byte per lane and round
template <bool NT>
NXG_DEV void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane) {
    for (uint32_t k = lane; k < len; k += 64) dst[k] = NT ? ldnt(src + k) : src[k];
}

// huf_sort_hist by the whole wave: a lane ranks its four symbols' keys among all 256 (the keys of
// present symbols are distinct, so the ranks are their places) and writes count and symbol there.
// Returns the present symbols.
NXG_DEV uint32_t sort_hist_wave(HufWork& W, uint32_t lane) {
    wave_lds_order();
    uint32_t key[4], rank[4] = {0, 0, 0, 0}, n = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t s = lane + 64 * j, c = W.hist[s];
        key[j] = c ? (c << 8) | s : ~0u;
        n += (uint32_t)__popcll(__ballot(c != 0));
    }
    for (uint32_t t = 0; t < 256; t++) {
        const uint32_t c = W.hist[t], kt = c ? (c << 8) | t : ~0u;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) rank[j] += kt < key[j] ? 1u : 0u;
    }
    wave_lds_order();  // the symbols' places lie over the counts: every lane has read them
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (key[j] != ~0u) {
            W.a[rank[j]] = key[j] >> 8;
            W.t.ord[rank[j]] = (uint8_t)key[j];
        }
    wave_lds_order();
    return n;
}

// The Huffman streams of a block's literals at `base`: ns = 1 (lane 0) or 4 (lanes 0..3, stream k
// = the literals [k * seg, ...)). A lane's loads from the literal buffer would each wait out a
// trip to L2, so the wave stages every stream's next HCH literals (from its end backwards, the
// order they are coded in) in LDS and the coding lanes read them there. True when every stream
// took exactly the bytes planned for it.
template <typename LT>
NXG_DEV bool huf_streams(LT& L, const HufCode* codes, uint8_t* base, const LitPlan& plan,
                         const uint8_t* lit, uint32_t nlit, uint32_t seg, uint32_t ns,
                         uint32_t lane) {
    uint32_t so = 0, sz = 0, cnt = 0;
    if (ns == 1) {
        sz = plan.ssz[0];
        cnt = nlit;
    } else if (lane < 4) {
        so = lane == 0 ? 0u
             : lane == 1 ? plan.ssz[0]
             : lane == 2 ? plan.ssz[0] + plan.ssz[1]
                         : plan.ssz[0] + plan.ssz[1] + plan.ssz[2];
        sz = lane == 0 ? plan.ssz[0] : lane == 1 ? plan.ssz[1] : lane == 2 ? plan.ssz[2] : plan.ssz[3];
        cnt = lane < 3 ? seg : nlit - 3 * seg;
    }
    const bool coder = lane < ns;
    BitW w(base + so, coder ? sz : 0u);
    const uint32_t longest = ns == 1 ? nlit : seg;
    for (uint32_t done = 0; done < longest; done += HCH) {
        wave_lds_order();
        for (uint32_t k = 0; k < ns; k++) {
            const uint32_t ck = ns == 1 ? nlit : (k < 3 ? seg : nlit - 3 * seg);
            if (done >= ck) continue;
            const uint32_t take = min(HCH, ck - done);
            const uint8_t* s = lit + k * seg + (ck - done - take);
            for (uint32_t j = lane; j < take; j += 64) L.stage[k][j] = ldnt(s + j);
        }
        wave_lds_order();
        if (coder && done < cnt) huf_put(w, &L.stage[lane][0], min(HCH, cnt - done), codes, LdsB{});
    }
    wave_lds_order();
    bool ok = true;
    if (coder) ok = w.close() == sz;
    return !__any(!ok);
}

// One block [b0, b1) of the record at dst (its 3-byte header first); returns the bytes written.
// `room` >= 3 + (b1 - b0) bytes are the caller's to give. `coded_dict`: L.codes holds a tree the
// frame's reader has (the dictionary's; with block trees the live one, which a block that writes
// its own tree replaces).
template <uint32_t MODE>
NXG_DEV uint32_t compress_block(typename LdsOf<MODE>::T& L, const Src& S, uint64_t b0, uint64_t b1,
                                bool& coded_dict, const EncTables* T, uint8_t* dst, uint8_t* lit,
                                uint64_t* seqs, bool last, uint32_t lane) {
    const uint32_t blen = (uint32_t)(b1 - b0);
    const uint8_t* blk = S.s + b0;
    // ---- one repeated byte: an RLE block
    {
        const uint32_t first = blk[0];
        bool same = true;
        for (uint32_t k = 0; k < blen; k += 64) {
            const uint32_t i = k + lane;
            if (__any(i < blen && blk[i] != first)) {
                same = false;
                break;
            }
        }
        if (same) {
            if (lane == 0) {
                write_block_header(dst, 1, blen, last);
                dst[3] = (uint8_t)first;
            }
            return 4;
        }
    }
    // ---- matches
    uint64_t p = b0, anchor = b0;
    uint32_t nseq = 0, nlit = 0;
    while (p + kMinMatch <= b1 && nseq < NSEQ_MAX) {
        const uint64_t i = p + lane;
        const bool valid = i + 4 <= b1;
        uint32_t v = 0, h = 0, cr = 0, cd = 0;
        if (valid) {
            v = rd32(S.s + i);
            h = hash4(v, HBITS);
            cr = L.ht[h];
            if (S.dt) cd = S.dt[hash4(v, DBITS)];
        }
        uint32_t off = 0;
        if (cr) {  // a position of the record, inserted by an earlier step: below p
            const uint64_t q = cr - 1;
            if (q < i && i - q <= kOffMax && rd32(S.s + q) == v) off = (uint32_t)(i - q);
        }
        if (!off && cd) {  // content index j, j + 4 <= dl
            const uint32_t j = cd - 1;
            const uint64_t d = i + (S.dl - j);
            if (d <= kOffMax && rd32(S.dc + j) == v) off = (uint32_t)d;
        }
        const uint64_t m = __ballot(off != 0);
        uint64_t next = p + 64;
        uint64_t ms = 0;
        uint32_t len = 0, o = 0;
        if (m) {
            const uint32_t first = (uint32_t)__builtin_ctzll(m);
            ms = p + first;
            o = (uint32_t)__shfl((int)off, (int)first);
            len = kMinMatch;
            for (;;) {  // 64 bytes per round; ends at the block's end at the latest
                const uint64_t k = ms + len + lane;
                bool eq = false;
                if (k < b1) eq = S.s[k] == hist(S, k, o);
                const uint64_t mm = __ballot(!eq);
                if (mm) {
                    len += (uint32_t)__builtin_ctzll(mm);
                    break;
                }
                len += 64;
            }
            next = ms + len;
        }
        // the positions this step covered enter the table: the greatest position wins a slot
        wave_lds_order();
        if (valid && i < next) atomicMax(&L.ht[h], (uint32_t)i + 1);
        wave_lds_order();
        if (m) {
            const uint32_t ll = (uint32_t)(ms - anchor);
            copy_bytes<false>(lit + nlit, S.s + anchor, ll, lane);
            if (lane == 0) seqs[nseq] = seq_pack(o, ll, len);
            nlit += ll;
            nseq++;
            anchor = next;
        }
        p = next;
    }
    {
        const uint32_t ll = (uint32_t)(b1 - anchor);
        copy_bytes<false>(lit + nlit, S.s + anchor, ll, lane);
        nlit += ll;
    }
    drain();  // the literal and sequence buffers are read back below
    // ---- the literals: one byte repeated? every one coded? the code lengths' sums per stream
    const bool four = nlit >= 1024;
    const uint32_t seg = four ? (nlit + 3) / 4 : (nlit ? nlit : 1u);
    uint32_t bsum0 = 0, bsum1 = 0, bsum2 = 0, bsum3 = 0;
    bool same = true, coded = coded_dict;
    const uint32_t lit0 = nlit ? ldnt(lit) : 0u;
    if constexpr (MODE == kLitBlockTrees) {  // the literals' histogram, taken in the same pass
        for (uint32_t i = lane; i < 256; i += 64) L.work.hist[i] = 0;
        wave_lds_order();
    }
    for (uint32_t i = lane; i < nlit; i += 64) {
        const uint32_t b = ldnt(lit + i);
        same &= b == lit0;
        if constexpr (MODE == kLitBlockTrees) atomicAdd(&L.work.hist[b], 1u);
        if (coded_dict) {
            const uint32_t nb = L.codes[b].nbits;
            coded &= nb != 0;
            const uint32_t k = i / seg;
            bsum0 += k == 0 ? nb : 0u;
            bsum1 += k == 1 ? nb : 0u;
            bsum2 += k == 2 ? nb : 0u;
            bsum3 += k == 3 ? nb : 0u;
        }
    }
    same = !__any(!same);
    coded = !__any(!coded);
    uint64_t bits[4] = {wave_sum<uint32_t>(bsum0), wave_sum<uint32_t>(bsum1),
                        wave_sum<uint32_t>(bsum2), wave_sum<uint32_t>(bsum3)};
    LitPlan plan;
    bool fresh = false;  // the literals take the block's own tree
    uint32_t dsz = 0;    // its description's bytes (L.work.t.desc)
    const HufCode* codes = L.codes;
    if constexpr (MODE == kLitBlockTrees) {
        uint64_t fbits[4] = {0, 0, 0, 0};
        if (!same && nlit >= kFreshMinLits) {
            const uint32_t nsym = sort_hist_wave(L.work, lane);  // >= 2: the literals differ
            if (lane == 0) {  // <= 256 symbols, serial: lengths, codes, description
                uint32_t ns = 0, mb = 0;
                huf_build_weights(L.work, nsym, L.w, &ns, &mb);
                build_huf_enc_ws(L.fresh, L.w, ns, mb, L.work.a, L.work.a + kHufMaxBits + 2);
                dsz = write_huf_desc(L.work, L.w, ns);
            }
            dsz = bcast(dsz);
            wave_lds_order();
            if (dsz) {  // the streams' bits under the block's own codes: a second pass
                uint32_t f0 = 0, f1 = 0, f2 = 0, f3 = 0;
                for (uint32_t i = lane; i < nlit; i += 64) {
                    const uint32_t nb = L.fresh[ldnt(lit + i)].nbits;
                    const uint32_t k = i / seg;
                    f0 += k == 0 ? nb : 0u;
                    f1 += k == 1 ? nb : 0u;
                    f2 += k == 2 ? nb : 0u;
                    f3 += k == 3 ? nb : 0u;
                }
                fbits[0] = wave_sum<uint32_t>(f0);
                fbits[1] = wave_sum<uint32_t>(f1);
                fbits[2] = wave_sum<uint32_t>(f2);
                fbits[3] = wave_sum<uint32_t>(f3);
            }
        }
        plan = plan_literals_trees(nlit, same, coded, bits, dsz != 0, fbits, dsz, &fresh);
        if (fresh) codes = L.fresh;
    } else {
        plan = plan_literals(nlit, same, coded, bits);
    }
    // ---- the compressed form, under blen - 1 bytes; else the raw block
    uint32_t body = 0;  // 0: raw
    if ((uint64_t)plan.size + 1 <= blen - 1) {
        uint8_t* lp = dst + 3;
        uint32_t at = 0;
        if constexpr (MODE == kLitBlockTrees) {
            if (lane == 0)
                at = write_lit_header_trees(lp, plan, nlit, lit0, fresh, L.work.t.desc, dsz);
            wave_lds_order();  // the description is out before the stage takes its bytes
        } else {
            if (lane == 0) at = write_lit_header(lp, plan, nlit, lit0);
        }
        at = bcast(at);
        bool ok = true;
        if (plan.mode == LIT_RAW) {
            copy_bytes<true>(lp + at, lit, nlit, lane);
        } else if (plan.mode == LIT_HUF1) {
            ok = huf_streams(L, codes, lp + at, plan, lit, nlit, seg, 1, lane);
        } else if (plan.mode == LIT_HUF4) {
            ok = huf_streams(L, codes, lp + at, plan, lit, nlit, seg, 4, lane);
        }
        ok = !__any(!ok);
        if (ok) {
            if (nseq == 0) {
                if (lane == 0) lp[plan.size] = 0;  // Number_of_Sequences 0
                body = plan.size + 1;
            } else {
                uint32_t r = 0;
                if (lane == 0)
                    r = encode_sequences(lp + plan.size, blen - 1 - plan.size, seqs, nseq, T, NtQ{});
                r = bcast(r);
                if (r) body = plan.size + r;
            }
        }
    }
    if (body) {
        if (lane == 0) write_block_header(dst, 2, body, last);
        if constexpr (MODE == kLitBlockTrees) {
            if (fresh) {  // the reader's tree from here on, until a block writes another
                wave_lds_order();
                for (uint32_t i = lane; i < 256; i += 64) L.codes[i] = L.fresh[i];
                wave_lds_order();
                coded_dict = true;
            }
        }
        return 3 + body;
    }
    drain();  // lane 0's stores of the dropped form land before the raw bytes
    if (lane == 0) write_block_header(dst, 0, blen, last);
    copy_bytes<false>(dst + 3, blk, blen, lane);
    return 3 + blen;
}

// MODE: NxgZstdCompressOpts.literals (kLitDictTree: the dictionary's tree only; kLitBlockTrees:
// a block may write its own)
template <uint32_t MODE>
__global__ __launch_bounds__(64) void nxg_zstd_enc_kernel(const uint8_t* __restrict__ src,
                                                          const NxzEncRec* __restrict__ recs,
                                                          uint32_t n, const NxzEncDict* dict,
                                                          const EncTables* T, uint8_t* out,
                                                          uint8_t* slab, NxzEncRes* res,
                                                          const uint32_t* __restrict__ order,
                                                          uint32_t* ticket) {
    __shared__ __attribute__((aligned(16))) typename LdsOf<MODE>::T L;
    const uint32_t lane = threadIdx.x;
    uint8_t* lit = slab + (uint64_t)blockIdx.x * SLAB;
    uint64_t* seqs = reinterpret_cast<uint64_t*>(lit + kBlockMax);
    const bool coded_dict = dict && dict->has_tables;
    if (coded_dict)
        for (uint32_t i = lane; i < 256; i += 64) L.codes[i] = dict->codes[i];
    {
        static_assert(sizeof(EncTables) % 4 == 0, "copied by words");
        const uint32_t* ts = reinterpret_cast<const uint32_t*>(T);
        uint32_t* td = reinterpret_cast<uint32_t*>(&L.enc);
        for (uint32_t i = lane; i < sizeof(EncTables) / 4; i += 64) td[i] = ts[i];
    }
    wave_lds_order();
    // records are handed out by a ticket, longest first (`order`, sorted on the host): a wave
    // that drew a two-block record does not also own a fixed share of the rest
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1u);
        t = bcast(t);
        if (t >= n) break;
        const uint32_t r = order[t];
        const NxzEncRec rc = recs[r];
        if (rc.out_cap < frame_bound(rc.src_len)) continue;  // rejected on the host: no slot
        for (uint32_t i = lane; i < (1u << HBITS); i += 64) L.ht[i] = 0;
        wave_lds_order();
        Src S{src + rc.src_off, rc.src_len, dict ? dict->content : nullptr,
              dict ? dict->content_len : 0u, dict ? dict->table : nullptr};
        uint8_t* dst = out + rc.out_off;
        uint32_t hl = 0;
        if (lane == 0) hl = write_frame_header(dst, S.n, dict ? dict->id : 0u);
        uint64_t op = bcast(hl);
        if (S.n == 0) {
            if (lane == 0) write_block_header(dst + op, 0, 0, true);
            op += 3;
        }
        bool live = coded_dict;  // a frame starts from the dictionary's tree, or none
        if constexpr (MODE == kLitBlockTrees) {  // the last frame may have left its own in L.codes
            if (coded_dict) {
                for (uint32_t i = lane; i < 256; i += 64) L.codes[i] = dict->codes[i];
                wave_lds_order();
            }
        }
        for (uint64_t b0 = 0; b0 < S.n; b0 += kBlockMax) {
            const uint64_t b1 = S.n - b0 > kBlockMax ? b0 + kBlockMax : S.n;
            op += compress_block<MODE>(L, S, b0, b1, live, &L.enc, dst + op, lit, seqs, b1 == S.n,
                                       lane);
        }
        if (lane == 0) res[r] = NxzEncRes{op, 0, 0};
        wave_lds_order();
    }
}

// the dictionary content's table: index j + 1 of the greatest j with the hash (atomic max: the
// result does not depend on the order of the threads)
__global__ __launch_bounds__(256) void nxg_zstd_dict_hash_kernel(const uint8_t* dc, uint32_t dl,
                                                                 uint32_t* tab) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (dl >= 4 && j <= dl - 4) atomicMax(&tab[hash4(rd32(dc + j), DBITS)], j + 1);
}

// the frames from their slots to one run of bytes: dst[pk[r], + res[r].out_len)
__global__ __launch_bounds__(256) void nxg_zstd_pack_kernel(const uint8_t* __restrict__ out,
                                                            const NxzEncRec* __restrict__ recs,
                                                            const NxzEncRes* __restrict__ res,
                                                            const uint64_t* __restrict__ pk,
                                                            uint32_t n, uint8_t* __restrict__ dst) {
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint64_t len = res[r].out_len;
        const uint8_t* s = out + recs[r].out_off;
        uint8_t* d = dst + pk[r];
        for (uint64_t k = threadIdx.x; k < len; k += 256) d[k] = s[k];
    }
}

struct PlainB {
    uint8_t operator()(const uint8_t* p) const { return *p; }
};
struct PlainQ {
    uint64_t operator()(const uint64_t* p) const { return *p; }
};

}  // namespace

// ---- host ---------------------------------------------------------------------------------
// the encode-side state of a dictionary (zstd format: the id and the Huffman codes from the
// weights; raw content: none), by the code the device runs (nxg_zstd_enc.h)
bool nxg_zstd_build_enc_dict(const uint8_t* d, uint64_t n, NxzEncDict* out) {
    memset(out, 0, sizeof *out);
    if (n < 8 || (uint32_t)(d[0] | d[1] << 8 | d[2] << 16 | (uint32_t)d[3] << 24) != kDictMagic)
        return true;
    out->id = (uint32_t)(d[4] | d[5] << 8 | d[6] << 16 | (uint32_t)d[7] << 24);
    uint8_t w[256];
    FseCell fse[64];
    int16_t norm[64];
    uint16_t next[64];
    uint32_t ns = 0, mb = 0;
    if (!read_huf_weights(d + 8, (uint32_t)(n - 8), w, &ns, &mb, fse, norm, next)) return false;
    build_huf_enc(out->codes, w, ns, mb);
    out->has_tables = 1;
    return true;
}
void nxg_zstd_enc_dict_set(NxzEncDict* d, const uint8_t* dcontent, uint32_t content_len,
                           const uint32_t* dtable) {
    d->content = dcontent;
    d->content_len = content_len;
    d->table = dtable;
}
bool nxg_zstd_build_enc_tables(void* o) { return build_enc_defaults(static_cast<EncTables*>(o)); }
uint64_t nxg_zstd_enc_dict_bytes() { return sizeof(NxzEncDict); }
uint64_t nxg_zstd_enc_tables_bytes() { return sizeof(EncTables); }
uint64_t nxg_zstd_enc_rec_bytes() { return sizeof(NxzEncRec); }
uint64_t nxg_zstd_enc_res_bytes() { return sizeof(NxzEncRes); }
uint64_t nxg_zstd_enc_slab_bytes() { return SLAB; }
uint64_t nxg_zstd_dict_table_bytes() { return sizeof(uint32_t) << DBITS; }
uint64_t nxg_zstd_frame_bound(uint64_t len) { return frame_bound(len); }
int nxg_zstd_enc_grid(int ncu) {
    int occ = 0;
    // both instantiations hold four workgroups per CU (by LDS); the grid sizes the slab once
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, nxg_zstd_enc_kernel<kLitDictTree>, 64,
                                                     0) != hipSuccess)
        occ = 1;
    return std::min(4, std::max(1, occ)) * ncu;
}

hipError_t nxg_launch_zstd_dict_hash(const uint8_t* dcontent, uint32_t content_len, uint32_t* dtable,
                                     hipStream_t s) {
    hipError_t e = hipMemsetAsync(dtable, 0, nxg_zstd_dict_table_bytes(), s);
    if (e != hipSuccess || content_len < 4) return e;
    hipLaunchKernelGGL(nxg_zstd_dict_hash_kernel, dim3((content_len + 255) / 256), dim3(256), 0, s,
                       dcontent, content_len, dtable);
    return hipGetLastError();
}

hipError_t nxg_launch_zstd_enc(const uint8_t* dsrc, const void* drecs, uint32_t n,
                               const void* ddict, const void* dtables, uint8_t* dout,
                               uint8_t* dslab, void* dres, const uint32_t* dorder,
                               uint32_t* dticket, int grid, uint32_t literals, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (literals > kLitBlockTrees) return hipErrorInvalidValue;  // no kernel for it: an error
    const uint32_t g = (uint32_t)std::min<uint64_t>((uint64_t)grid, n);
    auto k = literals == kLitBlockTrees ? nxg_zstd_enc_kernel<kLitBlockTrees>
                                        : nxg_zstd_enc_kernel<kLitDictTree>;
    hipLaunchKernelGGL(k, dim3(g), dim3(64), 0, s, dsrc,
                       reinterpret_cast<const NxzEncRec*>(drecs), n,
                       reinterpret_cast<const NxzEncDict*>(ddict),
                       reinterpret_cast<const EncTables*>(dtables), dout, dslab,
                       reinterpret_cast<NxzEncRes*>(dres), dorder, dticket);
    return hipGetLastError();
}

hipError_t nxg_launch_zstd_pack(const uint8_t* dout, const void* drecs, const void* dres,
                                const uint64_t* dpk, uint32_t n, uint8_t* dpacked, int ncu,
                                hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (uint32_t)std::min<uint64_t>((uint64_t)ncu * 8, n);
    hipLaunchKernelGGL(nxg_zstd_pack_kernel, dim3(g), dim3(256), 0, s, dout,
                       reinterpret_cast<const NxzEncRec*>(drecs),
                       reinterpret_cast<const NxzEncRes*>(dres), dpk, n, dpacked);
    return hipGetLastError();
}

// Not part of the ABI (tests, host only, no GPU): one frame of src[0, n) by the format code the
// device runs (nxg_zstd_enc.h: tables, headers, literals, sequences) behind a serial greedy
// matcher with the device's hash and tables' rules (the greatest position wins a slot). `dict`
// may be null. Returns the frame's bytes, 0 when `cap` is below nxg_zstd_frame_bound(n) or the
// dictionary does not parse. The device's parse differs (64 positions per step): its frames are
// pinned by tests/golden/zstd_gpu_records.bin.
static uint64_t compress_host(const uint8_t* dict, uint64_t dlen, const uint8_t* src, uint64_t n,
                              uint8_t* out, uint64_t cap, uint32_t literals) {
    if (cap < frame_bound(n) || n >= (1ull << 32) || literals > kLitBlockTrees) return 0;
    NxzEncDict ed;
    memset(&ed, 0, sizeof ed);
    const uint8_t* dc = nullptr;
    uint32_t dl = 0;
    if (dict) {
        if (!nxg_zstd_build_enc_dict(dict, dlen, &ed)) return 0;
        uint64_t coff = 0;
        if (ed.has_tables) {
            std::vector<uint8_t> dd(nxg_zstd_dict_dev_bytes());
            if (!nxg_zstd_build_dict(dict, dlen, reinterpret_cast<NxzDictDev*>(dd.data()), &coff))
                return 0;
        }
        dc = dict + coff;
        dl = (uint32_t)(dlen - coff);
    }
    EncTables T;
    if (!build_enc_defaults(&T)) return 0;
    std::vector<uint32_t> dt(1u << DBITS, 0), ht(1u << HBITS, 0);
    for (uint32_t j = 0; dl >= 4 && j <= dl - 4; j++) {
        uint32_t v;
        memcpy(&v, dc + j, 4);
        uint32_t& e = dt[hash4(v, DBITS)];
        e = std::max(e, j + 1);
    }
    uint64_t op = write_frame_header(out, n, ed.id);
    if (n == 0) {
        write_block_header(out + op, 0, 0, true);
        return op + 3;
    }
    std::vector<uint8_t> lit(kBlockMax);
    std::vector<uint64_t> seqs(NSEQ_MAX);
    bool live = ed.has_tables != 0;  // ed.codes is a tree the frame's reader has
    HufWork W;
    uint8_t fw[256];
    HufCode fcodes[256];
    auto hb = [&](uint64_t k, uint32_t off) -> uint8_t {
        return k >= off ? src[k - off] : dc[dl - (uint32_t)(off - k)];
    };
    for (uint64_t b0 = 0; b0 < n; b0 += kBlockMax) {
        const uint64_t b1 = std::min<uint64_t>(n, b0 + kBlockMax);
        const uint32_t blen = (uint32_t)(b1 - b0);
        const bool last = b1 == n;
        uint8_t* dst = out + op;
        bool same = true;
        for (uint64_t k = b0; k < b1 && same; k++) same = src[k] == src[b0];
        if (same) {
            write_block_header(dst, 1, blen, last);
            dst[3] = src[b0];
            op += 4;
            continue;
        }
        uint64_t p = b0, anchor = b0;
        uint32_t nseq = 0, nlit = 0;
        while (p + 4 <= b1 && nseq < NSEQ_MAX) {
            uint32_t v;
            memcpy(&v, src + p, 4);
            uint32_t& e = ht[hash4(v, HBITS)];
            uint32_t off = 0, w;
            if (e) {
                const uint64_t q = e - 1;
                memcpy(&w, src + q, 4);
                if (p - q <= kOffMax && w == v) off = (uint32_t)(p - q);
            }
            const uint32_t cd = dl ? dt[hash4(v, DBITS)] : 0;
            if (!off && cd) {
                memcpy(&w, dc + cd - 1, 4);
                const uint64_t d = p + (dl - (cd - 1));
                if (d <= kOffMax && w == v) off = (uint32_t)d;
            }
            e = (uint32_t)p + 1;
            if (!off) {
                p++;
                continue;
            }
            uint32_t len = 4;
            while (p + len < b1 && src[p + len] == hb(p + len, off)) len++;
            const uint32_t ll = (uint32_t)(p - anchor);
            memcpy(lit.data() + nlit, src + anchor, ll);
            seqs[nseq++] = seq_pack(off, ll, len);
            nlit += ll;
            p += len;
            anchor = p;
        }
        memcpy(lit.data() + nlit, src + anchor, b1 - anchor);
        nlit += (uint32_t)(b1 - anchor);
        const bool four = nlit >= 1024;
        const uint32_t seg = four ? (nlit + 3) / 4 : (nlit ? nlit : 1u);
        uint64_t bits[4] = {0, 0, 0, 0};
        bool lsame = true, coded = live;
        for (uint32_t i = 0; i < nlit; i++) {
            lsame &= lit[i] == lit[0];
            const uint32_t nb = ed.codes[lit[i]].nbits;
            coded &= nb != 0;
            bits[i / seg] += nb;
        }
        LitPlan plan;
        bool fresh = false;
        uint32_t dsz = 0;
        const HufCode* codes = ed.codes;  // the live tree
        if (literals == kLitBlockTrees) {
            uint64_t fbits[4] = {0, 0, 0, 0};
            if (!lsame && nlit >= kFreshMinLits) {
                memset(W.hist, 0, sizeof W.hist);
                for (uint32_t i = 0; i < nlit; i++) W.hist[lit[i]]++;
                const uint32_t nsym = huf_sort_hist(W);
                uint32_t ns = 0, mb = 0;
                huf_build_weights(W, nsym, fw, &ns, &mb);
                build_huf_enc_ws(fcodes, fw, ns, mb, W.a, W.a + kHufMaxBits + 2);
                dsz = write_huf_desc(W, fw, ns);
                for (uint32_t i = 0; dsz && i < nlit; i++) fbits[i / seg] += fcodes[lit[i]].nbits;
            }
            plan = plan_literals_trees(nlit, lsame, coded, bits, dsz != 0, fbits, dsz, &fresh);
            if (fresh) codes = fcodes;
        } else {
            plan = plan_literals(nlit, lsame, coded, bits);
        }
        uint32_t body = 0;
        if ((uint64_t)plan.size + 1 <= blen - 1) {
            uint8_t* lp = dst + 3;
            const uint32_t at = write_lit_header_trees(lp, plan, nlit, nlit ? lit[0] : 0, fresh,
                                                       W.t.desc, dsz);
            bool ok = true;
            if (plan.mode == LIT_RAW) {
                memcpy(lp + at, lit.data(), nlit);
            } else if (plan.mode == LIT_HUF1) {
                ok = huf_encode_stream(lp + at, plan.ssz[0], lit.data(), nlit, codes,
                                       PlainB{}) == plan.ssz[0];
            } else if (plan.mode == LIT_HUF4) {
                uint32_t so = 0;
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t c = k < 3 ? seg : nlit - 3 * seg;
                    ok &= huf_encode_stream(lp + at + so, plan.ssz[k], lit.data() + k * seg, c,
                                            codes, PlainB{}) == plan.ssz[k];
                    so += plan.ssz[k];
                }
            }
            if (ok && nseq == 0) {
                lp[plan.size] = 0;
                body = plan.size + 1;
            } else if (ok) {
                const uint32_t r = encode_sequences(lp + plan.size, blen - 1 - plan.size,
                                                    seqs.data(), nseq, &T, PlainQ{});
                if (r) body = plan.size + r;
            }
        }
        if (body) {
            write_block_header(dst, 2, body, last);
            op += 3 + body;
            if (fresh) {  // the frame's live tree from here on
                memcpy(ed.codes, fcodes, sizeof fcodes);
                live = true;
            }
        } else {
            write_block_header(dst, 0, blen, last);
            memcpy(dst + 3, src + b0, blen);
            op += 3 + blen;
        }
    }
    return op;
}
extern "C" uint64_t nxg_debug_zstd_compress_host(const uint8_t* dict, uint64_t dlen,
                                                 const uint8_t* src, uint64_t n, uint8_t* out,
                                                 uint64_t cap) {
    return compress_host(dict, dlen, src, n, out, cap, kLitDictTree);
}
// the same with NxgZstdCompressOpts.literals (0 also for a value the library does not know)
extern "C" uint64_t nxg_debug_zstd_compress_host_opts(const uint8_t* dict, uint64_t dlen,
                                                      const uint8_t* src, uint64_t n,
                                                      uint32_t literals, uint8_t* out,
                                                      uint64_t cap) {
    return compress_host(dict, dlen, src, n, out, cap, literals);
}

// Not part of the ABI (tests, host only, no GPU): the code builder and the tree description
// writer of a block's own Huffman tree (nxg_zstd_enc.h), as the device and the host-only encoder
// run them. huf_weights: a 256-entry histogram -> w[256] (0: absent); returns the symbols listed
// (the last present symbol + 1; 0 when fewer than two symbols are present), *max_bits the longest
// code. huf_desc: the weights of n_sym symbols -> the description at out (at least 132 bytes);
// returns its bytes, 0 when no form can describe the tree.
extern "C" uint32_t nxg_debug_zstd_huf_weights(const uint32_t* hist, uint8_t* w,
                                               uint32_t* max_bits) {
    HufWork W;
    uint64_t total = 0;
    for (uint32_t s = 0; s < 256; s++) total += hist[s];
    if (total > kBlockMax) return 0;  // a block's literals: the sort's keys hold 24-bit counts
    memcpy(W.hist, hist, sizeof W.hist);
    const uint32_t n = huf_sort_hist(W);
    if (n < 2) return 0;
    uint32_t ns = 0;
    huf_build_weights(W, n, w, &ns, max_bits);
    return ns;
}
extern "C" uint32_t nxg_debug_zstd_huf_desc(const uint8_t* w, uint32_t n_sym, uint8_t* out) {
    if (n_sym < 2 || n_sym > 256) return 0;
    for (uint32_t i = 0; i < n_sym; i++)
        if (w[i] > kHufEncBits) return 0;
    HufWork W;
    const uint32_t n = write_huf_desc(W, w, n_sym);
    memcpy(out, W.t.desc, n);
    return n;
}

// Not part of the ABI (tests, host only, no GPU): one frame (no dictionary) of one compressed
// block made of the given literals (raw) and sequences, by encode_sequences: the sequences
// section's count forms and bitstream against libzstd, for counts no matcher reaches on small
// inputs. Returns the frame's bytes, 0 when they do not fit or an argument is out of range.
extern "C" uint64_t nxg_debug_zstd_encode_seqs(const uint8_t* lits, uint32_t nlit,
                                               const uint32_t* off, const uint32_t* ll,
                                               const uint32_t* ml, uint32_t nseq,
                                               uint64_t content_size, uint8_t* out, uint64_t cap) {
    if (nseq == 0 || nlit > kBlockMax || content_size > kBlockMax || cap < kFrameHdrMax + 3 + 3)
        return 0;
    std::vector<uint64_t> seqs(nseq);
    for (uint32_t i = 0; i < nseq; i++) {
        if (off[i] == 0 || off[i] > kOffMax || ml[i] < 3 || ml[i] > kBlockMax || ll[i] > kBlockMax)
            return 0;
        seqs[i] = seq_pack(off[i], ll[i], ml[i]);
    }
    EncTables T;
    if (!build_enc_defaults(&T)) return 0;
    uint64_t op = write_frame_header(out, content_size, 0);
    uint8_t* body = out + op + 3;
    const uint64_t room = std::min<uint64_t>(cap - op - 3, kBlockMax - 1);
    LitPlan plan{};
    plan.mode = LIT_RAW;
    plan.hdr = raw_lit_hdr(nlit);
    plan.size = plan.hdr + nlit;
    if (plan.size + 5 > room) return 0;
    const uint32_t at = write_lit_header(body, plan, nlit, 0);
    memcpy(body + at, lits, nlit);
    const uint32_t r = encode_sequences(body + plan.size, (uint32_t)(room - plan.size), seqs.data(),
                                        nseq, &T, PlainQ{});
    if (!r) return 0;
    write_block_header(out + op, 2, plan.size + r, true);
    return op + 3 + plan.size + r;
}
