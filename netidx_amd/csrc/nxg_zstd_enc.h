// nxg_zstd_enc.h -- the encode side of the zstd format (RFC 8878), shared by the host (the
// dictionary's and the predefined distributions' encoding tables) and the gfx950 compressor of
// archive batch records (nxg_zstd_enc.hip).
//
// The reference compresses a record with zstd::bulk::Compressor::with_dictionary(19, dict)
// (netidx-archive/src/logfile/reader.rs:741-769). The format restated here:
//   frame header as ZSTD_writeFrameHeader emits it for a one-shot call  RFC 8878 3.1.1.1
//   literals-length / match-length / offset codes                       3.1.1.3.2.1.1 (ZSTD_LLcode,
//                                                                       ZSTD_MLcode, ZSTD_highbit32)
//   FSE encoding tables and the backward bitstream                      4.1 (FSE_buildCTable,
//                                                                       FSE_encodeSymbol, BIT_addBits)
//   the sequences section, predefined distributions                     3.1.1.3.2 (ZSTD_encodeSequences)
//   Huffman codes from weights, 1 / 4 streams                           4.2 (HUF_compress1X / 4X)
//   literals section headers                                            3.1.1.3.1
//   a block's own Huffman tree: length-limited code lengths, the tree's   4.2.1 (HUF_buildCTable,
//   description as direct or FSE-compressed weights                      HUF_writeCTable)
// Functions are pure (no memory outside their arguments). Loads of bytes the caller produced
// itself go through a `Ld` functor: the device reads its own per-wave buffers with loads that
// bypass the CU's L1, the host with plain loads.
#pragma once
#include "nxg_zstd.h"

namespace nxz {

// a sequence as the matcher leaves it: offset (29 bits) | literals length (17) | match length - 3
// (17). A block has at most 128 KiB, a match at least 4 bytes, an offset at most kOffMax.
constexpr uint32_t kOffMax = 1u << 28;  // offset + 3 < 2^29: code <= 28, the predefined table's last
constexpr uint32_t kMinMatch = 4;
NXZ_HD uint64_t seq_pack(uint32_t off, uint32_t ll, uint32_t ml) {
    return (uint64_t)off | ((uint64_t)ll << 29) | ((uint64_t)(ml - 3) << 46);
}
NXZ_HD uint32_t seq_off(uint64_t s) { return (uint32_t)s & ((1u << 29) - 1); }
NXZ_HD uint32_t seq_ll(uint64_t s) { return (uint32_t)(s >> 29) & ((1u << 17) - 1); }
NXZ_HD uint32_t seq_ml(uint64_t s) { return (uint32_t)(s >> 46) + 3; }

// value -> code (the inverse of ll_base / ml_base)
NXZ_HD uint32_t ll_code(uint32_t ll) {
    if (ll < 16) return ll;
    if (ll < 24) return 16 + ((ll - 16) >> 1);
    if (ll < 32) return 20 + ((ll - 24) >> 2);
    if (ll < 48) return 22 + ((ll - 32) >> 3);
    if (ll < 64) return 24;
    return highbit(ll) + 19;
}
NXZ_HD uint32_t ml_code(uint32_t ml) {  // ml >= 3
    const uint32_t b = ml - 3;
    if (b < 32) return b;
    if (b < 40) return 32 + ((b - 32) >> 1);
    if (b < 48) return 36 + ((b - 40) >> 2);
    if (b < 64) return 38 + ((b - 48) >> 3);
    if (b < 96) return 40 + ((b - 64) >> 4);
    if (b < 128) return 42;
    return highbit(b) + 36;
}

// ---- FSE encoding tables (FSE_buildCTable) --------------------------------------------------
struct FseSym {
    int32_t find;  // deltaFindState
    uint32_t nb;   // deltaNbBits
};
// `state` has 1 << al entries, `tt` max_sym + 1. Scratch: `cumul` max_sym + 2 u16, `tsym` 1 << al
// bytes. False on a malformed distribution.
NXZ_HD bool build_fse_enc(uint16_t* state, FseSym* tt, const int16_t* norm, uint32_t max_sym,
                          uint32_t al, uint16_t* cumul, uint8_t* tsym) {
    const uint32_t size = 1u << al;
    uint32_t high = size - 1;
    cumul[0] = 0;
    for (uint32_t s = 0; s <= max_sym; s++) {
        if (norm[s] == -1) {
            cumul[s + 1] = (uint16_t)(cumul[s] + 1);
            tsym[high--] = (uint8_t)s;
        } else {
            cumul[s + 1] = (uint16_t)(cumul[s] + (norm[s] > 0 ? norm[s] : 0));
        }
    }
    if (cumul[max_sym + 1] != size) return false;
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t pos = 0;
    for (uint32_t s = 0; s <= max_sym; s++)
        for (int i = 0; i < norm[s]; i++) {
            tsym[pos] = (uint8_t)s;
            do {
                pos = (pos + step) & mask;
            } while (pos > high);
        }
    if (pos != 0) return false;
    for (uint32_t u = 0; u < size; u++) state[cumul[tsym[u]]++] = (uint16_t)(size + u);
    uint32_t total = 0;
    for (uint32_t s = 0; s <= max_sym; s++) {
        const int n = norm[s];
        if (n == 0) {
            tt[s].nb = ((al + 1) << 16) - size;
            tt[s].find = 0;
        } else if (n == -1 || n == 1) {
            tt[s].nb = (al << 16) - size;
            tt[s].find = (int32_t)total - 1;
            total++;
        } else {
            const uint32_t max_out = al - highbit((uint32_t)n - 1);
            tt[s].nb = (max_out << 16) - ((uint32_t)n << max_out);
            tt[s].find = (int32_t)total - n;
            total += (uint32_t)n;
        }
    }
    return true;
}

// the predefined distributions' encoding tables (Compression_Mode 0 for all three)
struct EncTables {
    uint16_t ll_state[64], ml_state[64], of_state[32];
    FseSym ll[kLLMax + 1], ml[kMLMax + 1], of[29];
};
NXZ_HD bool build_enc_defaults(EncTables* t) {
    int16_t norm[64];
    uint16_t cumul[66];
    uint8_t tsym[64];
    for (int s = 0; s < 36; s++) norm[s] = kLLDefault[s];
    if (!build_fse_enc(t->ll_state, t->ll, norm, 35, 6, cumul, tsym)) return false;
    for (int s = 0; s < 53; s++) norm[s] = kMLDefault[s];
    if (!build_fse_enc(t->ml_state, t->ml, norm, 52, 6, cumul, tsym)) return false;
    for (int s = 0; s < 29; s++) norm[s] = kOFDefault[s];
    return build_fse_enc(t->of_state, t->of, norm, 28, 5, cumul, tsym);
}

// ---- Huffman codes from weights ---------------------------------------------------------------
// The code of symbol s is the index of its first cell in build_huf's decoding table without the
// bits a shorter code leaves free: weights in increasing order, symbols in order within a weight.
struct HufCode {
    uint16_t code;
    uint8_t nbits;  // 0: the symbol has no code
    uint8_t pad;
};
// `start`, `cnt`: kHufMaxBits + 2 words of scratch each
NXZ_HD void build_huf_enc_ws(HufCode* codes, const uint8_t* w, uint32_t n_sym, uint32_t max_bits,
                             uint32_t* start, uint32_t* cnt) {
    for (uint32_t k = 0; k < kHufMaxBits + 2; k++) start[k] = cnt[k] = 0;
    for (uint32_t s = 0; s < n_sym; s++) cnt[w[s]]++;
    uint32_t acc = 0;
    for (uint32_t k = 1; k <= max_bits; k++) {
        start[k] = acc;
        acc += cnt[k] << (k - 1);
    }
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t k = s < n_sym ? w[s] : 0;
        if (!k) {
            codes[s] = HufCode{0, 0, 0};
            continue;
        }
        codes[s] = HufCode{(uint16_t)(start[k] >> (k - 1)), (uint8_t)(max_bits + 1 - k), 0};
        start[k] += 1u << (k - 1);
    }
}
NXZ_HD void build_huf_enc(HufCode* codes, const uint8_t* w, uint32_t n_sym, uint32_t max_bits) {
    uint32_t start[kHufMaxBits + 2], cnt[kHufMaxBits + 2];
    build_huf_enc_ws(codes, w, n_sym, max_bits, start, cnt);
}

// ---- the backward bitstream, written forwards (BIT_CStream_t) -----------------------------------
// Bits are appended from bit 0 up; the reader starts from the closing marker bit of the last byte.
// A write past `cap` sets `ovf` and is dropped.
struct BitW {
    uint8_t* p;
    uint32_t cap, n = 0, nb = 0;
    uint64_t acc = 0;
    bool ovf = false;
    NXZ_HD BitW(uint8_t* p_, uint32_t cap_) : p(p_), cap(cap_) {}
    NXZ_HD void add(uint32_t v, uint32_t k) {  // k <= 32, nb + k <= 64 (flush in between)
        if (k == 0) return;
        acc |= ((uint64_t)v & ((1ull << k) - 1ull)) << nb;
        nb += k;
    }
    NXZ_HD void flush() {
        while (nb >= 8) {
            if (n < cap) p[n] = (uint8_t)acc;
            else ovf = true;
            n++;
            acc >>= 8;
            nb -= 8;
        }
    }
    NXZ_HD uint32_t close() {  // the marker bit, zero padding; the bytes written (0: overflow)
        add(1, 1);
        flush();
        if (nb) {
            if (n < cap) p[n] = (uint8_t)acc;
            else ovf = true;
            n++;
            nb = 0;
        }
        return ovf ? 0u : n;
    }
};

NXZ_HD void fse_init(uint32_t& st, const FseSym* tt, const uint16_t* tab, uint32_t sym) {
    const uint32_t nb = (tt[sym].nb + (1u << 15)) >> 16;
    const uint32_t value = (nb << 16) - tt[sym].nb;
    st = tab[(int32_t)(value >> nb) + tt[sym].find];
}
NXZ_HD void fse_put(BitW& w, uint32_t& st, const FseSym* tt, const uint16_t* tab, uint32_t sym) {
    const uint32_t nb = (st + tt[sym].nb) >> 16;
    w.add(st, nb);
    st = tab[(int32_t)(st >> nb) + tt[sym].find];
}

// The sequences section of `nseq` >= 1 sequences at dst: the count, the modes byte (all
// predefined) and the bitstream, last sequence first (ZSTD_encodeSequences). Returns the bytes
// written, 0 when they do not fit in `cap`.
template <typename Ld>
NXZ_HD uint32_t encode_sequences(uint8_t* dst, uint32_t cap, const uint64_t* seqs, uint32_t nseq,
                                 const EncTables* T, Ld ld) {
    if (cap < 5) return 0;
    uint32_t h;
    if (nseq < 128) {
        dst[0] = (uint8_t)nseq;
        h = 1;
    } else if (nseq < 0x7F00) {
        dst[0] = (uint8_t)((nseq >> 8) + 128);
        dst[1] = (uint8_t)nseq;
        h = 2;
    } else {
        dst[0] = 255;
        dst[1] = (uint8_t)(nseq - 0x7F00);
        dst[2] = (uint8_t)((nseq - 0x7F00) >> 8);
        h = 3;
    }
    dst[h++] = 0;  // Literals_Lengths, Offsets, Match_Lengths: Predefined_Mode
    BitW w(dst + h, cap - h);
    uint64_t s = ld(seqs + (nseq - 1));
    uint32_t ofv = seq_off(s) + 3, ll = seq_ll(s), ml = seq_ml(s);
    uint32_t llc = ll_code(ll), mlc = ml_code(ml), ofc = highbit(ofv);
    uint32_t sll, sml, sof;
    fse_init(sml, T->ml, T->ml_state, mlc);
    fse_init(sof, T->of, T->of_state, ofc);
    fse_init(sll, T->ll, T->ll_state, llc);
    w.add(ll - ll_base(llc), ll_bits(llc));
    w.add(ml - ml_base(mlc), ml_bits(mlc));
    w.flush();
    w.add(ofv - (1u << ofc), ofc);
    w.flush();
    for (uint32_t i = nseq - 1; i-- > 0;) {
        s = ld(seqs + i);
        ofv = seq_off(s) + 3;
        ll = seq_ll(s);
        ml = seq_ml(s);
        llc = ll_code(ll);
        mlc = ml_code(ml);
        ofc = highbit(ofv);
        fse_put(w, sof, T->of, T->of_state, ofc);
        fse_put(w, sml, T->ml, T->ml_state, mlc);
        fse_put(w, sll, T->ll, T->ll_state, llc);
        w.add(ll - ll_base(llc), ll_bits(llc));
        w.add(ml - ml_base(mlc), ml_bits(mlc));
        w.flush();
        w.add(ofv - (1u << ofc), ofc);
        w.flush();
        if (w.ovf) return 0;
    }
    w.add(sml, 6);
    w.add(sof, 5);
    w.add(sll, 6);
    const uint32_t n = w.close();
    return n ? h + n : 0u;
}

// ---- literals -----------------------------------------------------------------------------------
// One Huffman stream of lit[0, n), last symbol first (HUF_compress1X_usingCTable): exactly
// huf_stream_bytes(bits) bytes, where `bits` is the sum of the symbols' code lengths. Every symbol
// has a code (the caller checked). Returns the bytes written, 0 when they do not fit.
NXZ_HD uint32_t huf_stream_bytes(uint64_t bits) { return (uint32_t)(bits >> 3) + 1; }
// the symbols lit[n - 1] .. lit[0] appended to w
template <typename Ld>
NXZ_HD void huf_put(BitW& w, const uint8_t* lit, uint32_t n, const HufCode* codes, Ld ld) {
    for (uint32_t i = n; i-- > 0;) {
        const HufCode c = codes[ld(lit + i)];
        w.add(c.code, c.nbits);
        if (w.nb > 48) w.flush();
    }
}
template <typename Ld>
NXZ_HD uint32_t huf_encode_stream(uint8_t* dst, uint32_t cap, const uint8_t* lit, uint32_t n,
                                  const HufCode* codes, Ld ld) {
    BitW w(dst, cap);
    huf_put(w, lit, n, codes, ld);
    return w.close();
}

// how a block's literals are written
enum : uint32_t { LIT_RAW = 0, LIT_RLE = 1, LIT_HUF1 = 2, LIT_HUF4 = 3 };
struct LitPlan {
    uint32_t mode, hdr, size;  // header bytes; the whole section's bytes, header included
    uint32_t ssz[4];           // Huffman: each stream's bytes
};
NXZ_HD uint32_t raw_lit_hdr(uint32_t n) { return n < 32 ? 1u : (n < 4096 ? 2u : 3u); }
// `bits[k]`: the code lengths' sum of stream k (one stream: bits[0]; four: segments of
// (n + 3) / 4 literals); `coded`: the dictionary's tree is live and every literal has a code.
NXZ_HD LitPlan plan_literals(uint32_t n, bool all_same, bool coded, const uint64_t* bits) {
    LitPlan p{};
    p.mode = LIT_RAW;
    p.hdr = raw_lit_hdr(n);
    p.size = p.hdr + n;
    if (n > 1 && all_same) {
        p.mode = LIT_RLE;
        p.size = p.hdr + 1;
        return p;
    }
    if (!coded || n < 8) return p;
    if (n < 1024) {
        const uint32_t cs = huf_stream_bytes(bits[0]);
        if (cs < 1024 && 3 + cs < p.size) {
            p.mode = LIT_HUF1;
            p.hdr = 3;
            p.size = 3 + cs;
            p.ssz[0] = cs;
        }
        return p;
    }
    uint32_t cs = 6;
    for (int k = 0; k < 4; k++) cs += huf_stream_bytes(bits[k]);
    const uint32_t hdr = n < 16384 && cs < 16384 ? 4u : 5u;
    if (hdr + cs < p.size) {
        p.mode = LIT_HUF4;
        p.hdr = hdr;
        p.size = hdr + cs;
        for (int k = 0; k < 4; k++) p.ssz[k] = huf_stream_bytes(bits[k]);
    }
    return p;
}
// the literals section's header (and the RLE byte, and the four streams' jump table); the
// streams / raw bytes follow at dst + the return value
NXZ_HD uint32_t write_lit_header(uint8_t* dst, const LitPlan& p, uint32_t n, uint32_t rle_byte) {
    if (p.mode == LIT_RAW || p.mode == LIT_RLE) {
        const uint32_t t = p.mode;
        if (p.hdr == 1) {
            dst[0] = (uint8_t)(t | (n << 3));
        } else if (p.hdr == 2) {
            dst[0] = (uint8_t)(t | (1u << 2) | (n << 4));
            dst[1] = (uint8_t)(n >> 4);
        } else {
            dst[0] = (uint8_t)(t | (3u << 2) | (n << 4));
            dst[1] = (uint8_t)(n >> 4);
            dst[2] = (uint8_t)(n >> 12);
        }
        if (t == LIT_RLE) dst[p.hdr] = (uint8_t)rle_byte;
        return p.hdr + (t == LIT_RLE ? 1u : 0u);
    }
    // Treeless_Literals_Block (3): the dictionary's tree
    const uint32_t cs = p.size - p.hdr;
    uint64_t h;
    if (p.mode == LIT_HUF1) h = 3u | (0u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 14);
    else if (p.hdr == 4) h = 3u | (2u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 18);
    else h = 3u | (3u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 22);
    for (uint32_t i = 0; i < p.hdr; i++) dst[i] = (uint8_t)(h >> (8 * i));
    if (p.mode == LIT_HUF1) return p.hdr;
    for (int k = 0; k < 3; k++) {
        dst[p.hdr + 2 * k] = (uint8_t)p.ssz[k];
        dst[p.hdr + 2 * k + 1] = (uint8_t)(p.ssz[k] >> 8);
    }
    return p.hdr + 6;
}

// ---- a block's own Huffman tree (Compressed_Literals_Block) ----------------------------------------
// From a block's literal histogram: code lengths of at most kHufEncBits, the codes
// (build_huf_enc), and the tree's description (direct 4-bit weights or FSE-compressed weights,
// the smaller). Integer arithmetic only, ties broken by symbol value: the tree is a function of
// the histogram alone.
constexpr uint32_t kHufEncBits = 11;    // the longest code written (readers accept kHufMaxBits)
constexpr uint32_t kHufDescMax = 128;   // header byte + at most 127 bytes of FSE-compressed weights
// Below this many literals no tree pays for itself: the section is at least 3 (header) + 2 (the
// smallest description: one listed weight) + n / 8 + 1 (a bit per literal and the marker) bytes
// against 1 + n raw, smaller only from n = 6.
constexpr uint32_t kFreshMinLits = 6;
enum : uint32_t { kLitDictTree = 0, kLitBlockTrees = 1 };  // NxgZstdCompressOpts.literals

// 2 KiB of working memory (the device lays it over its literal stage, idle at that time).
// a: the symbols' (count << 8 | symbol) keys sorted, then their counts, then their code lengths,
// in place; afterwards build_huf_enc_ws' scratch. hist: the counts by symbol, dead once sorted;
// its bytes then hold the symbols in sorted order, the description and the weights' FSE tables.
struct HufWork {
    uint32_t a[256];
    union {
        uint32_t hist[256];
        struct {
            uint8_t ord[256];
            uint8_t desc[kHufDescMax + 4];
            uint16_t fstate[64];
            FseSym ftt[13];
            int16_t norm[14];
            uint16_t cumul[16];
            uint8_t tsym[64];
            uint32_t cnt[16];
        } t;
    };
};
static_assert(sizeof(HufWork) == 2048, "laid over the literal stage");

// hist -> the present symbols sorted by (count, symbol) ascending: counts in a[0, n), symbols in
// t.ord[0, n). Returns n. Serial (the device sorts with the whole wave: the keys are distinct, so
// every sort gives this order).
NXZ_HD uint32_t huf_sort_hist(HufWork& W) {
    uint32_t n = 0;
    for (uint32_t s = 0; s < 256; s++) {
        const uint32_t c = W.hist[s];
        if (!c) continue;
        const uint32_t key = (c << 8) | s;
        uint32_t i = n++;
        for (; i > 0 && W.a[i - 1] > key; i--) W.a[i] = W.a[i - 1];
        W.a[i] = key;
    }
    for (uint32_t i = 0; i < n; i++) {
        W.t.ord[i] = (uint8_t)W.a[i];
        W.a[i] >>= 8;
    }
    return n;
}

// The weights of n >= 2 sorted symbols (huf_sort_hist): minimum-redundancy code lengths computed
// in place (Moffat and Katajainen 1995: parents left to right, internal depths right to left, leaf
// depths right to left), lengths above kHufEncBits cut to it and the Kraft sum repaired on the
// lengths' counts (one code of the limit and one of the deepest shorter length become two one bit
// longer: the sum falls by one unit of 2^-limit per step, so it ends at exactly 1), the lengths
// then dealt longest first to the symbols in sorted order. w[256]: weight = max_bits + 1 - length,
// 0 for an absent symbol; *n_sym: the last present symbol + 1.
NXZ_HD void huf_build_weights(HufWork& W, uint32_t n, uint8_t* w, uint32_t* n_sym,
                              uint32_t* max_bits) {
    uint32_t* A = W.a;
    const int32_t N = (int32_t)n;
    A[0] += A[1];
    int32_t root = 0, leaf = 2, next;
    for (next = 1; next < N - 1; next++) {
        if (leaf >= N || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= N || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[N - 2] = 0;
    for (next = N - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int32_t avbl = 1, used = 0;
    uint32_t dpth = 0;
    root = N - 2;
    next = N - 1;
    while (avbl > 0) {
        while (root >= 0 && A[root] == dpth) {
            used++;
            root--;
        }
        while (avbl > used) {
            A[next--] = dpth;
            avbl--;
        }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
    uint32_t* nc = W.t.cnt;
    for (uint32_t l = 0; l <= kHufEncBits; l++) nc[l] = 0;
    for (uint32_t i = 0; i < n; i++) nc[A[i] > kHufEncBits ? kHufEncBits : A[i]]++;
    uint32_t total = 0;
    for (uint32_t l = 1; l <= kHufEncBits; l++) total += nc[l] << (kHufEncBits - l);
    while (total > (1u << kHufEncBits)) {
        nc[kHufEncBits]--;
        for (uint32_t l = kHufEncBits - 1; l > 0; l--)
            if (nc[l]) {
                nc[l]--;
                nc[l + 1] += 2;
                break;
            }
        total--;
    }
    uint32_t mb = kHufEncBits;
    while (!nc[mb]) mb--;
    for (uint32_t s = 0; s < 256; s++) w[s] = 0;
    uint32_t i = 0, last = 0;
    for (uint32_t l = mb; l > 0; l--)
        for (uint32_t k = nc[l]; k > 0; k--) {
            const uint32_t s = W.t.ord[i++];
            w[s] = (uint8_t)(mb + 1 - l);
            last = s > last ? s : last;
        }
    *n_sym = last + 1;
    *max_bits = mb;
}

// The listed weights w[0, listed) FSE-compressed at W.t.desc + 1 (HUF_compressWeights): their
// histogram normalised to an accuracy log of 5 (below 64 weights) or 6, the NCount header
// (FSE_writeNCount), two interleaved states from the last weight back. Returns the bytes (0: not
// representable -- one weight value only, or 128 bytes and more).
NXZ_HD uint32_t huf_fse_weights(HufWork& W, const uint8_t* w, uint32_t listed) {
    uint32_t* cnt = W.t.cnt;
    int16_t* norm = W.t.norm;
    for (uint32_t s = 0; s < 14; s++) cnt[s] = 0;
    for (uint32_t i = 0; i < listed; i++) cnt[w[i]]++;
    uint32_t max_sym = 0, distinct = 0, big = 0;
    for (uint32_t s = 0; s <= kHufEncBits; s++) {
        if (!cnt[s]) continue;
        max_sym = s;
        distinct++;
        if (cnt[s] > cnt[big]) big = s;
    }
    if (distinct < 2) return 0;
    const uint32_t al = listed < 64 ? 5u : 6u, size = 1u << al;
    // every present weight at least 1; what is left goes to the most frequent, what is too much
    // comes off the largest
    uint32_t sum = 0;
    for (uint32_t s = 0; s <= max_sym; s++) {
        uint32_t p = cnt[s] * size / listed;
        if (cnt[s] && !p) p = 1;
        norm[s] = (int16_t)p;
        sum += p;
    }
    if (sum < size) norm[big] = (int16_t)(norm[big] + (size - sum));
    for (; sum > size; sum--) {
        uint32_t m = 0;
        for (uint32_t s = 1; s <= max_sym; s++)
            if (norm[s] > norm[m]) m = s;
        norm[m]--;
    }
    uint8_t* d = W.t.desc + 1;
    BitW hw(d, kHufDescMax - 1);
    hw.add(al - 5, 4);
    int32_t remaining = (int32_t)size + 1, threshold = (int32_t)size;
    uint32_t nb = al + 1, sym = 0;
    bool prev0 = false;
    while (remaining > 1) {
        if (prev0) {
            uint32_t run = 0;
            while (norm[sym] == 0) {
                sym++;
                run++;
            }
            for (; run >= 3; run -= 3) hw.add(3, 2);
            hw.add(run, 2);
            hw.flush();
        }
        int32_t c = norm[sym++];
        const int32_t max = (2 * threshold - 1) - remaining;
        remaining -= c;
        prev0 = c == 0;
        c++;
        if (c >= threshold) c += max;
        hw.add((uint32_t)c, nb - (c < max ? 1u : 0u));
        hw.flush();
        while (remaining < threshold) {
            nb--;
            threshold >>= 1;
        }
    }
    if (hw.nb) {  // the last bits' byte
        hw.nb = 8;
        hw.flush();
    }
    if (hw.ovf) return 0;
    const uint32_t nh = hw.n;
    if (!build_fse_enc(W.t.fstate, W.t.ftt, norm, max_sym, al, W.t.cumul, W.t.tsym)) return 0;
    BitW sw(d + nh, kHufDescMax - 1 - nh);
    uint32_t s1 = 0, s2 = 0;  // weights of even index: state 1, of odd index: state 2
    for (uint32_t i = listed; i-- > 0;) {
        uint32_t& st = (i & 1) ? s2 : s1;
        if (i + 2 >= listed) fse_init(st, W.t.ftt, W.t.fstate, w[i]);
        else fse_put(sw, st, W.t.ftt, W.t.fstate, w[i]);
        sw.flush();
    }
    sw.add(s2, al);
    sw.add(s1, al);
    const uint32_t sn = sw.close();
    return sn ? nh + sn : 0u;
}

// The tree's description at W.t.desc: the smaller of the direct form (header 127 + listed
// weights, two weights a byte; up to 128 listed weights) and the FSE form (header: its bytes,
// below 128). Nothing outside W is written, so the size is known before the section is laid out.
// Returns the bytes, 0 when neither form can describe the tree.
NXZ_HD uint32_t write_huf_desc(HufWork& W, const uint8_t* w, uint32_t n_sym) {
    const uint32_t listed = n_sym - 1;
    const uint32_t direct = listed <= 128 ? 1 + (listed + 1) / 2 : 0u;
    const uint32_t fse = huf_fse_weights(W, w, listed);
    uint8_t* d = W.t.desc;
    if (fse && (!direct || 1 + fse < direct)) {
        d[0] = (uint8_t)fse;
        return 1 + fse;
    }
    if (!direct) return 0;
    d[0] = (uint8_t)(127 + listed);
    for (uint32_t i = 0; i < listed; i += 2)
        d[1 + i / 2] = (uint8_t)((w[i] << 4) | (i + 1 < listed ? w[i + 1] : 0));
    return direct;
}

// A Huffman form of `desc` description bytes tried against plan p: taken when smaller.
NXZ_HD bool plan_huf(LitPlan& p, uint32_t n, const uint64_t* bits, uint32_t desc) {
    if (n < 1024) {
        const uint32_t cs = desc + huf_stream_bytes(bits[0]);
        if (cs >= 1024 || 3 + cs >= p.size) return false;
        p.mode = LIT_HUF1;
        p.hdr = 3;
        p.size = 3 + cs;
        p.ssz[0] = cs - desc;
        return true;
    }
    uint32_t cs = desc + 6;
    for (int k = 0; k < 4; k++) cs += huf_stream_bytes(bits[k]);
    const uint32_t hdr = n < 16384 && cs < 16384 ? 4u : 5u;
    if (hdr + cs >= p.size) return false;
    p.mode = LIT_HUF4;
    p.hdr = hdr;
    p.size = hdr + cs;
    for (int k = 0; k < 4; k++) p.ssz[k] = huf_stream_bytes(bits[k]);
    return true;
}
// Literals with block trees (kLitBlockTrees). The candidates in order, the earlier on a tie: raw,
// RLE, treeless with the frame's live tree (`live`: there is one and every literal has a code;
// this is plan_literals), a Compressed_Literals_Block with the fresh tree (`fresh_ok`: it has a
// description, of `desc` bytes, which count in the section's compressed size). *fresh: the last
// was taken, and the block's tree becomes the live one once the block is written.
NXZ_HD LitPlan plan_literals_trees(uint32_t n, bool all_same, bool live, const uint64_t* bits_live,
                                   bool fresh_ok, const uint64_t* bits_fresh, uint32_t desc,
                                   bool* fresh) {
    LitPlan p = plan_literals(n, all_same, live, bits_live);
    *fresh = false;
    if (p.mode == LIT_RLE || !fresh_ok || n < kFreshMinLits) return p;
    *fresh = plan_huf(p, n, bits_fresh, desc);
    return p;
}
// write_lit_header for a plan of plan_literals_trees: a fresh tree's section is header (type 2),
// description, jump table, streams.
NXZ_HD uint32_t write_lit_header_trees(uint8_t* dst, const LitPlan& p, uint32_t n, uint32_t rle_byte,
                                       bool fresh, const uint8_t* desc, uint32_t dsz) {
    if (!fresh) return write_lit_header(dst, p, n, rle_byte);
    const uint32_t cs = p.size - p.hdr;
    uint64_t h;
    if (p.mode == LIT_HUF1) h = 2u | (0u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 14);
    else if (p.hdr == 4) h = 2u | (2u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 18);
    else h = 2u | (3u << 2) | ((uint64_t)n << 4) | ((uint64_t)cs << 22);
    for (uint32_t i = 0; i < p.hdr; i++) dst[i] = (uint8_t)(h >> (8 * i));
    uint32_t at = p.hdr;
    for (uint32_t i = 0; i < dsz; i++) dst[at++] = desc[i];
    if (p.mode == LIT_HUF1) return at;
    for (int k = 0; k < 3; k++) {
        dst[at++] = (uint8_t)p.ssz[k];
        dst[at++] = (uint8_t)(p.ssz[k] >> 8);
    }
    return at;
}

// ---- frame and block headers --------------------------------------------------------------------
constexpr uint32_t kFrameHdrMax = 17;  // magic 4, descriptor 1, Dictionary_ID 4, content size 8
// Single_Segment, Frame_Content_Size, no checksum, the Dictionary_ID (0: none) in its smallest
// field (ZSTD_writeFrameHeader). Returns the header's bytes.
NXZ_HD uint32_t write_frame_header(uint8_t* p, uint64_t size, uint32_t dict_id) {
    const uint32_t dc = (dict_id > 0) + (dict_id >= 256) + (dict_id >= 65536);
    const uint32_t fc = (size >= 256) + (size >= 65536 + 256) + (size >= 0xFFFFFFFFull);
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(kFrameMagic >> (8 * i));
    p[4] = (uint8_t)(dc | (1u << 5) | (fc << 6));
    uint32_t n = 5;
    const uint32_t dl = dc == 3 ? 4 : dc;
    for (uint32_t i = 0; i < dl; i++) p[n++] = (uint8_t)(dict_id >> (8 * i));
    const uint64_t v = fc == 1 ? size - 256 : size;
    const uint32_t fl = 1u << fc;
    for (uint32_t i = 0; i < fl; i++) p[n++] = (uint8_t)(v >> (8 * i));
    return n;
}
NXZ_HD void write_block_header(uint8_t* p, uint32_t type, uint32_t size, bool last) {
    const uint32_t h = (last ? 1u : 0u) | (type << 1) | (size << 3);
    p[0] = (uint8_t)h;
    p[1] = (uint8_t)(h >> 8);
    p[2] = (uint8_t)(h >> 16);
}
// the blocks of a batch, and a frame's worst case: every block raw
NXZ_HD uint64_t n_blocks(uint64_t len) { return len ? (len + kBlockMax - 1) / kBlockMax : 1; }
NXZ_HD uint64_t frame_bound(uint64_t len) { return kFrameHdrMax + len + 3 * n_blocks(len); }

// the match hash: 4 bytes, `bits` bits
NXZ_HD uint32_t hash4(uint32_t v, uint32_t bits) { return (v * 2654435761u) >> (32 - bits); }

}  // namespace nxz
