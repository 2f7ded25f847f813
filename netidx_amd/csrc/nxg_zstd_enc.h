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
NXZ_HD void build_huf_enc(HufCode* codes, const uint8_t* w, uint32_t n_sym, uint32_t max_bits) {
    uint32_t start[kHufMaxBits + 2] = {0};
    uint32_t cnt[kHufMaxBits + 2] = {0};
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
