// nxg_decode_writes_fast.hip -- the fast decoder of publisher::To frames (NxgStatus.path 8) for
// gfx950: the To counterpart of nxg_decode_mixed.hip, built on the same helpers
// (nxg_fmx_common.h). Opt-in (nxg_decode_writes_opts, fast = 1); the general decoder's To
// instantiation (nxg_decode_gen.hip) is the exact fallback and the only reporter of errors.
//
// What it takes. Every message of the frame must be one of
//   Write        L 02 varint(id) bool Value [varint(wid)]: a one-byte L (the message < 128 bytes),
//                an id of any width, bool 0 / 1, a Value without child slots that
//                val_decode takes and finds valid (fixed-size and varint scalars, DateTime,
//                Duration, String, Bytes, Decimal, Error(String)), then nothing (NXG_WRITE_NO_WID)
//                or one varint of 1-10 bytes that ends exactly at the message end
//   Unsubscribe  L 01 varint(id), the id of any width, L filled exactly
//   Subscribe    varint(L) 00 varint(plen) path tag addr u64 u32 varint(tlen) token: address tag
//                0 / 1, L filled exactly, the path valid UTF-8, the whole message (its one- or
//                two-byte prefix included) at most 256 bytes
// with canonical length prefixes (L counts its own prefix: a message at p ends at p + L).
// The choices the contract leaves open: ids wider than 35 bits and non-canonical id / wid varints
// are taken (wvar decodes them as decode_varint does); non-canonical plen / tlen,
// Subscribes longer than 256 bytes, Abstract values and every value with child slots (Array, Map,
// Error(Value)) are declined, as is a message with bytes left inside its length wrap (a wid cut
// short by the message end included). A declined frame raises DevStatus.fast_fail and the host
// reruns it on the general decoder, so path 8 implies err_kind 0 and n_children 0.
//
// Since no message is longer than 256 bytes, a message starts within the first 256 bytes of
// every tile and every message lies inside the image (tile + 256 B) of the tile it starts in.
//
//   count    per tile (a wave): the guessed entry -- the first positions among the tile's first
//            256 bytes that hold a complete message of the accepted set (probe: prefix, variant,
//            the Unsubscribe / Subscribe length identity, the Write's bool and value tag), tried
//            in order until the chain of messages from one reaches the tile end (the starts on a
//            chain that breaks are struck from the candidates; at most 16 chains) -- then exit,
//            Writes, control messages and the message starts as a bit per byte. Tile 0 enters
//            at 0; if its chain breaks the frame is declined at once. A chain is followed as
//            tile_chain of the mixed decoder does: each lane takes a 64-byte chunk, finds its
//            first two confirmed starts (a SWAR filter, then probe) and where their chains leave
//            the chunk; one uniform loop over the chunks then hops from exit to exit (an entry
//            that is neither start is walked), and each lane walks its chunk from its entry for
//            the starts and counts.
//   fix      per tile: a tile whose entry is not its predecessor's counted exit is recounted
//            from that exit (descriptors read from the count pass's array, written to a second
//            one, so no wave reads what another is writing)
//   resolve  a lane per tile: block scan of (Writes, control messages), the chain check, and the
//            last block to arrive scans the block sums and checks cap_rows / cap_ctl before
//            anything is emitted
//   emit     per tile: the chain check (entry = predecessor's exit, tile 0 at 0; the count pass
//            lets no chain end anywhere but exactly at W), then the messages 64 at a time, one
//            per lane: val_decode for a Write's value, the wid, the text checks (ASCII per lane,
//            the rest by utf8_packed), rows and spans through col_st
// A guess that is wrong but merges into the true chain inside its tile (the common case: a false
// start inside a token or a float dies or merges within a few messages) costs that tile a
// recount; a false chain that leaves its tile unmerged, or two tiles in a row that each hold
// more than 16 breaking false chains in front of their true entry (the second has no counted
// predecessor exit to be recounted from), leave a broken link after the one fix round and the
// frame goes to the general decoder. No workgroup waits on another.
#include <algorithm>

#include "nxg_fmx_common.h"

#ifndef NXG_FF_CHECK
#define NXG_FF_CHECK 1  // the later passes skip a frame already declined
#endif

namespace {
using namespace fmx;
using namespace nxgmsg;

constexpr uint32_t MAXMSG = 256;  // bytes of the longest message taken, prefix included
constexpr uint32_t MINMSG = 3;    // 03 01 xx: an Unsubscribe with a one-byte id
// message starts per tile (TILE / MINMSG = 1366), rounded up to whole rounds of 64
constexpr uint32_t MAXW = ((TILE + MINMSG - 1) / MINMSG + 63) / 64 * 64;
constexpr uint32_t PAD = 64;  // ascii_ok reads up to 39 bytes past a position < IMG
constexpr uint32_t TRIES = 16;  // entry guesses per tile (broken chains tried before giving up)
static_assert(MAXMSG <= IMG - TILE, "a message lies inside the image of the tile it starts in");

struct CountLds {
    uint8_t img[IMG + PAD];
};
struct EmitLds {
    uint8_t img[IMG + PAD];
    uint16_t msg[MAXW];  // the tile's message starts
    uint8_t mark[256];   // utf8_packed
};
static_assert(sizeof(EmitLds) * (TPB / 64) <= 32768, "emit LDS: 5 workgroups per CU");

struct WTile {
    uint32_t entry, exit;  // tile offsets (FAIL: no chain)
    uint32_t rows, ctl;    // Writes, Subscribes + Unsubscribes
};

struct Msg {
    uint32_t len;         // prefix included; 0: not a message of the accepted set
    uint32_t kind;        // the variant: 0 Subscribe, 1 Unsubscribe, 2 Write
    uint32_t soff, slen;  // a Subscribe's path (tile offset, bytes)
};

NXG_DEV uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// byte i (0..15) of a 16-byte window
NXG_DEV uint32_t byte_at(Win16 w, uint32_t i) {
    const uint64_t lo = w.lo, hi = w.hi;  // (values, so that the select is not one of addresses)
    const uint64_t x = i < 8u ? lo : hi;
    return (uint32_t)(x >> (8u * (i & 7u))) & 0xffu;
}

// The message at tile offset x, when it is one the fast path takes as far as its structure goes
// (the value's payload, the wid and the text are the emit pass's): everything read lies below
// x + len <= wend, the end of the frame in the image.
NXG_DEV Msg probe(lds_bytes img, uint32_t x, uint32_t wend) {
    Msg r{0, 0, 0, 0};
    const Win16 w = win16(img, x);
    const uint32_t b0 = (uint32_t)w.lo & 0xffu, b1 = (uint32_t)(w.lo >> 8) & 0xffu;
    const bool two = b0 >= 0x80u;
    const uint32_t L = two ? (b0 & 0x7fu) | (b1 << 7) : b0;
    const uint32_t nbp = two ? 2u : 1u;
    if ((two && (b1 == 0u || b1 >= 0x80u)) || L < MINMSG || L > MAXMSG || x + L > wend) return r;
    const uint32_t sh = 8u * nbp;
    const uint32_t v = (uint32_t)(w.lo >> sh) & 0xffu;  // the variant
    // the 8 bytes after the variant
    const uint64_t f = (w.lo >> (sh + 8u)) | (w.hi << (56u - sh));
    const uint64_t stop = ~f & 0x8080808080808080ull;
    const uint32_t k = stop ? (uint32_t)__builtin_ctzll(stop) >> 3 : 8u;  // varint bytes - 1
    if (v == 1u || v == 2u) {  // an id varint of 1-10 bytes at x + 2 (a one-byte L)
        uint32_t vl = k + 1u;
        if (!stop) {  // 9 or 10 bytes: wire bytes x + 10, x + 11
            const uint32_t c8 = (uint32_t)(w.hi >> 16) & 0xffu, c9 = (uint32_t)(w.hi >> 24) & 0xffu;
            vl = c8 < 0x80u ? 9u : (c9 < 0x80u ? 10u : 0u);
        }
        if (two || vl == 0u) return r;
        if (v == 1u) {  // Unsubscribe(Id): L = 2 + vl(id)
            if (L != 2u + vl) return r;
        } else {  // Write(Id, bool, Value, WriteId): bool, a leaf tag (wire bytes <= x + 14)
            if (L < vl + 4u) return r;
            const uint32_t reply = byte_at(w, 2u + vl), t = byte_at(w, 3u + vl);
            const uint32_t c = byte_at(w, 4u + vl);
            if (reply > 1u || t >= 27u || t == 19u || t == 21u || (t == 22u && c != 12u)) return r;
        }
        r.len = L;
        r.kind = v;
        return r;
    }
    if (v != 0u) return r;
    // Subscribe: L = nbp + 1 + vl(plen) + plen + 1 + (6 | 26) + 12 + vl(tlen) + tlen
    const uint32_t p0 = (uint32_t)f & 0xffu, p1 = (uint32_t)(f >> 8) & 0xffu;
    const bool ptwo = p0 >= 0x80u;
    if (ptwo && (p1 == 0u || p1 >= 0x80u)) return r;
    const uint32_t plen = ptwo ? (p0 & 0x7fu) | (p1 << 7) : p0;
    const uint32_t hdr = nbp + 1u + (ptwo ? 2u : 1u);
    if (plen > MAXMSG || hdr + plen + 20u > L) return r;  // tag, V4 address, u64, u32, tlen
    const uint32_t a = hdr + plen;  // the address tag
    const uint32_t at = img[x + a];
    if (at > 1u) return r;
    const uint32_t tp = a + 1u + (at ? 26u : 6u) + 12u;  // the token's length
    if (tp >= L) return r;
    const uint32_t t0 = img[x + tp], t1 = img[x + tp + 1u];
    const bool ttwo = t0 >= 0x80u;
    if (ttwo && (t1 == 0u || t1 >= 0x80u)) return r;
    const uint32_t tlen = ttwo ? (t0 & 0x7fu) | (t1 << 7) : t0;
    if (tp + (ttwo ? 2u : 1u) + tlen != L) return r;
    r.len = L;
    r.kind = 0;
    r.soff = x + hdr;
    r.slen = plen;
    return r;
}

// Positions of the lane's chunk (bit i: chunk byte i) that may start a message: a byte in
// [3, 127] followed by a variant <= 2, or a two-byte prefix of 128..256 (a byte >= 0x80, then 1 or
// 2) followed by 00. A superset of the starts probe() confirms wherever a chain can enter a
// chunk -- and only a filter: a start it misses is walked by the uniform fallback of chain().
// Lane j reads its words in the order k + j / 2 (mod 16), as cand_mask of the mixed decoder does,
// so that a half-wave's 32 lanes read 32 different banks.
NXG_DEV uint64_t start_filter(const uint8_t* img, uint32_t c) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(img + c);
    const uint32_t rot = (c >> 7) & 15u;
    uint64_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t kk = ((uint32_t)k + rot) & 15u;
        const uint32_t a = w[kk], b = w[kk + 1];
        const uint32_t a1 = alignbyte(b, a, 1), a2 = alignbyte(b, a, 2);
        const uint32_t ge3 = ((a & 0x7f7f7f7fu) + 0x7d7d7d7du) & ~a & 0x80808080u;
        const uint32_t le2 = ~(((a1 & 0x7f7f7f7fu) + 0x7d7d7d7du) | a1) & 0x80808080u;
        const uint32_t two = a & le2 & ~zero_bytes(a1) & zero_bytes(a2);
        m |= (uint64_t)nib((ge3 & le2) | two) << (4 * kk);
    }
    return m;
}

// where the chain of messages from tile offset x leaves [.., end), or FAIL (a position on the way
// holds no message of the accepted set)
NXG_DEV uint32_t chunk_exit(lds_bytes img, uint32_t x, uint32_t end, uint32_t wend) {
#pragma unroll 1
    while (x < end) {
        const uint32_t len = probe(img, x, wend).len;
        if (len == 0u) return FAIL;
        x += len;
    }
    return x;
}

// per lane: the first two confirmed message starts of its chunk and where their chains leave it
struct Cands {
    uint32_t c0, x0, c1, x1;
};
NXG_DEV Cands lane_cands(const uint8_t* img, uint32_t lane, uint32_t lim, uint32_t wend) {
    Cands r{FAIL, FAIL, FAIL, FAIL};
    const uint32_t c = lane * CH;
    if (c >= lim) return r;
    const uint32_t end = min(c + CH, lim);
    uint64_t pm = start_filter(img, c);
    if (end - c < 64u) pm &= (1ull << (end - c)) - 1ull;
    uint32_t found = 0;
#pragma unroll 1
    while (pm && found < 2u) {
        const uint32_t p = c + (uint32_t)__builtin_ctzll(pm);
        pm &= pm - 1;
        if (probe((lds_bytes)img, p, wend).len == 0u) continue;
        const uint32_t x = chunk_exit((lds_bytes)img, p, end, wend);
        if (found == 0u) {
            r.c0 = p;
            r.x0 = x;
        } else {
            r.c1 = p;
            r.x1 = x;
        }
        found++;
    }
    return r;
}

// The chain of messages from tile offset e (uniform): the tile's descriptor, and the starts that
// fall into the lane's chunk as bits. One uniform loop over the 64 chunks follows the chain: a
// chunk entered at its lane's first or second confirmed start takes that start's exit, any other
// entry is walked; then every lane walks its own chunk from where the chain enters it for the
// starts and the counts. FAIL entry and exit when a position on the way holds no message of the
// accepted set (bits then hold the starts passed on the way). lim: the tile's end (the frame's,
// in the last tile); no message ends past wend, so the last tile's chain ends exactly at the
// frame end or not at all.
NXG_DEV WTile walk(lds_bytes img, const Cands& cd, uint32_t e, uint32_t lim, uint32_t wend,
                   uint32_t lane, uint64_t& bits) {
    uint32_t ce = NONE, x = e;
#pragma unroll 1
    for (uint32_t j = e >> 6; j < TILE / CH && x < lim && x != FAIL; j++) {
        if (x >= (j + 1u) * CH) continue;  // a message covers the whole chunk
        if (lane == j) ce = x;
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)cd.c0, (int)j);
        const uint32_t a1 = (uint32_t)__builtin_amdgcn_readlane((int)cd.c1, (int)j);
        if (x == a0) {
            x = (uint32_t)__builtin_amdgcn_readlane((int)cd.x0, (int)j);
        } else if (x == a1) {
            x = (uint32_t)__builtin_amdgcn_readlane((int)cd.x1, (int)j);
        } else {
            x = (uint32_t)__builtin_amdgcn_readfirstlane(
                (int)chunk_exit(img, x, min((j + 1u) * CH, lim), wend));
        }
    }
    // the lane's chunk from its entry: starts, Writes, control messages
    uint32_t nw = 0, nc = 0;
    bool ok = true;
    bits = 0;
    if (ce != NONE) {
        const uint32_t c = lane * CH, end = min(c + CH, lim);
        uint32_t y = ce;
#pragma unroll 1
        while (y < end) {
            const Msg m = probe(img, y, wend);
            if (m.len == 0u) {
                ok = false;
                break;
            }
            bits |= 1ull << (y - c);
            nw += m.kind == 2u ? 1u : 0u;
            nc += m.kind == 2u ? 0u : 1u;
            y += m.len;
        }
    }
    if (__any(!ok) || x == FAIL) return WTile{FAIL, FAIL, 0, 0};
    return WTile{e, x, wave_sum<uint32_t>(nw), wave_sum<uint32_t>(nc)};
}

struct Geo {  // tile t of a W-byte frame
    uint64_t t0;
    uint32_t lim, wend;
};
NXG_DEV Geo geo_of(uint64_t t, uint64_t W) {
    const uint64_t t0 = t * TILE;
    return Geo{t0, (uint32_t)min<uint64_t>(TILE, W - t0), (uint32_t)min<uint64_t>(IMG, W - t0)};
}

}  // namespace

// count: one wave per tile
__global__ __launch_bounds__(TPB) void nxg_wfast_count_kernel(const uint8_t* __restrict__ wire,
                                                              uint64_t W, uint64_t nt,
                                                              WTile* __restrict__ td,
                                                              uint64_t* __restrict__ starts,
                                                              DevStatus* __restrict__ st,
                                                              DevStatus* zst) {
    zero_status(zst);
    __shared__ __attribute__((aligned(16))) CountLds lds[TPB / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * (TPB / 64) + w;
    if (t >= nt) return;
    const Geo g = geo_of(t, W);
    uint8_t* img = lds[w].img;
    const lds_bytes limg = (lds_bytes)img;
    TileRegs tr;
    tile_load(tr, wire, g.t0, W, lane);
    tile_store(img, tr, lane);
    uint64_t bits = 0;
    WTile d{FAIL, FAIL, 0, 0};
    const Cands cd = lane_cands(img, lane, g.lim, g.wend);
    if (t == 0) {
        d = walk(limg, cd, 0, g.lim, g.wend, lane, bits);
        if (d.entry == FAIL) bits = 0;
        if (d.entry == FAIL && lane == 0) atomicOr(&st->fast_fail, 1u);  // not a frame for this path
    } else {
        // candidates: position lane + 64 q of the tile's first 256 bytes holds a whole message
        uint64_t cm[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t p = lane + 64u * q;
            cm[q] = __ballot(p < g.lim && probe(limg, p, g.wend).len != 0u);
        }
#pragma unroll 1
        for (uint32_t tries = 0; tries < TRIES && d.entry == FAIL; tries++) {
            uint32_t gss = FAIL;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if (gss == FAIL && cm[q]) {
                    gss = 64u * q + (uint32_t)__builtin_ctzll(cm[q]);
                    cm[q] &= cm[q] - 1;
                }
            }
            if (gss == FAIL) break;
            d = walk(limg, cd, gss, g.lim, g.wend, lane, bits);
            if (d.entry == FAIL) {
                // every start on a broken chain leads to the same break: none is tried again
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, (int)q);
                    const uint32_t hi =
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), (int)q);
                    cm[q] &= ~(((uint64_t)hi << 32) | lo);
                }
            }
        }
        if (d.entry == FAIL) bits = 0;
    }
    starts[t * 64 + lane] = bits;
    if (lane == 0) td[t] = d;
}

// fix: one wave per tile; a tile entered elsewhere than at its predecessor's counted exit is
// recounted from that exit. Reads td (the count pass's), writes td2.
__global__ __launch_bounds__(TPB) void nxg_wfast_fix_kernel(const uint8_t* __restrict__ wire,
                                                            uint64_t W, uint64_t nt,
                                                            const WTile* __restrict__ td,
                                                            WTile* __restrict__ td2,
                                                            uint64_t* __restrict__ starts,
                                                            DevStatus* __restrict__ st) {
    __shared__ __attribute__((aligned(16))) CountLds lds[TPB / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * (TPB / 64) + w;
    if (t >= nt) return;
    if (NXG_FF_CHECK && st->fast_fail) return;
    WTile d = td[t];
    uint32_t pe = FAIL;
    if (t > 0) {
        const uint32_t px = td[t - 1].exit;
        if (px != FAIL && px - TILE < MAXMSG) pe = px - TILE;
    }
    pe = (uint32_t)__builtin_amdgcn_readfirstlane((int)pe);
    if (pe != FAIL && pe != (uint32_t)__builtin_amdgcn_readfirstlane((int)d.entry)) {
        const Geo g = geo_of(t, W);
        uint8_t* img = lds[w].img;
        TileRegs tr;
        tile_load(tr, wire, g.t0, W, lane);
        tile_store(img, tr, lane);
        uint64_t bits;
        const Cands cd = lane_cands(img, lane, g.lim, g.wend);
        d = walk((lds_bytes)img, cd, pe, g.lim, g.wend, lane, bits);
        starts[t * 64 + lane] = d.entry == FAIL ? 0ull : bits;
        if (lane == 0) atomicAdd(&st->diag[5], 1ull);  // recounted tiles (diagnostics)
    }
    if (lane == 0) td2[t] = d;
}

// resolve: a lane per tile. Block scan of (Writes | control messages << 32) -> tloc; the chain
// check; the last block to arrive (DevStatus.diag[7], zeroed with the slot) scans the block sums
// -> bpre, checks the capacities and writes the totals. Frames are shorter than 2^32 bytes, so
// both halves stay in 32 bits.
__global__ __launch_bounds__(TPB) void nxg_wfast_resolve_kernel(
    uint64_t nt, const WTile* __restrict__ td2, uint64_t* __restrict__ tloc,
    uint64_t* __restrict__ bsum, uint64_t* __restrict__ bpre, uint64_t cap_rows, uint64_t cap_ctl,
    DevStatus* __restrict__ st) {
    __shared__ uint64_t scan_tmp[TPB / 64];
    __shared__ uint32_t is_last;
    const uint32_t bid = blockIdx.x;
    const uint64_t tl = (uint64_t)bid * TPB + threadIdx.x;
    uint64_t v = 0;
    bool broken = false;
    if (tl < nt) {
        const WTile d = td2[tl];
        const uint32_t px = tl ? td2[tl - 1].exit : TILE;
        broken = d.entry == FAIL || px == FAIL || px - TILE != d.entry;
        v = (uint64_t)d.rows | ((uint64_t)d.ctl << 32);
    }
    if (__any(broken) && (threadIdx.x & 63) == 0) atomicOr(&st->fast_fail, 1u);
    uint64_t tot;
    const uint64_t ex = block_excl_scan<uint64_t, TPB>(v, scan_tmp, &tot);
    if (tl < nt) tloc[tl] = ex;
    // the block sums go out with agent-scope stores, drained before the arrival count; the last
    // block reads them with agent-scope loads
    if (threadIdx.x == 0) {
        st_agent(&bsum[bid], tot);
        drain_stores();
        is_last = atomicAdd(&st->diag[7], 1ull) == (unsigned long long)gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    const uint32_t nb = gridDim.x;
    uint64_t run = 0;
#pragma unroll 1
    for (uint32_t b0 = 0; b0 < nb; b0 += TPB) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t x = b < nb ? ld_agent(&bsum[b]) : 0ull;
        uint64_t t2;
        const uint64_t e2 = block_excl_scan<uint64_t, TPB>(x, scan_tmp, &t2);
        if (b < nb) bpre[b] = run + e2;
        run += t2;
    }
    if (threadIdx.x == 0) {
        const uint64_t nr = run & 0xffffffffull, nc = run >> 32;
        if (nr > cap_rows || nc > cap_ctl) {
            // columns too small: the general decoder reports the capacity error
            st->capacity = 1u;
            atomicOr(&st->fast_fail, 1u);
        } else {
            st->n_rows = nr;
            st->n_children = 0;
            st->n_ctl = nc;
            st->n_heartbeat = 0;
            st->path = NXG_PATH_WRITES_FAST;
        }
    }
}

// emit: one wave per tile, a message per lane and round
__global__ __launch_bounds__(TPB, 5) void nxg_wfast_emit_kernel(
    const uint8_t* __restrict__ wire, uint64_t W, uint64_t nt, const WTile* __restrict__ td2,
    const uint64_t* __restrict__ tloc, const uint64_t* __restrict__ bpre,
    const uint64_t* __restrict__ starts, ColsDesc cols, DevStatus* __restrict__ st) {
    __shared__ __attribute__((aligned(16))) EmitLds lds[TPB / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * (TPB / 64) + w;
    if (t >= nt) return;
    uint8_t* img = lds[w].img;
    uint16_t* msg = lds[w].msg;
    const lds_bytes limg = (lds_bytes)img;
    const Geo g = geo_of(t, W);
    TileRegs tr;
    tile_load(tr, wire, g.t0, W, lane);
    uint64_t bits = starts[t * 64 + lane];
    const WTile d = td2[t];
    const uint32_t px = t ? td2[t - 1].exit : TILE;
    const uint64_t base = bpre[t / TPB] + tloc[t];
    // a frame already declined (a plain read: one scalar load, not an agent-scope load per wave)
    if (NXG_FF_CHECK && st->fast_fail) return;
    tile_store(img, tr, lane);
    const uint32_t nm = d.rows + d.ctl;
    uint64_t rnext = base & 0xffffffffull;  // next row
    uint64_t cnext = base >> 32;            // next control span
    // the message list in wire order
    const uint32_t n0 = (uint32_t)__popcll(bits);
    uint32_t at = wave_incl_scan<uint32_t>(n0) - n0;
    // the chain: this tile is entered at its predecessor's exit (tile 0 at 0)
    bool bad = d.entry == FAIL || px == FAIL || px - TILE != d.entry || nm > MAXW ||
               wave_last<uint32_t>(at + n0) != nm;
    if (!bad) {
#pragma unroll 1
        while (bits) {
            msg[at++] = (uint16_t)(lane * CH + (uint32_t)__builtin_ctzll(bits));
            bits &= bits - 1;
        }
    }
    wave_lds_order();
    uint32_t wseen = 0;  // Writes emitted (against the count)
#pragma unroll 1
    for (uint32_t k = 0; k < nm && !bad; k += 64) {
        const uint32_t i = k + lane;
        const bool has = i < nm;
        const uint32_t p = has ? msg[i] : 0u;
        const Msg m = probe(limg, p, g.wend);
        const bool isw = has && m.len && m.kind == 2u;
        const bool isc = has && m.len && m.kind != 2u;
        bool ok = !has || m.len != 0u;
        const uint64_t wm = __ballot(isw);
        const uint32_t wbefore = lanes_below(wm);
        const uint64_t row = rnext + wbefore;
        const uint64_t cix = cnext + (lane - wbefore);
        // the Write: L 02, the id varint, bool, tag (16 bytes from the id), then the 12 bytes
        // after the tag
        const uint32_t lim = p + m.len;
        const Win16 hw = win16(limg, p + 2u);
        uint64_t id;
        const uint32_t nb = wvar(hw.lo, hw.hi, id);  // 1..10 (0: no varint; the count pass)
        const uint32_t reply = byte_at(hw, nb), tg = byte_at(hw, nb + 1u);
        const uint32_t u = 4u + nb;  // the payload, relative to p
        uint32_t V[3];
        win_words<3>(limg, p + u, V);
        const uint32_t V0 = V[0], V1 = V[1], V2 = V[2];
        // (lanes without a Write decode a V32 from their bytes: cheap, and never used)
        const FV o = val_decode(isw ? tg : 1u, V0, V1, V2, p + u, isw ? lim : p + u + 12u, false,
                                g.t0);
        uint64_t wid = 0;
        uint32_t wfl = reply;
        if (isw) {
            ok = o.ok && o.end <= lim && tg != 27u && reply <= 1u && nb != 0u;
            if (ok && o.end < lim) {  // the WriteId: one varint that ends the message
                const Win16 ww = win16(limg, o.end);
                const uint32_t nw = wvar(ww.lo, ww.hi, wid);
                ok = nw != 0u && o.end + nw == lim;
            } else {
                wfl |= (uint32_t)NXG_WRITE_NO_WID;
            }
        }
        bad = __any(!ok);
        if (bad) break;
        // text: a Write's String / Error(String), a Subscribe's path
        const uint32_t so = isw ? o.soff : m.soff;
        const uint32_t sl = isw ? o.slen : (isc ? m.slen : 0u);
        const bool na = sl && !ascii_ok(limg, so, sl);
        bad = !utf8_packed(limg, lds[w].mark, na, so, sl, lane);
        if (bad) break;
        if (isw && row < cols.cap_rows) {
            col_st(&cols.id[row], (uint64_t)id);
            col_st(&cols.tag[row], (uint8_t)o.tag);
            col_st(&cols.fixed[row], (uint64_t)o.fixed);
            col_st(&cols.aux[row], (uint32_t)o.aux);
            col_st(&cols.wflags[row], (uint8_t)wfl);
            col_st(&cols.wid[row], (uint64_t)wid);
        }
        if (isc && cix < cols.cap_ctl) {
            col_st(&cols.ctl_row[cix], (uint64_t)row);
            col_st(&cols.ctl_off[cix], (uint64_t)(g.t0 + p));
            col_st(&cols.ctl_len[cix], (uint32_t)m.len);
            col_st(&cols.ctl_variant[cix], (uint8_t)m.kind);
        }
        const uint32_t nwr = (uint32_t)__popcll(wm);
        rnext += nwr;
        cnext += min(nm - k, 64u) - nwr;
        wseen += nwr;
    }
    bad = bad || wseen != d.rows;
    if (bad && lane == 0) atomicOr(&st->fast_fail, 1u);
}

// ---- launch (host) --------------------------------------------------------------------------------
static uint64_t wfast_tiles(uint64_t W) { return (W + TILE - 1) / TILE; }

uint64_t nxg_wfast_scratch_bytes(uint64_t W) {
    const uint64_t nt = wfast_tiles(W);
    // 2 descriptors 32 B, message starts 512 B, tloc 8 B per tile; bsum + bpre 16 B per 256
    // tiles; alignment
    return nt * 552 + 16 * (nt / TPB + 1) + 6 * 16;
}

// frames the fast decoder is launched on at all: 32-bit per-tile counts and row totals
bool nxg_wfast_takes(uint64_t W) { return W > 0 && W < (1ull << 32); }

hipError_t nxg_launch_dec_wfast(const uint8_t* wire, uint64_t W, const ColsDesc& cols,
                                uint8_t* scratch, DevStatus* st, hipStream_t s) {
    if (!nxg_wfast_takes(W)) return hipErrorInvalidValue;
    if (!cols.id || !cols.tag || !cols.fixed || !cols.aux || !cols.ctl_row || !cols.ctl_off ||
        !cols.ctl_len || !cols.ctl_variant || !cols.wflags || !cols.wid)
        return hipErrorInvalidValue;
    const uint64_t nt = wfast_tiles(W);
    uint8_t* p = scratch;
    auto take = [&](uint64_t bytes) {
        uint8_t* r = p;
        p += (bytes + 15) & ~15ull;
        return r;
    };
    WTile* td = reinterpret_cast<WTile*>(take(16 * nt));
    WTile* td2 = reinterpret_cast<WTile*>(take(16 * nt));
    uint64_t* starts = reinterpret_cast<uint64_t*>(take(512 * nt));
    uint64_t* tloc = reinterpret_cast<uint64_t*>(take(8 * nt));
    const uint64_t nb = (nt + TPB - 1) / TPB;
    uint64_t* bsum = reinterpret_cast<uint64_t*>(take(8 * nb));
    uint64_t* bpre = reinterpret_cast<uint64_t*>(take(8 * nb));
    constexpr uint64_t WV = TPB / 64;  // waves (tiles) per workgroup
    const uint32_t gc = (uint32_t)((nt + WV - 1) / WV);
    hipLaunchKernelGGL(nxg_wfast_count_kernel, dim3(gc), dim3(TPB), 0, s, wire, W, nt, td, starts,
                       st, nxg_take_zero_slot());
    hipLaunchKernelGGL(nxg_wfast_fix_kernel, dim3(gc), dim3(TPB), 0, s, wire, W, nt, td, td2,
                       starts, st);
    hipLaunchKernelGGL(nxg_wfast_resolve_kernel, dim3((uint32_t)nb), dim3(TPB), 0, s, nt, td2,
                       tloc, bsum, bpre, cols.cap_rows, cols.cap_ctl, st);
    hipLaunchKernelGGL(nxg_wfast_emit_kernel, dim3(gc), dim3(TPB), 0, s, wire, W, nt, td2, tloc,
                       bpre, starts, cols, st);
    return hipGetLastError();
}
