// nxg_archive_index.hip -- the RecordIndex of an indexed archive (netidx-archive logfile/mod.rs:
// 146-149): written per record (nxg_archive_index_records, the HashSet loop of writer.rs:407-429)
// and scanned by Id set (nxg_archive_scan_index, scan_index_at, reader.rs:394-422).
//
// ---- the writer ---------------------------------------------------------------------------------
// Record c's index lists the distinct kept Ids of positions [seg_off[c], seg_off[c+1]), each once,
// in order of first occurrence:  varint(L) varint(count) varint(id)...  with `inner` the bytes from
// the count on and L = inner + varint_len(inner + varint_len(inner)) (pack.rs:522-525). A record
// that keeps nothing gets no bytes. Indexes lie back to back in record order.
//
// Positions of different records may hold the same Id, so the distinct-test is on the pair: an
// open-addressing table (linear probing) keyed by record << 32 | Id with a parallel word for the
// lowest position that holds the key. The table is the ctx's own buffer, 12 bytes per slot, a
// power of two >= 2 * positions slots, set to all ones by one hipMemsetAsync per call (no key is
// all ones: a record index is below 2^32 - 1).
//
// Passes, separate launches, none of which waits on another workgroup:
//   claim  one lane per position: its record (the block's first and last by wave_lower_bound over
//          seg_off, bisection between them), its Id (translated through arch_id_of_sub or taken as
//          it is; the lowest position with an Id >= 2^32 by one atomicMax), the key's slot by
//          compare-and-swap, atomicMin of the position into the slot's minimum.
//   first  a position is a first occurrence iff its slot's minimum is its own: a byte per position
//          (vl(Id), 0: not a first) and the firsts and their bytes per block of AIX_KEYS_PER_BLOCK.
//   top    two levels: each workgroup scans AIX_TOP_WIDTH block sums, one workgroup the groups'.
//   seg    one wave per record boundary: the firsts and their bytes in front of seg_off[c].
//   plan   one workgroup over the records: idx_ids, L, the widths of varint(L) varint(count) and
//          their scan, idx_off, the seg_off and MAX_VEC checks, the totals and the verdict head.ok.
//   emit   gated on head.ok, tiles of AIX_KEYS_PER_TILE positions, one lane per position. A record's
//          first first-occurrence carries varint(L) varint(count) in front of its Id, so a tile's
//          bytes are one contiguous range: staged in LDS at the output's 16-byte phase and stored
//          as aligned 16-byte blocks (bytes at both edges).
//
// ---- the scan -----------------------------------------------------------------------------------
// Up to the first error a varint of the index body starts at the body's first byte or right after
// a byte < 0x80, so every lane decides its own 16-byte block: the starts from the top bits (the
// block before's last top bit by DPP), up to 10 bytes decoded from each start (the block after by
// DPP), the Id truncated to 32 bits and looked up in `keep`. The lowest start that hits or fails
// wins, by one atomicMin on the record's result word of (offset << 2 | code). One wave per piece of
// AIX_PIECE_BYTES bytes of a record; every wave decodes the record's length varint itself.
#include "nxg_device.h"
#include "nxg_archive_index.h"

namespace {

constexpr int AIX_KEYS_PER_BLOCK = 256;  // claim / first kernels: positions per workgroup and block sum
constexpr int AIX_KEYS_PER_TILE = 512;   // emit kernel: positions per workgroup
constexpr int AIX_LEAD_MAX = 10;         // varint(L) varint(count): 5 + 5 bytes at the most
constexpr int AIX_STAGING_BYTES = AIX_KEYS_PER_TILE * (5 + AIX_LEAD_MAX);  // emit kernel: LDS staging
constexpr int AIX_TOP_WIDTH = 1024;      // block sums per workgroup of the first top kernel
constexpr int AIX_MIN_SLOT_BITS = 10;    // the table's smallest size
constexpr uint64_t AIX_HASH_MUL = 0x9E3779B97F4A7C15ull;  // slot = (key * AIX_HASH_MUL) >> (64 - slot_bits)
constexpr int AIX_PIECE_BYTES = 4096;    // scan kernel: bytes of an index per wave
constexpr int AIX_SCAN_BLOCK = 16;       // scan kernel: bytes per lane and step
constexpr int AIX_BLOCKS_PER_TILE = AIX_KEYS_PER_TILE / AIX_KEYS_PER_BLOCK;
static_assert(AIX_KEYS_PER_TILE % AIX_KEYS_PER_BLOCK == 0, "a tile starts at a block");
static_assert(AIX_TOP_WIDTH % AIX_BLOCKS_PER_TILE == 0, "a tile lies in one group of blocks");
static_assert(AIX_STAGING_BYTES % 16 == 0, "staging in 16-byte blocks");
static_assert(AIX_PIECE_BYTES % (64 * AIX_SCAN_BLOCK) == 0, "a piece is whole wave steps");
constexpr unsigned long long AIX_EMPTY = ~0ull;

// exclusive scan over the NT threads of a workgroup; tmp: NT / 64 + 1 words of LDS
template <int NT>
NXG_DEV uint64_t wg_scan(uint64_t v, uint64_t* tmp, uint64_t* total) {
    constexpr uint32_t NW = NT / 64;
    static_assert(NW <= 64, "the waves' sums are scanned by one wave");
    const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint64_t inc = wave_incl_scan<uint64_t>(v);
    if (l == 63) tmp[w] = inc;
    __syncthreads();
    if (w == 0) {
        const uint64_t x = l < NW ? tmp[l] : 0;
        const uint64_t xi = wave_incl_scan<uint64_t>(x);
        if (l < NW) tmp[l] = xi - x;
        if (l == 63) tmp[NW] = xi;
    }
    __syncthreads();
    const uint64_t wbase = tmp[w];
    *total = tmp[NW];
    __syncthreads();
    return wbase + inc - v;
}

// The positions that belong to a record: [seg_off[0], seg_off[n_recs]), clamped to the keys there
// are (a seg_off past them is refused by the plan kernel).
NXG_DEV bool aix_active(const NxgAixArgs& A, uint64_t p) {
    return p < A.n_keys && p >= A.seg_off[0] && p < A.seg_off[A.n_recs];
}

// The Id of the active position p. false: not kept (no archive Id, or an Id >= 2^32: *wide).
NXG_DEV bool aix_id(const NxgAixArgs& A, uint64_t p, uint32_t* id, bool* wide) {
    const uint64_t k = A.key[p];
    *wide = false;
    if (!A.translate) {
        *id = (uint32_t)k;
        *wide = k > 0xFFFFFFFFull;
        return !*wide;
    }
    if (k >= A.n_subs) return false;
    *id = A.arch_id_of_sub[k];
    return *id != NXG_NO_SLOT;
}

NXG_DEV uint32_t put_var(uint8_t* o, uint32_t p, uint64_t v) {
    while (v >= 0x80) {
        o[p++] = (uint8_t)((v & 0x7f) | 0x80);
        v >>= 7;
    }
    o[p++] = (uint8_t)v;
    return p;
}

}  // namespace

__global__ __launch_bounds__(AIX_KEYS_PER_BLOCK) void nxg_aix_claim_kernel(NxgAixArgs A) {
    __shared__ uint64_t sh_c[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t p0 = (uint64_t)blockIdx.x * AIX_KEYS_PER_BLOCK, p = p0 + tid;
    const uint64_t p1 = p0 + AIX_KEYS_PER_BLOCK < A.n_keys ? p0 + AIX_KEYS_PER_BLOCK : A.n_keys;
    // the records of the block's first and last position: position x is in record c iff seg_off[c]
    // <= x < seg_off[c + 1], i.e. c = the first k with seg_off[k + 1] > x
    if (tid < 128) {
        const uint64_t x = tid < 64 ? p0 : p1 - 1;
        uint64_t cx = wave_lower_bound(A.seg_off + 1, A.n_recs, x + 1);
        if (cx >= A.n_recs) cx = A.n_recs - 1;
        if (lane == 0) sh_c[tid >> 6] = cx;
    }
    __syncthreads();
    if (p >= A.n_keys) return;
    uint32_t id = 0, slot = kAixNoSlot;
    bool wide = false;
    uint64_t lo = 0;
    if (aix_active(A, p) && aix_id(A, p, &id, &wide)) {
        uint64_t hi = sh_c[1];  // the position's record is in [lo, hi]
        lo = sh_c[0];
        if (lo > hi) lo = hi;  // (only under a seg_off that decreases)
#pragma unroll 1
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (A.seg_off[mid + 1] > p) hi = mid;
            else lo = mid + 1;
        }
        const unsigned long long k = (unsigned long long)lo << 32 | id;
        const uint32_t mask = (1u << A.slot_bits) - 1u;
        uint32_t h = (uint32_t)((k * AIX_HASH_MUL) >> (64 - A.slot_bits));
        // ends: at most half of the slots are ever taken
#pragma unroll 1
        for (;;) {
            unsigned long long cur =
                __hip_atomic_load(&A.tkey[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == AIX_EMPTY) cur = atomicCAS(&A.tkey[h], AIX_EMPTY, k);
            if (cur == AIX_EMPTY || cur == k) break;
            h = (h + 1) & mask;
        }
        atomicMin(&A.tmin[h], (uint32_t)p);
        slot = h;
    }
    if (wide) atomicMax((unsigned long long*)&A.head->wide_inv, (unsigned long long)~p);
    A.rec[p] = (uint32_t)lo;
    A.slot[p] = slot;
}

__global__ __launch_bounds__(AIX_KEYS_PER_BLOCK) void nxg_aix_first_kernel(NxgAixArgs A) {
    constexpr int NWAVE = AIX_KEYS_PER_BLOCK / 64;
    __shared__ uint64_t red[2][NWAVE];
    const uint64_t p = (uint64_t)blockIdx.x * AIX_KEYS_PER_BLOCK + threadIdx.x;
    uint32_t len = 0;
    if (p < A.n_keys) {
        const uint32_t slot = A.slot[p];
        if (slot != kAixNoSlot && A.tmin[slot] == (uint32_t)p) {
            uint32_t id;
            bool wide;
            aix_id(A, p, &id, &wide);
            len = vl64(id);
        }
        A.len[p] = (uint8_t)len;
    }
    // per block, not one counter that every wave of the grid adds to
    const uint64_t wc = (uint64_t)__popcll(__ballot(len != 0)), wb = wave_sum<uint64_t>(len);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][w] = wc, red[1][w] = wb;
    __syncthreads();
    if (threadIdx.x < 2) {
        uint64_t t = 0;
#pragma unroll
        for (int i = 0; i < NWAVE; i++) t += red[threadIdx.x][i];
        (threadIdx.x ? A.bbytes : A.bcnt)[blockIdx.x] = t;
    }
}

// level 1: the block sums of one group, scanned in place; the group's sums
__global__ __launch_bounds__(AIX_TOP_WIDTH) void nxg_aix_top_kernel(NxgAixArgs A, uint64_t nb) {
    __shared__ uint64_t tmp[AIX_TOP_WIDTH / 64 + 1];
    const uint64_t b = (uint64_t)blockIdx.x * AIX_TOP_WIDTH + threadIdx.x;
    const bool in = b < nb;
    uint64_t tot;
    const uint64_t ec = wg_scan<AIX_TOP_WIDTH>(in ? A.bcnt[b] : 0, tmp, &tot);
    if (in) A.bcnt[b] = ec;
    if (threadIdx.x == 0) A.gcnt[blockIdx.x] = tot;
    const uint64_t eb = wg_scan<AIX_TOP_WIDTH>(in ? A.bbytes[b] : 0, tmp, &tot);
    if (in) A.bbytes[b] = eb;
    if (threadIdx.x == 0) A.gbytes[blockIdx.x] = tot;
}

// level 2: the groups' sums scanned in place (one workgroup), and the totals
__global__ __launch_bounds__(AIX_TOP_WIDTH) void nxg_aix_top2_kernel(NxgAixArgs A, uint64_t ng) {
    __shared__ uint64_t tmp[AIX_TOP_WIDTH / 64 + 1];
    uint64_t cc = 0, cb = 0;
#pragma unroll 1
    for (uint64_t g0 = 0; g0 < ng; g0 += AIX_TOP_WIDTH) {
        const uint64_t g = g0 + threadIdx.x;
        const bool in = g < ng;
        uint64_t tot;
        const uint64_t ec = wg_scan<AIX_TOP_WIDTH>(in ? A.gcnt[g] : 0, tmp, &tot);
        if (in) A.gcnt[g] = cc + ec;
        cc += tot;
        const uint64_t eb = wg_scan<AIX_TOP_WIDTH>(in ? A.gbytes[g] : 0, tmp, &tot);
        if (in) A.gbytes[g] = cb + eb;
        cb += tot;
    }
    if (threadIdx.x == 0) {
        A.head->n_ids = cc;
        A.head->id_bytes = cb;
    }
}

// one wave per boundary k <= n_recs: the firsts in front of position seg_off[k] (clamped to the
// positions there are)
__global__ __launch_bounds__(256) void nxg_aix_seg_kernel(NxgAixArgs A) {
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k > A.n_recs) return;
    const uint32_t lane = lane_id();
    const uint64_t e = A.seg_off[k];
    uint64_t cnt, by;
    if (e >= A.n_keys) {
        cnt = A.head->n_ids;
        by = A.head->id_bytes;
    } else {
        const uint64_t b = e / AIX_KEYS_PER_BLOCK;
        uint64_t pc = 0, pb = 0;
#pragma unroll 1
        for (uint64_t i = b * AIX_KEYS_PER_BLOCK + lane; i < e; i += 64) {
            const uint32_t l = A.len[i];
            pc += l != 0;
            pb += l;
        }
        cnt = A.bcnt[b] + A.gcnt[b / AIX_TOP_WIDTH] + wave_sum<uint64_t>(pc);
        by = A.bbytes[b] + A.gbytes[b / AIX_TOP_WIDTH] + wave_sum<uint64_t>(pb);
    }
    if (lane == 0) {
        A.ccnt[k] = cnt;
        A.cbytes[k] = by;
    }
}

// the records' indexes laid out, everything checked, the verdict (one workgroup)
__global__ __launch_bounds__(AIX_TOP_WIDTH) void nxg_aix_plan_kernel(NxgAixArgs A) {
    __shared__ uint64_t tmp[AIX_TOP_WIDTH / 64 + 1];
    __shared__ uint32_t sh_bad, sh_vec;
    if (threadIdx.x == 0) sh_bad = sh_vec = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t nc = A.n_recs;
    uint64_t hdr = 0;  // lead bytes of the records before this step's
#pragma unroll 1
    for (uint64_t c0 = 0; c0 < nc; c0 += AIX_TOP_WIDTH) {
        const uint64_t c = c0 + threadIdx.x;
        const bool in = c < nc;
        uint64_t ids = 0, cb = 0, by = 0, L = 0;
        if (in) {
            const uint64_t lo = A.seg_off[c], hi = A.seg_off[c + 1];
            if (hi < lo || (c == nc - 1 && hi > A.n_keys)) atomicMin(&sh_bad, (uint32_t)c);
            cb = A.ccnt[c];
            by = A.cbytes[c];
            const uint64_t ce = A.ccnt[c + 1], be = A.cbytes[c + 1];
            ids = ce > cb ? ce - cb : 0;
            if (ids > kAixMaxVecIds) atomicMin(&sh_vec, (uint32_t)c);
            if (ids) L = lwlen(vl64(ids) + (be > by ? be - by : 0));
        }
        const uint64_t width = ids ? vl64(L) + vl64(ids) : 0;  // varint(L) varint(count)
        uint64_t tot;
        const uint64_t hx = hdr + wg_scan<AIX_TOP_WIDTH>(width, tmp, &tot);
        if (in) {
            A.idx_off[c] = by + hx;
            A.idx_ids[c] = ids;
            A.cinfo[3 * c] = cb;
            A.cinfo[3 * c + 1] = (hx + width) | (width << 60);
            A.cinfo[3 * c + 2] = L;
        }
        hdr += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NxgAixHead* h = A.head;
        const uint64_t nbytes = A.cbytes[nc] + hdr;
        A.idx_off[nc] = nbytes;
        h->n_bytes = nbytes;
        h->seg_bad = sh_bad + 1u;
        h->vec_bad = sh_vec + 1u;
        h->ok = A.out && !h->wide_inv && sh_bad == 0xFFFFFFFFu && sh_vec == 0xFFFFFFFFu &&
                nbytes <= A.cap;
    }
}

__global__ __launch_bounds__(AIX_KEYS_PER_TILE) void nxg_aix_emit_kernel(NxgAixArgs A) {
    constexpr int NT = AIX_KEYS_PER_TILE, NWAVE = NT / 64;
    __shared__ __attribute__((aligned(16))) uint8_t stg[AIX_STAGING_BYTES + 32];
    __shared__ uint64_t tmp[NWAVE + 1];
    __shared__ uint64_t sh_t;
    if (!A.head->ok) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t p = (uint64_t)blockIdx.x * NT + tid;
    const uint32_t len = p < A.n_keys ? A.len[p] : 0u;
    const bool first = len != 0;
    uint64_t ctot;
    const uint64_t ce = wg_scan<NT>(first ? 1 : 0, tmp, &ctot);
    if (ctot == 0) return;
    const uint64_t b0 = (uint64_t)blockIdx.x * AIX_BLOCKS_PER_TILE;
    uint32_t id = 0, lead = 0;
    uint64_t hdr_incl = 0, L = 0, count = 0;
    if (first) {
        const uint64_t c = A.rec[p];
        const uint64_t before = A.bcnt[b0] + A.gcnt[b0 / AIX_TOP_WIDTH] + ce;
        const uint64_t inf = A.cinfo[3 * c + 1];
        hdr_incl = inf & ((1ull << 60) - 1);
        if (before == A.cinfo[3 * c]) {  // the record's first Id
            lead = (uint32_t)(inf >> 60);
            L = A.cinfo[3 * c + 2];
            count = A.idx_ids[c];
        }
        bool wide;
        aix_id(A, p, &id, &wide);
    }
    uint64_t tot;
    const uint64_t off = wg_scan<NT>(first ? (uint64_t)len + lead : 0, tmp, &tot);
    if (first && ce == 0)  // the tile's first Id: nothing of the tile is written before it
        sh_t = A.bbytes[b0] + A.gbytes[b0 / AIX_TOP_WIDTH] + hdr_incl - lead;
    __syncthreads();
    const uint64_t tbase = sh_t;  // the tile's bytes are out[tbase, tbase + tot), tot <= the staging
    const uint32_t phase = (uint32_t)(((uintptr_t)A.out + tbase) & 15u);
    if (first) {
        uint32_t w = phase + (uint32_t)off;
        if (lead) {
            w = put_var(stg, w, L);
            w = put_var(stg, w, count);
        }
        put_var(stg, w, id);
    }
    __syncthreads();
    // staging block b is the 16 bytes at the aligned address out + tbase - phase + 16 b
    uint8_t* const g0 = reinterpret_cast<uint8_t*>((uintptr_t)A.out + tbase - phase);
    const uint32_t end = phase + (uint32_t)tot, nblk = (end + 15) >> 4;
    for (uint32_t b = tid; b < nblk; b += NT) {
        if (16 * b >= phase && 16 * b + 16 <= end) {
            *reinterpret_cast<uint4*>(g0 + 16ull * b) = *reinterpret_cast<const uint4*>(stg + 16 * b);
        } else {
            for (uint32_t k = 16 * b; k < 16 * b + 16; k++)
                if (k >= phase && k < end) g0[k] = stg[k];
        }
    }
}

// ---- the scan -------------------------------------------------------------------------------------
namespace {
// the top bits of a dword's four bytes as bits 0..3
NXG_DEV uint32_t top_bits(uint32_t d) { return nib(d & 0x80808080u); }
// the previous lane's value (lane 0: 0) -- DPP wave_shr:1
NXG_DEV uint32_t wave_prev(uint32_t v) { return dpp0<0x138, 0xf>(v); }
}  // namespace

__global__ __launch_bounds__(256) void nxg_aix_scan_kernel(
    const uint8_t* dbuf, const uint64_t* off, const uint64_t* end, const uint64_t* pbase,
    uint32_t n, uint64_t n_pieces, const uint8_t* keep, uint64_t n_ids, unsigned long long* res) {
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_pieces) return;
    const uint32_t lane = lane_id();
    // the wave's record: the first i with pbase[i + 1] > w
    const uint64_t i = wave_lower_bound(pbase + 1, n, w + 1);
    if (i >= n) return;
    const uint64_t piece = w - pbase[i];
    const uint64_t o = off[i], e = end[i];
    // index_len = decode_varint (pack.rs:504-520) over the record's bytes
    uint64_t index_len = 0;
    uint32_t used = 0, code = NXG_INDEX_ERR_FORMAT;
#pragma unroll 1
    for (uint32_t k = 0; k < 10; k++) {
        if (o + k >= e) {
            code = NXG_INDEX_ERR_SHORT;
            break;
        }
        const uint32_t b = dbuf[o + k];
        index_len |= (uint64_t)(b & 0x7f) << (7 * k);
        if (b < 0x80) {
            used = k + 1;
            code = index_len ? 0u : (uint32_t)NXG_INDEX_ERR_FORMAT;  // (0 underflows in the reference)
            break;
        }
    }
    if (code) {
        if (piece == 0 && lane == 0) atomicMin(&res[i], (unsigned long long)code);
        return;
    }
    // the body: index_len - varint_len(index_len) bytes behind the bytes consumed, clipped at the
    // record's end (Buf::take)
    const uint64_t blen = index_len - vl64(index_len), bs = o + used;
    const uint64_t be = blen > e - bs ? e : bs + blen;
    const uintptr_t base = (uintptr_t)dbuf, lo_a = base + bs, hi_a = base + be;
    const uintptr_t pa = (lo_a & ~(uintptr_t)15) + piece * AIX_PIECE_BYTES;
    uint32_t carry = 0;  // the top bit of the byte in front of lane 0's block
    if (pa > lo_a && pa < hi_a) carry = *reinterpret_cast<const uint8_t*>(pa - 1) >> 7;
#pragma unroll 1
    for (uint32_t it = 0; it < AIX_PIECE_BYTES / (64 * AIX_SCAN_BLOCK); it++) {
        const uintptr_t wa = pa + (uintptr_t)it * 64 * AIX_SCAN_BLOCK;
        if (wa >= hi_a) break;
        // an aligned block that holds a byte of the body lies in the body's pages
        const uintptr_t a = wa + lane * AIX_SCAN_BLOCK;
        uint4 own = make_uint4(0, 0, 0, 0);
        if (a < hi_a) own = *reinterpret_cast<const uint4*>(a);
        uint4 nxt = make_uint4(wave_next(own.x), wave_next(own.y), wave_next(own.z), wave_next(own.w));
        if (lane == 63 && a + 16 < hi_a) nxt = *reinterpret_cast<const uint4*>(a + 16);
        const uint32_t c16 = top_bits(own.x) | top_bits(own.y) << 4 | top_bits(own.z) << 8 |
                             top_bits(own.w) << 12;
        const uint32_t cont = c16 | (top_bits(nxt.x) | top_bits(nxt.y) << 4 | top_bits(nxt.z) << 8 |
                                     top_bits(nxt.w) << 12) << 16;
        uint32_t prev = wave_prev(c16 >> 15);
        if (lane == 0) prev = carry;
        // the block's bytes inside the body, and the varint starts among them
        const uint32_t k_lo = a < lo_a ? (uint32_t)(lo_a - a) : 0u;
        const uint32_t k_hi = a >= hi_a ? 0u : (hi_a - a < 16 ? (uint32_t)(hi_a - a) : 16u);
        const uint32_t valid = k_hi > k_lo ? ((1u << k_hi) - 1u) & ~((1u << k_lo) - 1u) : 0u;
        uint32_t starts = valid & ~(c16 << 1 | prev);
        if (a <= lo_a && lo_a < a + 16 && lo_a < hi_a) starts |= 1u << k_lo;  // the body's first byte
        const uint64_t q0 = own.x | (uint64_t)own.y << 32, q1 = own.z | (uint64_t)own.w << 32;
        const uint64_t q2 = nxt.x | (uint64_t)nxt.y << 32;
        unsigned long long found = AIX_EMPTY;
#pragma unroll 1
        while (starts) {
            const uint32_t k = (uint32_t)__builtin_ctz(starts);
            starts &= starts - 1;
            const uint64_t rem = hi_a - (a + k);  // bytes of the body from the start on
            const uint32_t nc = (uint32_t)__builtin_ctz(~(cont >> k));  // continuation bytes
            uint32_t c = 0;
            if (nc >= 10) {
                c = rem >= 10 ? NXG_INDEX_ERR_FORMAT : NXG_INDEX_ERR_SHORT;
            } else if (nc >= rem) {
                c = NXG_INDEX_ERR_SHORT;
            } else {
                // bytes k .. k + 7 of the 24 at hand; the Id is the low 32 bits of the value
                const uint64_t ql = k < 8 ? q0 : q1, qh = k < 8 ? q1 : q2;
                const uint32_t sh = 8 * (k & 7);
                uint64_t x = sh ? ql >> sh | qh << (64 - sh) : ql;
                if (nc < 4) x &= (1ull << (8 * (nc + 1))) - 1;
                const uint32_t v = (uint32_t)(x & 0x7f) | (uint32_t)(x >> 8 & 0x7f) << 7 |
                                   (uint32_t)(x >> 16 & 0x7f) << 14 |
                                   (uint32_t)(x >> 24 & 0x7f) << 21 | (uint32_t)(x >> 32 & 0x7f) << 28;
                if (v < n_ids && keep[v]) c = NXG_INDEX_MATCH;
            }
            if (c) {
                found = (unsigned long long)(a + k - (base + o)) << 2 | c;
                break;
            }
        }
        if (found != AIX_EMPTY) atomicMin(&res[i], found);
        if (__any(found != AIX_EMPTY)) break;  // nothing behind it can be lower
        carry = (uint32_t)__builtin_amdgcn_readlane((int)(c16 >> 15), 63);
    }
}

// ---- launch (host) ------------------------------------------------------------------------------
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

uint64_t aix_layout(NxgAixArgs& a, uint8_t* p, uint64_t n_keys, uint32_t n_recs) {
    const uint64_t nb = (n_keys + AIX_KEYS_PER_BLOCK - 1) / AIX_KEYS_PER_BLOCK;
    const uint64_t ng = (nb + AIX_TOP_WIDTH - 1) / AIX_TOP_WIDTH;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgAixHead*>(take(256));
    a.rec = reinterpret_cast<uint32_t*>(take(4 * n_keys));
    a.slot = reinterpret_cast<uint32_t*>(take(4 * n_keys));
    a.len = take(n_keys);
    a.bcnt = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.bbytes = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.gcnt = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.gbytes = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.ccnt = reinterpret_cast<uint64_t*>(take(8 * ((uint64_t)n_recs + 1)));
    a.cbytes = reinterpret_cast<uint64_t*>(take(8 * ((uint64_t)n_recs + 1)));
    a.cinfo = reinterpret_cast<uint64_t*>(take(24 * (uint64_t)n_recs));
    return o;
}
}  // namespace

uint32_t nxg_aix_slot_bits(uint64_t n_keys) {
    uint32_t b = AIX_MIN_SLOT_BITS;
    while ((1ull << b) < 2 * n_keys) b++;
    return b;
}

uint64_t nxg_aix_table_bytes(uint32_t slot_bits) { return 12ull << slot_bits; }

uint64_t nxg_aix_scratch_bytes(uint64_t n_keys, uint32_t n_recs) {
    NxgAixArgs a{};
    return aix_layout(a, nullptr, n_keys, n_recs);
}

// 0 < n_keys <= kAixMaxKeys, n_recs > 0
hipError_t nxg_launch_aix_index(NxgAixArgs a, uint8_t* scratch, uint8_t* table, hipStream_t s) {
    const uint64_t n = a.n_keys;
    if (n == 0 || n > kAixMaxKeys || a.n_recs == 0) return hipErrorInvalidValue;
    aix_layout(a, scratch, n, a.n_recs);
    a.slot_bits = nxg_aix_slot_bits(n);
    a.tkey = reinterpret_cast<unsigned long long*>(table);
    a.tmin = reinterpret_cast<uint32_t*>(table + (8ull << a.slot_bits));
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgAixHead), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(table, 0xFF, nxg_aix_table_bytes(a.slot_bits), s);
    if (e != hipSuccess) return e;
    const uint64_t nb = (n + AIX_KEYS_PER_BLOCK - 1) / AIX_KEYS_PER_BLOCK;
    const uint64_t ng = (nb + AIX_TOP_WIDTH - 1) / AIX_TOP_WIDTH;
    const uint64_t nt = (n + AIX_KEYS_PER_TILE - 1) / AIX_KEYS_PER_TILE;
    hipLaunchKernelGGL(nxg_aix_claim_kernel, dim3((uint32_t)nb), dim3(AIX_KEYS_PER_BLOCK), 0, s, a);
    hipLaunchKernelGGL(nxg_aix_first_kernel, dim3((uint32_t)nb), dim3(AIX_KEYS_PER_BLOCK), 0, s, a);
    hipLaunchKernelGGL(nxg_aix_top_kernel, dim3((uint32_t)ng), dim3(AIX_TOP_WIDTH), 0, s, a, nb);
    hipLaunchKernelGGL(nxg_aix_top2_kernel, dim3(1), dim3(AIX_TOP_WIDTH), 0, s, a, ng);
    const uint64_t nk = ((uint64_t)a.n_recs + 1 + 3) / 4;
    hipLaunchKernelGGL(nxg_aix_seg_kernel, dim3((uint32_t)nk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(nxg_aix_plan_kernel, dim3(1), dim3(AIX_TOP_WIDTH), 0, s, a);
    if (a.out)
        hipLaunchKernelGGL(nxg_aix_emit_kernel, dim3((uint32_t)nt), dim3(AIX_KEYS_PER_TILE), 0, s, a);
    return hipGetLastError();
}

uint64_t nxg_aix_scan_pieces(uintptr_t dbuf, uint64_t off, uint64_t end) {
    const uintptr_t lo = (dbuf + off) & ~(uintptr_t)15, hi = dbuf + end;
    const uint64_t span = hi > lo ? hi - lo : 0;
    const uint64_t np = (span + AIX_PIECE_BYTES - 1) / AIX_PIECE_BYTES;
    return np ? np : 1;
}

hipError_t nxg_launch_aix_scan(const uint8_t* dbuf, const uint64_t* off, const uint64_t* end,
                               const uint64_t* pbase, uint32_t n, uint64_t n_pieces,
                               const uint8_t* keep, uint64_t n_ids, unsigned long long* res,
                               hipStream_t s) {
    const uint64_t nwg = (n_pieces + 3) / 4;
    if (nwg == 0 || nwg >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nxg_aix_scan_kernel, dim3((uint32_t)nwg), dim3(256), 0, s, dbuf, off, end,
                       pbase, n, n_pieces, keep, n_ids, res);
    return hipGetLastError();
}
