// nxg_oneshot.hip -- the sections of a oneshot reply shard (netidx-archive/src/recorder/
// oneshot.rs:100-157, recorder_client.rs:29-37) that are made on the device.
//
// The pathmap section (nxg_oneshot_pack_pathmap): the filter set and
//     varint(n_sel) { varint(a) varint(len) path bytes }...     (<FxHashMap<Id, Path> as Pack>::
// encode, pack.rs:1113-1124; Id: logfile/mod.rs:154-166; Path: path.rs:61-68 over ArcStr,
// pack.rs:444-455) over the selected Ids in ascending order. Id a is selected iff keep[a] != 0 and
// it has a path (oneshot.rs:113-120: the pathmap holds the matching Ids of the path index).
//
// Passes, separate launches, none of which waits on another workgroup:
//   size   one lane per Id: sel[a] and the item's length vl(a) + vl(len) + len (0: not selected);
//          the selected count and bytes per block of OS_PM_IDS_PER_BLOCK Ids. The lowest Id at
//          which path_off decreases by one atomicMax.
//   top    each workgroup scans OS_PM_TOP_WIDTH block sums in place and leaves its group's sums
//          (nxg_os_top_kernel, which serves both calls).
//   plan   one workgroup: the groups' sums scanned in place, the totals, the MAX_VEC and capacity
//          checks and the verdict head.ok.
//   emit   gated on head.ok, tiles of OS_PM_IDS_PER_TILE Ids, one lane per Id. A tile's bytes are
//          one contiguous range. When no path of the tile is long and the range fits the staging,
//          the items are written to LDS at the output's 16-byte phase and stored as aligned
//          16-byte blocks (bytes at both edges). Otherwise every lane writes its item's two
//          varints and a short path straight to the output, and a path of OS_PM_LONG_PATH bytes
//          or more is copied by its whole wave, 16 bytes per lane and step.
//
// The deltas elements of one window (nxg_oneshot_pack_deltas): oneshot.rs:146-149,
// batch.retain(|BatchItem(id, _)| pathmap.contains_key(id)) and the drop of records that end up
// empty, then per kept record  i64 BE secs, u32 BE nanos  (DateTime<Utc>, pack.rs:1555-1567) and
// varint(items) item...  (<Vec<BatchItem> as Pack>::encode, pack.rs:941-952), item = varint(Id) Event.
// Window row r of a record is kept iff id[r] < n_ids and sel[id[r]] != 0. The passes are those of
// nxg_record.hip (the value walk, the scan and the writer are shared, nxg_record_walk.h) with an
// implicit entry list -- entry = window row, channel = record -- and a lead of 12 bytes plus the
// count varint in front of a record's first kept item:
//   size   one lane per row of [first, first + n): its record by bisection between the records of
//          the block's first and last row, the keep flag, the item's length. A u32 length per row
//          (0: not kept, or in no record) and the kept count and bytes per block. The lowest
//          refused row and its cause by one atomicMax.
//   top    as above; top2: one workgroup scans the groups' sums and leaves the totals.
//   bound  one wave per record boundary k <= n_recs: what is kept in front of row rbeg[k].
//   plan   one workgroup over the records: rec_items, the leads' widths and their scan, rec_off,
//          the MAX_VEC check, the totals and the verdict head.ok.
//   emit   gated on head.ok, tiles of OS_DL_ROWS_PER_TILE rows, one lane per row; staged in LDS
//          at the output's 16-byte phase and stored as aligned 16-byte blocks, or, when the tile's
//          bytes exceed the staging, written straight to the output.
#include "nxg_device.h"
#include "nxg_oneshot.h"
#include "nxg_record_walk.h"

namespace {

using namespace nxgrec;  // the value walk, the scan and the writer

constexpr int OS_PM_IDS_PER_BLOCK = 256;  // size kernel: Ids per workgroup and per block sum
constexpr int OS_PM_IDS_PER_TILE = 256;   // emit kernel: Ids per workgroup
constexpr int OS_PM_STAGING_BYTES = 16384;  // emit kernel: LDS staging (64 bytes per Id)
constexpr int OS_PM_TOP_WIDTH = 1024;     // block sums per workgroup of the top kernel
constexpr int OS_PM_LONG_PATH = 256;      // emit kernel: from this length on the wave copies a path
constexpr int OS_PM_BLOCKS_PER_TILE = OS_PM_IDS_PER_TILE / OS_PM_IDS_PER_BLOCK;
static_assert(OS_PM_IDS_PER_TILE % OS_PM_IDS_PER_BLOCK == 0, "a tile starts at a block");
static_assert(OS_PM_TOP_WIDTH % OS_PM_BLOCKS_PER_TILE == 0, "a tile lies in one group of blocks");
static_assert(OS_PM_STAGING_BYTES % 16 == 0, "staging in 16-byte blocks");

constexpr int OS_DL_ROWS_PER_BLOCK = 256;  // size kernel: rows per workgroup and per block sum
constexpr int OS_DL_ROWS_PER_TILE = 512;   // emit kernel: rows per workgroup
constexpr int OS_DL_STAGING_BYTES = 14336;  // emit kernel: LDS staging (28 bytes per row)
constexpr int OS_DL_TOP_WIDTH = 1024;      // block sums per workgroup of the top kernel
constexpr int OS_DL_BLOCKS_PER_TILE = OS_DL_ROWS_PER_TILE / OS_DL_ROWS_PER_BLOCK;
static_assert(OS_DL_ROWS_PER_TILE % OS_DL_ROWS_PER_BLOCK == 0, "a tile starts at a block");
static_assert(OS_DL_TOP_WIDTH % OS_DL_BLOCKS_PER_TILE == 0, "a tile lies in one group of blocks");
static_assert(OS_DL_STAGING_BYTES % 16 == 0, "staging in 16-byte blocks");
static_assert(OS_DL_TOP_WIDTH == OS_PM_TOP_WIDTH, "one top kernel serves both calls");
constexpr int OS_TOP_WIDTH = OS_PM_TOP_WIDTH;

// n > 0 bytes from src to o[p ...] by one lane: the covering aligned dwords of src (a
// dword-aligned read never leaves the page of the bytes it covers), realigned, written byte by
// byte (o has any alignment)
NXG_DEV void lane_copy(uint8_t* o, uint64_t p, const uint8_t* src, uint64_t n) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t* w = reinterpret_cast<const uint32_t*>((uintptr_t)src & ~(uintptr_t)3);
    const uint64_t nw = (sh + n + 3) >> 2;  // aligned dwords that hold a byte of src
    uint32_t lo = w[0];
#pragma unroll 2
    for (uint64_t i = 0; 4 * i < n; i++) {
        const uint32_t hi = i + 1 < nw ? w[i + 1] : 0u;
        const uint32_t e = __builtin_amdgcn_alignbyte(hi, lo, sh);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (4 * i + k < n) o[p + 4 * i + k] = (uint8_t)(e >> (8 * k));
        lo = hi;
    }
}

// lane l's value, l wave-uniform
NXG_DEV uint64_t lane_value(uint64_t v, uint32_t l) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32);
}

// n bytes from src to dst by the whole wave (arguments wave-uniform): bytes up to dst's first
// 16-byte boundary, then aligned 16-byte stores (1 KiB per step of the wave) of source dwords
// realigned as in lane_copy, then the bytes behind the last whole block. Nothing outside [dst,
// dst + n) is written, and every dword read holds a byte of [src, src + n).
NXG_DEV void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t lane) {
    uint64_t h = (16 - ((uintptr_t)dst & 15u)) & 15u;
    if (h > n) h = n;
    if (lane < h) dst[lane] = src[lane];
    const uint64_t nblk = (n - h) >> 4;
    const uint32_t sh = (uint32_t)((uintptr_t)(src + h) & 3u);
    const uint32_t* w0 = reinterpret_cast<const uint32_t*>((uintptr_t)(src + h) & ~(uintptr_t)3);
#pragma unroll 1
    for (uint64_t b = lane; b < nblk; b += 64) {
        const uint32_t* w = w0 + 4 * b;
        const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3];
        const uint32_t d4 = sh ? w[4] : 0u;  // (source dword-aligned: w[4] holds no byte of the block)
        uint4 e;
        e.x = __builtin_amdgcn_alignbyte(d1, d0, sh);
        e.y = __builtin_amdgcn_alignbyte(d2, d1, sh);
        e.z = __builtin_amdgcn_alignbyte(d3, d2, sh);
        e.w = __builtin_amdgcn_alignbyte(d4, d3, sh);
        *reinterpret_cast<uint4*>(dst + h + 16 * b) = e;
    }
    const uint64_t t0 = h + 16 * nblk;
    if (lane < n - t0) dst[t0 + lane] = src[t0 + lane];
}

}  // namespace

// ---- the pathmap section ------------------------------------------------------------------------
__global__ __launch_bounds__(OS_PM_IDS_PER_BLOCK) void nxg_os_pm_size_kernel(NxgOsPmArgs A) {
    constexpr int NWAVE = OS_PM_IDS_PER_BLOCK / 64;
    __shared__ uint64_t red[2][NWAVE];
    const uint64_t a = (uint64_t)blockIdx.x * OS_PM_IDS_PER_BLOCK + threadIdx.x;
    uint64_t len = 0;
    if (a < A.n_ids) {
        const uint64_t lo = A.path_off[a], hi = A.path_off[a + 1];
        bool s = false;
        if (hi < lo) {
            atomicMax((unsigned long long*)&A.head->bad_inv, (unsigned long long)~a);
        } else {
            s = A.keep[a] != 0 && hi != lo;
            if (s) len = vl64(a) + vl64(hi - lo) + (hi - lo);
        }
        A.sel[a] = s ? 1 : 0;
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

// the block sums of one group, scanned in place; the group's sums (both calls)
__global__ __launch_bounds__(OS_TOP_WIDTH) void nxg_os_top_kernel(uint64_t* bcnt, uint64_t* bbytes,
                                                                  uint64_t* gcnt, uint64_t* gbytes,
                                                                  uint64_t nb) {
    __shared__ uint64_t tmp[OS_TOP_WIDTH / 64 + 1];
    const uint64_t b = (uint64_t)blockIdx.x * OS_TOP_WIDTH + threadIdx.x;
    const bool in = b < nb;
    uint64_t tot;
    const uint64_t ec = wg_scan<OS_TOP_WIDTH>(in ? bcnt[b] : 0, tmp, &tot);
    if (in) bcnt[b] = ec;
    if (threadIdx.x == 0) gcnt[blockIdx.x] = tot;
    const uint64_t eb = wg_scan<OS_TOP_WIDTH>(in ? bbytes[b] : 0, tmp, &tot);
    if (in) bbytes[b] = eb;
    if (threadIdx.x == 0) gbytes[blockIdx.x] = tot;
}

namespace {
// the groups' sums scanned in place by one workgroup of OS_TOP_WIDTH threads; the totals
NXG_DEV void scan_groups(uint64_t* gcnt, uint64_t* gbytes, uint64_t ng, uint64_t* tmp,
                         uint64_t* count, uint64_t* bytes) {
    uint64_t cc = 0, cb = 0;
#pragma unroll 1
    for (uint64_t g0 = 0; g0 < ng; g0 += OS_TOP_WIDTH) {
        const uint64_t g = g0 + threadIdx.x;
        const bool in = g < ng;
        uint64_t tot;
        const uint64_t ec = wg_scan<OS_TOP_WIDTH>(in ? gcnt[g] : 0, tmp, &tot);
        if (in) gcnt[g] = cc + ec;
        cc += tot;
        const uint64_t eb = wg_scan<OS_TOP_WIDTH>(in ? gbytes[g] : 0, tmp, &tot);
        if (in) gbytes[g] = cb + eb;
        cb += tot;
    }
    *count = cc;
    *bytes = cb;
}
}  // namespace

// the groups' sums scanned in place, the totals, the checks and the verdict (one workgroup)
__global__ __launch_bounds__(OS_TOP_WIDTH) void nxg_os_pm_plan_kernel(NxgOsPmArgs A, uint64_t ng) {
    __shared__ uint64_t tmp[OS_TOP_WIDTH / 64 + 1];
    uint64_t cc, cb;
    scan_groups(A.gcnt, A.gbytes, ng, tmp, &cc, &cb);
    if (threadIdx.x == 0) {
        NxgOsPmHead* h = A.head;
        const uint64_t nbytes = vl64(cc) + cb;
        h->n_sel = cc;
        h->item_bytes = cb;
        h->n_bytes = nbytes;
        const bool vec = cc > kMaxVecBytes / kOsPathmapEntrySize;
        h->vec_bad = vec;
        h->ok = A.out && !h->bad_inv && !vec && nbytes <= A.cap;
    }
}

__global__ __launch_bounds__(OS_PM_IDS_PER_TILE) void nxg_os_pm_emit_kernel(NxgOsPmArgs A) {
    constexpr int NT = OS_PM_IDS_PER_TILE, NWAVE = NT / 64;
    __shared__ __attribute__((aligned(16))) uint8_t stg[OS_PM_STAGING_BYTES + 32];
    __shared__ uint64_t tmp[NWAVE + 1];
    if (!A.head->ok) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t a = (uint64_t)blockIdx.x * NT + tid;
    const uint64_t n_sel = A.head->n_sel;
    if (blockIdx.x == 0 && tid == 0) {
        Wr w{A.out, 0};
        w.var(n_sel);
    }
    const bool s = a < A.n_ids && A.sel[a] != 0;
    uint64_t lo = 0, plen = 0;
    if (s) {
        lo = A.path_off[a];
        plen = A.path_off[a + 1] - lo;
    }
    const uint32_t lead = s ? vl64(a) + vl64(plen) : 0u;
    uint64_t tot;
    const uint64_t off = wg_scan<NT>(lead + plen, tmp, &tot);
    if (tot == 0) return;
    const uint64_t b0 = (uint64_t)blockIdx.x * OS_PM_BLOCKS_PER_TILE;
    // the tile's bytes are out[tbase, tbase + tot)
    const uint64_t tbase = vl64(n_sel) + A.bbytes[b0] + A.gbytes[b0 / OS_TOP_WIDTH];
    const bool is_long = s && plen >= (uint64_t)OS_PM_LONG_PATH;
    const bool any_long = __syncthreads_or(is_long) != 0;
    const uint8_t* const src = A.path_bytes + lo;
    if (any_long || tot > (uint64_t)OS_PM_STAGING_BYTES) {
        if (s) {
            Wr w{A.out, tbase + off};
            w.var(a);
            w.var(plen);
            if (!is_long) lane_copy(w.o, w.p, src, plen);
        }
        uint64_t m = __ballot(is_long);
#pragma unroll 1
        while (m) {
            const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            m &= m - 1;
            uint8_t* const d = A.out + lane_value(tbase + off + lead, l);
            const uint8_t* const f = A.path_bytes + lane_value(lo, l);
            wave_copy(d, f, lane_value(plen, l), lane);
        }
        return;
    }
    const uint32_t phase = (uint32_t)(((uintptr_t)A.out + tbase) & 15u);
    if (s) {
        Wr w{stg, phase + off};
        w.var(a);
        w.var(plen);
        lane_copy(w.o, w.p, src, plen);
    }
    __syncthreads();
    store_staged<NT>(A.out + tbase, phase, (uint32_t)tot, stg);
}

// ---- the deltas elements of one window ----------------------------------------------------------
namespace {
// the record of entry e, between the records lo and hi of the first and last entry of its block
// or tile: the first k with rbeg[k + 1] > e
NXG_DEV uint64_t record_of(const uint64_t* rbeg, uint64_t lo, uint64_t hi, uint64_t e) {
#pragma unroll 1
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rbeg[mid + 1] > e) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the records of entries e0 and e1 - 1 to sh_c[0] and sh_c[1], by the first two waves of the
// workgroup (the caller's next barrier publishes them)
NXG_DEV void records_of_ends(const NxgOsDlArgs& A, uint64_t e0, uint64_t e1, uint64_t* sh_c) {
    if (threadIdx.x < 128) {
        const uint64_t x = threadIdx.x < 64 ? e0 : e1 - 1;
        const uint64_t cx = wave_lower_bound(A.rbeg + 1, A.n_recs, x + 1);
        if ((threadIdx.x & 63) == 0) sh_c[threadIdx.x >> 6] = cx;
    }
}
}  // namespace

__global__ __launch_bounds__(OS_DL_ROWS_PER_BLOCK) void nxg_os_dl_size_kernel(NxgOsDlArgs A) {
    constexpr int NWAVE = OS_DL_ROWS_PER_BLOCK / 64;
    __shared__ WalkStack wstk[NWAVE];
    __shared__ uint64_t red[2][NWAVE];
    __shared__ uint64_t sh_c[2];
    const ColsDesc& c = A.cols;
    const uint64_t e0 = (uint64_t)blockIdx.x * OS_DL_ROWS_PER_BLOCK, e = e0 + threadIdx.x;
    const uint64_t e1 = e0 + OS_DL_ROWS_PER_BLOCK < A.n ? e0 + OS_DL_ROWS_PER_BLOCK : A.n;
    records_of_ends(A, e0, e1, sh_c);
    __syncthreads();
    const uint64_t row = A.first + e;
    bool kept = false;
    uint64_t id = 0;
    if (e < A.n) {
        const uint64_t k = record_of(A.rbeg, sh_c[0], sh_c[1], e);
        if (e < A.rend[k]) {  // (else: between two records)
            id = c.id[row];
            kept = id < A.n_ids && A.sel[id] != 0;
        }
    }
    uint32_t cause = 0;
    const uint64_t vlen = event_len(c, kept, false, row, &cause, &wstk[threadIdx.x >> 6]);
    uint64_t len = kept && !cause ? vl64(id) + vlen : 0;
    if (len > 0xFFFFFFFFull) cause = kRecBig;  // (the bound nxg_encode_archive_batch puts on an item)
    if (cause) {
        atomicMax((unsigned long long*)&A.head->err_inv, (unsigned long long)((~row << 8) | cause));
        len = 0;
    }
    if (e < A.n) A.len[e] = (uint32_t)len;
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

// level 2: the groups' sums scanned in place (one workgroup), and the totals
__global__ __launch_bounds__(OS_TOP_WIDTH) void nxg_os_dl_top2_kernel(NxgOsDlArgs A, uint64_t ng) {
    __shared__ uint64_t tmp[OS_TOP_WIDTH / 64 + 1];
    uint64_t cc, cb;
    scan_groups(A.gcnt, A.gbytes, ng, tmp, &cc, &cb);
    if (threadIdx.x == 0) {
        A.head->n_items = cc;
        A.head->item_bytes = cb;
    }
}

// one wave per boundary k <= n_recs: what is kept in front of entry rbeg[k] (rbeg[n_recs] == n)
__global__ __launch_bounds__(256) void nxg_os_dl_bound_kernel(NxgOsDlArgs A) {
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k > A.n_recs) return;
    const uint32_t lane = lane_id();
    const uint64_t e = A.rbeg[k];
    uint64_t cnt, by;
    if (e >= A.n) {
        cnt = A.head->n_items;
        by = A.head->item_bytes;
    } else {
        const uint64_t b = e / OS_DL_ROWS_PER_BLOCK;
        uint64_t pc = 0, pb = 0;
#pragma unroll 1
        for (uint64_t i = b * OS_DL_ROWS_PER_BLOCK + lane; i < e; i += 64) {
            const uint32_t l = A.len[i];
            pc += l != 0;
            pb += l;
        }
        cnt = A.bcnt[b] + A.gcnt[b / OS_TOP_WIDTH] + wave_sum<uint64_t>(pc);
        by = A.bbytes[b] + A.gbytes[b / OS_TOP_WIDTH] + wave_sum<uint64_t>(pb);
    }
    if (lane == 0) {
        A.ccnt[k] = cnt;
        A.cbytes[k] = by;
    }
}

// the records' elements laid out, everything checked, the verdict (one workgroup)
__global__ __launch_bounds__(OS_TOP_WIDTH) void nxg_os_dl_plan_kernel(NxgOsDlArgs A) {
    __shared__ uint64_t tmp[OS_TOP_WIDTH / 64 + 1];
    __shared__ uint32_t sh_vec;
    if (threadIdx.x == 0) sh_vec = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t nc = A.n_recs;
    uint64_t hdr = 0;   // lead bytes of the records before this step's
    uint64_t live = 0;  // records that keep an item
#pragma unroll 1
    for (uint64_t c0 = 0; c0 < nc; c0 += OS_TOP_WIDTH) {
        const uint64_t c = c0 + threadIdx.x;
        const bool in = c < nc;
        uint64_t items = 0, cb = 0, by = 0;
        if (in) {
            cb = A.ccnt[c];
            by = A.cbytes[c];
            items = A.ccnt[c + 1] - cb;
            if (items > kMaxVecBytes / kBatchItemSize) atomicMin(&sh_vec, (uint32_t)c);
        }
        // the timestamp (pack.rs:1555-1567: put_i64, put_u32) and the count varint
        const uint64_t width = items ? 12 + vl64(items) : 0;
        uint64_t tot;
        const uint64_t hx = hdr + wg_scan<OS_TOP_WIDTH>(width, tmp, &tot);
        live += (uint64_t)__syncthreads_count(items != 0);
        if (in) {
            A.rec_off[c] = by + hx;
            A.rec_items[c] = items;
            A.cinfo[2 * c] = cb;
            A.cinfo[2 * c + 1] = (hx + width) | (width << 56);
        }
        hdr += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NxgOsDlHead* h = A.head;
        const uint64_t nbytes = A.cbytes[nc] + hdr;
        A.rec_off[nc] = nbytes;
        h->n_bytes = nbytes;
        h->n_kept_recs = live;
        h->vec_bad = sh_vec + 1u;
        h->ok = A.out && !h->err_inv && sh_vec == 0xFFFFFFFFu && nbytes <= A.cap;
    }
}

__global__ __launch_bounds__(OS_DL_ROWS_PER_TILE) void nxg_os_dl_emit_kernel(NxgOsDlArgs A) {
    constexpr int NT = OS_DL_ROWS_PER_TILE, NWAVE = NT / 64;
    __shared__ __attribute__((aligned(16))) uint8_t stg[OS_DL_STAGING_BYTES + 32];
    __shared__ WalkStack wstk[NWAVE];
    __shared__ uint64_t tmp[NWAVE + 1];
    __shared__ uint64_t sh_c[2], sh_t;
    if (!A.head->ok) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t e0 = (uint64_t)blockIdx.x * NT, e = e0 + tid;
    const uint64_t e1 = e0 + NT < A.n ? e0 + NT : A.n;
    const uint32_t len = e < A.n ? A.len[e] : 0u;
    const bool kept = len != 0;
    records_of_ends(A, e0, e1, sh_c);
    uint64_t ctot;
    const uint64_t ce = wg_scan<NT>(kept ? 1 : 0, tmp, &ctot);  // (its barriers publish sh_c)
    if (ctot == 0) return;
    const uint64_t row = A.first + e;
    uint64_t id = 0, count = 0, secs = 0, hdr_incl = 0;
    uint32_t lead = 0, nanos = 0;  // lead: bytes in front of the item (0: not the record's first)
    if (kept) {
        const uint64_t k = record_of(A.rbeg, sh_c[0], sh_c[1], e);
        const uint64_t b0 = (uint64_t)blockIdx.x * OS_DL_BLOCKS_PER_TILE;
        const uint64_t before = A.bcnt[b0] + A.gcnt[b0 / OS_TOP_WIDTH] + ce;
        const uint64_t inf = A.cinfo[2 * k + 1];
        hdr_incl = inf & ((1ull << 56) - 1);
        if (before == A.cinfo[2 * k]) {  // the record's first kept row
            lead = (uint32_t)(inf >> 56);
            count = A.rec_items[k];
            secs = A.secs[k];
            nanos = (uint32_t)A.nanos[k];
        }
        id = A.cols.id[row];
    }
    uint64_t tot;
    const uint64_t off = wg_scan<NT>(kept ? (uint64_t)len + lead : 0, tmp, &tot);
    if (kept && ce == 0) {  // the tile's first kept row: nothing of the tile is kept before it
        const uint64_t b0 = (uint64_t)blockIdx.x * OS_DL_BLOCKS_PER_TILE;
        sh_t = A.bbytes[b0] + A.gbytes[b0 / OS_TOP_WIDTH] + hdr_incl - lead;
    }
    __syncthreads();
    const uint64_t tbase = sh_t;  // the tile's bytes are out[tbase, tbase + tot)
    WalkStack* const stk = &wstk[tid >> 6];
    auto item = [&](Wr& w) {
        if (kept) {
            if (lead) {
                w.be(secs, 8);
                w.be(nanos, 4);
                w.var(count);
            }
            w.var(id);
        }
        emit_event(A.cols, A.heap, kept, false, row, w, stk);
    };
    if (tot > (uint64_t)OS_DL_STAGING_BYTES) {
        Wr w{A.out, tbase + off};
        item(w);
        return;
    }
    const uint32_t phase = (uint32_t)(((uintptr_t)A.out + tbase) & 15u);
    {
        Wr w{stg, phase + off};
        item(w);
    }
    __syncthreads();
    store_staged<NT>(A.out + tbase, phase, (uint32_t)tot, stg);
}

// ---- launch (host) ------------------------------------------------------------------------------
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

uint64_t pm_layout(NxgOsPmArgs& a, uint8_t* p, uint64_t n_ids) {
    const uint64_t nb = (n_ids + OS_PM_IDS_PER_BLOCK - 1) / OS_PM_IDS_PER_BLOCK;
    const uint64_t ng = (nb + OS_TOP_WIDTH - 1) / OS_TOP_WIDTH;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgOsPmHead*>(take(256));
    a.bcnt = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.bbytes = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.gcnt = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.gbytes = reinterpret_cast<uint64_t*>(take(8 * ng));
    return o;
}
}  // namespace

uint64_t nxg_os_pm_scratch_bytes(uint64_t n_ids) {
    NxgOsPmArgs a{};
    return pm_layout(a, nullptr, n_ids);
}

// n_ids > 0 (the host answers an empty path index itself)
hipError_t nxg_launch_os_pathmap(NxgOsPmArgs a, uint8_t* scratch, hipStream_t s) {
    const uint64_t n = a.n_ids;
    pm_layout(a, scratch, n);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgOsPmHead), s);
    if (e != hipSuccess) return e;
    const uint64_t nb = (n + OS_PM_IDS_PER_BLOCK - 1) / OS_PM_IDS_PER_BLOCK;
    const uint64_t ng = (nb + OS_TOP_WIDTH - 1) / OS_TOP_WIDTH;
    const uint64_t nt = (n + OS_PM_IDS_PER_TILE - 1) / OS_PM_IDS_PER_TILE;
    if (nb == 0 || nb >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nxg_os_pm_size_kernel, dim3((uint32_t)nb), dim3(OS_PM_IDS_PER_BLOCK), 0, s, a);
    hipLaunchKernelGGL(nxg_os_top_kernel, dim3((uint32_t)ng), dim3(OS_TOP_WIDTH), 0, s, a.bcnt,
                       a.bbytes, a.gcnt, a.gbytes, nb);
    hipLaunchKernelGGL(nxg_os_pm_plan_kernel, dim3(1), dim3(OS_TOP_WIDTH), 0, s, a, ng);
    if (a.out)
        hipLaunchKernelGGL(nxg_os_pm_emit_kernel, dim3((uint32_t)nt), dim3(OS_PM_IDS_PER_TILE), 0, s, a);
    return hipGetLastError();
}

namespace {
uint64_t dl_layout(NxgOsDlArgs& a, uint8_t* p, uint64_t n, uint32_t n_recs) {
    const uint64_t nb = (n + OS_DL_ROWS_PER_BLOCK - 1) / OS_DL_ROWS_PER_BLOCK;
    const uint64_t ng = (nb + OS_TOP_WIDTH - 1) / OS_TOP_WIDTH;
    const uint64_t nr = n_recs;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgOsDlHead*>(take(256));
    // one copy up: rbeg[nr + 1], rend[nr], secs[nr], nanos[nr]
    a.rbeg = reinterpret_cast<uint64_t*>(take(8 * (4 * nr + 1)));
    a.rend = a.rbeg ? a.rbeg + nr + 1 : nullptr;
    a.secs = a.rbeg ? a.rend + nr : nullptr;
    a.nanos = a.rbeg ? a.secs + nr : nullptr;
    a.len = reinterpret_cast<uint32_t*>(take(4 * n));
    a.bcnt = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.bbytes = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.gcnt = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.gbytes = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.ccnt = reinterpret_cast<uint64_t*>(take(8 * (nr + 1)));
    a.cbytes = reinterpret_cast<uint64_t*>(take(8 * (nr + 1)));
    a.cinfo = reinterpret_cast<uint64_t*>(take(16 * nr));
    return o;
}
}  // namespace

uint64_t nxg_os_dl_scratch_bytes(uint64_t n, uint32_t n_recs) {
    NxgOsDlArgs a{};
    return dl_layout(a, nullptr, n, n_recs);
}

// n > 0 and n_recs > 0 (the host answers a window without rows itself). `up`: host, 4 * n_recs + 1
// words: the records' first entries and n, their ends, the timestamps' seconds and nanoseconds.
hipError_t nxg_launch_os_deltas(NxgOsDlArgs a, uint8_t* scratch, const uint64_t* up, hipStream_t s) {
    const uint64_t n = a.n;
    if (n == 0 || a.n_recs == 0) return hipErrorInvalidValue;
    dl_layout(a, scratch, n, a.n_recs);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgOsDlHead), s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(a.rbeg, up, 8 * (4 * (uint64_t)a.n_recs + 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    const uint64_t nb = (n + OS_DL_ROWS_PER_BLOCK - 1) / OS_DL_ROWS_PER_BLOCK;
    const uint64_t ng = (nb + OS_TOP_WIDTH - 1) / OS_TOP_WIDTH;
    const uint64_t nt = (n + OS_DL_ROWS_PER_TILE - 1) / OS_DL_ROWS_PER_TILE;
    if (nb >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nxg_os_dl_size_kernel, dim3((uint32_t)nb), dim3(OS_DL_ROWS_PER_BLOCK), 0, s, a);
    hipLaunchKernelGGL(nxg_os_top_kernel, dim3((uint32_t)ng), dim3(OS_TOP_WIDTH), 0, s, a.bcnt,
                       a.bbytes, a.gcnt, a.gbytes, nb);
    hipLaunchKernelGGL(nxg_os_dl_top2_kernel, dim3(1), dim3(OS_TOP_WIDTH), 0, s, a, ng);
    const uint64_t nk = ((uint64_t)a.n_recs + 1 + 3) / 4;
    hipLaunchKernelGGL(nxg_os_dl_bound_kernel, dim3((uint32_t)nk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(nxg_os_dl_plan_kernel, dim3(1), dim3(OS_TOP_WIDTH), 0, s, a);
    if (a.out)
        hipLaunchKernelGGL(nxg_os_dl_emit_kernel, dim3((uint32_t)nt), dim3(OS_DL_ROWS_PER_TILE), 0, s, a);
    return hipGetLastError();
}
