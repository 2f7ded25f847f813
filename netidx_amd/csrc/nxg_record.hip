// nxg_record.hip -- a dispatch's entries as archive batch records (nxg_record_entries).
//
// Replaces the recorder's batch loop (netidx-archive/src/recorder/record.rs:307-347): each entry
// (SubId, row) of channel c is translated through by_subid (arch_id_of_sub), dropped when it has
// no archive Id, and otherwise becomes the item varint(Id) Event of the channel's record
//     varint(items) item item ...          (<Vec<BatchItem> as Pack>::encode, pack.rs:941-952)
// with Event = 0x40 for Unsubscribed, else the bare Value (logfile/mod.rs:188-205). A channel that
// keeps nothing gets no bytes (writer.rs:405). Records lie back to back in channel order.
//
// Passes, separate launches, none of which waits on another workgroup:
//   size   one lane per entry: the keep flag and the item's length, vl(Id) + |Event|. Scalars and
//          text from the row, flat arrays in registers, everything else one lane at a time on the
//          wave's LDS stack. The walk is nxg_record_walk.h's (nxgenc::value_len does not bound
//          child ranges; this call promises to). A u32 length per entry (0: not kept), and the kept
//          count and bytes per block of REC_ENTRIES_PER_BLOCK entries. The lowest refused entry
//          and its cause by one atomicMax.
//   top    two levels: each workgroup scans REC_TOP_WIDTH block sums, one workgroup the groups'.
//   chan   one wave per channel boundary: the kept entries and item bytes in front of entry
//          chan_off[c] (block prefix + the partial block from the length array).
//   plan   one workgroup over the channels: rec_items, the count varints' widths and their scan,
//          rec_off, the chan_off and MAX_VEC checks, the totals and the verdict head.ok.
//   emit   gated on head.ok, tiles of REC_ENTRIES_PER_TILE entries, one lane per entry. The tile's
//          channels from wave_lower_bound over chan_off, each entry's by bisection between them.
//          The first kept entry of a channel carries the channel's count varint in front of its
//          item, so a tile's bytes are one contiguous range: staged in LDS at the output's 16-byte
//          phase and stored as aligned 16-byte blocks (bytes at both edges), or, when they exceed
//          the staging, written straight to the output.
#include "nxg_device.h"
#include "nxg_record.h"
#include "nxg_record_walk.h"

namespace {

using namespace nxgrec;  // the value walk, the scan and the writer (nxg_record_walk.h)

constexpr int REC_ENTRIES_PER_BLOCK = 256;  // size kernel: entries per workgroup and per block sum
constexpr int REC_ENTRIES_PER_TILE = 512;   // emit kernel: entries per workgroup
constexpr int REC_STAGING_BYTES = 14336;    // emit kernel: LDS staging (28 bytes per entry)
constexpr int REC_TOP_WIDTH = 1024;         // block sums per workgroup of the first top kernel
constexpr int REC_BLOCKS_PER_TILE = REC_ENTRIES_PER_TILE / REC_ENTRIES_PER_BLOCK;
static_assert(REC_ENTRIES_PER_TILE % REC_ENTRIES_PER_BLOCK == 0, "a tile starts at a block");
static_assert(REC_TOP_WIDTH % REC_BLOCKS_PER_TILE == 0, "a tile lies in one group of blocks");
static_assert(REC_STAGING_BYTES % 16 == 0, "staging in 16-byte blocks");

NXG_DEV void refuse(NxgRecHead* h, uint64_t entry, uint32_t cause) {
    atomicMax((unsigned long long*)&h->err_inv, (unsigned long long)((~entry << 8) | cause));
}

// what the emit kernel knows of one kept entry
struct Item {
    uint64_t row;    // ent_row[e]
    uint64_t count;  // lead: the channel's item count
    uint32_t arch;
    uint32_t lead;   // bytes of the count varint in front of the item (0: not the channel's first)
};

// The item (and the channel's count in front of it) at w. Called by every lane of the workgroup
// (`kept` false: nothing written), since the stack walk takes the wave's lanes in turn.
NXG_DEV void emit_item(const NxgRecArgs& A, bool kept, const Item& it, Wr& w, WalkStack* stk) {
    if (kept) {
        if (it.lead) w.var(it.count);
        w.var(it.arch);
    }
    emit_event(A.cols, A.heap, kept, (it.row & NXG_ENT_SPAN) != 0, it.row, w, stk);
}

}  // namespace

__global__ __launch_bounds__(REC_ENTRIES_PER_BLOCK) void nxg_rec_size_kernel(NxgRecArgs A) {
    constexpr int NWAVE = REC_ENTRIES_PER_BLOCK / 64;
    __shared__ WalkStack wstk[NWAVE];
    __shared__ uint64_t red[2][NWAVE];
    const ColsDesc& c = A.cols;
    const uint64_t e = (uint64_t)blockIdx.x * REC_ENTRIES_PER_BLOCK + threadIdx.x;
    const bool in = e < A.n_ent && e >= A.chan_off[0];
    uint32_t arch = NXG_NO_SLOT;
    if (in) {
        const uint64_t sub = A.ent_sub[e];
        if (sub < A.n_subs) arch = A.arch_id_of_sub[sub];
    }
    const bool kept = arch != NXG_NO_SLOT;
    const uint64_t row = kept ? A.ent_row[e] : 0;
    uint32_t cause = 0;
    const uint64_t vlen = event_len(c, kept, (row & NXG_ENT_SPAN) != 0, row, &cause,
                                    &wstk[threadIdx.x >> 6]);
    uint64_t len = kept && !cause ? vl64(arch) + vlen : 0;
    if (len > 0xFFFFFFFFull) cause = kRecBig;  // (the bound nxg_encode_archive_batch puts on an item)
    if (cause) {
        refuse(A.head, e, cause);
        len = 0;
    }
    if (e < A.n_ent) A.len[e] = (uint32_t)len;
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
__global__ __launch_bounds__(REC_TOP_WIDTH) void nxg_rec_top_kernel(NxgRecArgs A, uint64_t nb) {
    __shared__ uint64_t tmp[REC_TOP_WIDTH / 64 + 1];
    const uint64_t b = (uint64_t)blockIdx.x * REC_TOP_WIDTH + threadIdx.x;
    const bool in = b < nb;
    uint64_t tot;
    const uint64_t ec = wg_scan<REC_TOP_WIDTH>(in ? A.bcnt[b] : 0, tmp, &tot);
    if (in) A.bcnt[b] = ec;
    if (threadIdx.x == 0) A.gcnt[blockIdx.x] = tot;
    const uint64_t eb = wg_scan<REC_TOP_WIDTH>(in ? A.bbytes[b] : 0, tmp, &tot);
    if (in) A.bbytes[b] = eb;
    if (threadIdx.x == 0) A.gbytes[blockIdx.x] = tot;
}

// level 2: the groups' sums scanned in place (one workgroup), and the totals
__global__ __launch_bounds__(REC_TOP_WIDTH) void nxg_rec_top2_kernel(NxgRecArgs A, uint64_t ng) {
    __shared__ uint64_t tmp[REC_TOP_WIDTH / 64 + 1];
    uint64_t cc = 0, cb = 0;
#pragma unroll 1
    for (uint64_t g0 = 0; g0 < ng; g0 += REC_TOP_WIDTH) {
        const uint64_t g = g0 + threadIdx.x;
        const bool in = g < ng;
        uint64_t tot;
        const uint64_t ec = wg_scan<REC_TOP_WIDTH>(in ? A.gcnt[g] : 0, tmp, &tot);
        if (in) A.gcnt[g] = cc + ec;
        cc += tot;
        const uint64_t eb = wg_scan<REC_TOP_WIDTH>(in ? A.gbytes[g] : 0, tmp, &tot);
        if (in) A.gbytes[g] = cb + eb;
        cb += tot;
    }
    if (threadIdx.x == 0) {
        A.head->n_items = cc;
        A.head->item_bytes = cb;
    }
}

// one wave per boundary k <= n_chans: what is kept in front of entry chan_off[k] (clamped to the
// entries there are: a chan_off past them is refused by the plan kernel)
__global__ __launch_bounds__(256) void nxg_rec_chan_kernel(NxgRecArgs A) {
    const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k > A.n_chans) return;
    const uint32_t lane = lane_id();
    uint64_t e = A.chan_off[k];
    uint64_t cnt, by;
    if (e >= A.n_ent) {
        cnt = A.head->n_items;
        by = A.head->item_bytes;
    } else {
        const uint64_t b = e / REC_ENTRIES_PER_BLOCK;
        uint64_t pc = 0, pb = 0;
#pragma unroll 1
        for (uint64_t i = b * REC_ENTRIES_PER_BLOCK + lane; i < e; i += 64) {
            const uint32_t l = A.len[i];
            pc += l != 0;
            pb += l;
        }
        cnt = A.bcnt[b] + A.gcnt[b / REC_TOP_WIDTH] + wave_sum<uint64_t>(pc);
        by = A.bbytes[b] + A.gbytes[b / REC_TOP_WIDTH] + wave_sum<uint64_t>(pb);
    }
    if (lane == 0) {
        A.ccnt[k] = cnt;
        A.cbytes[k] = by;
    }
}

// the channels' records laid out, everything checked, the verdict (one workgroup)
__global__ __launch_bounds__(REC_TOP_WIDTH) void nxg_rec_plan_kernel(NxgRecArgs A) {
    __shared__ uint64_t tmp[REC_TOP_WIDTH / 64 + 1];
    __shared__ uint32_t sh_bad, sh_vec;
    if (threadIdx.x == 0) sh_bad = sh_vec = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t nc = A.n_chans;
    if (nc == 0 && threadIdx.x == 0 && A.chan_off[0] != A.n_ent) sh_bad = 0;
    uint64_t hdr = 0;  // count-varint bytes of the channels before this step's
#pragma unroll 1
    for (uint64_t c0 = 0; c0 < nc; c0 += REC_TOP_WIDTH) {
        const uint64_t c = c0 + threadIdx.x;
        const bool in = c < nc;
        uint64_t items = 0, cb = 0, by = 0;
        if (in) {
            const uint64_t lo = A.chan_off[c], hi = A.chan_off[c + 1];
            if (hi < lo || (c == nc - 1 && hi != A.n_ent)) atomicMin(&sh_bad, (uint32_t)c);
            cb = A.ccnt[c];
            by = A.cbytes[c];
            const uint64_t ce = A.ccnt[c + 1];
            items = ce > cb ? ce - cb : 0;
            if (items > kMaxVecBytes / kBatchItemSize) atomicMin(&sh_vec, (uint32_t)c);
        }
        const uint64_t width = items ? vl64(items) : 0;
        uint64_t tot;
        const uint64_t hx = hdr + wg_scan<REC_TOP_WIDTH>(width, tmp, &tot);
        if (in) {
            A.rec_off[c] = by + hx;
            A.rec_items[c] = items;
            A.cinfo[2 * c] = cb;
            A.cinfo[2 * c + 1] = (hx + width) | (width << 60);
        }
        hdr += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NxgRecHead* h = A.head;
        const uint64_t nbytes = A.cbytes[nc] + hdr;
        A.rec_off[nc] = nbytes;
        h->n_bytes = nbytes;
        const uint64_t first = A.chan_off[0] < A.n_ent ? A.chan_off[0] : A.n_ent;
        h->n_dropped = A.n_ent - first - h->n_items;
        h->chan_bad = sh_bad + 1u;
        h->vec_bad = sh_vec + 1u;
        h->ok = A.out && !h->err_inv && sh_bad == 0xFFFFFFFFu && sh_vec == 0xFFFFFFFFu &&
                nbytes <= A.cap;
    }
}

__global__ __launch_bounds__(REC_ENTRIES_PER_TILE) void nxg_rec_emit_kernel(NxgRecArgs A) {
    constexpr int NT = REC_ENTRIES_PER_TILE, NWAVE = NT / 64;
    __shared__ __attribute__((aligned(16))) uint8_t stg[REC_STAGING_BYTES + 32];
    __shared__ WalkStack wstk[NWAVE];
    __shared__ uint64_t tmp[NWAVE + 1];
    __shared__ uint64_t sh_c[2], sh_t;
    if (!A.head->ok) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t rt = (uint64_t)blockIdx.x * NT, e = rt + tid;
    const uint64_t r_end = rt + NT < A.n_ent ? rt + NT : A.n_ent;
    const uint32_t len = e < A.n_ent ? A.len[e] : 0u;
    const bool kept = len != 0;
    // the channels of the tile's first and last entry: entry x is in channel c iff chan_off[c] <=
    // x < chan_off[c + 1], i.e. c = the first k with chan_off[k + 1] > x
    if (tid < 128) {
        const uint64_t x = tid < 64 ? rt : r_end - 1;
        const uint64_t cx = wave_lower_bound(A.chan_off + 1, A.n_chans, x + 1);
        if (lane == 0) sh_c[tid >> 6] = cx;
    }
    uint64_t ctot;
    const uint64_t ce = wg_scan<NT>(kept ? 1 : 0, tmp, &ctot);  // (its barriers publish sh_c)
    if (ctot == 0) return;
    Item it{0, 0, 0, 0};
    uint64_t hdr_incl = 0;
    if (kept) {
        uint64_t lo = sh_c[0], hi = sh_c[1];  // the entry's channel is in [lo, hi]
#pragma unroll 1
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (A.chan_off[mid + 1] > e) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t b0 = (uint64_t)blockIdx.x * REC_BLOCKS_PER_TILE;
        const uint64_t before = A.bcnt[b0] + A.gcnt[b0 / REC_TOP_WIDTH] + ce;
        const uint64_t inf = A.cinfo[2 * lo + 1];
        hdr_incl = inf & ((1ull << 60) - 1);
        if (before == A.cinfo[2 * lo]) {  // the channel's first kept entry
            it.lead = (uint32_t)(inf >> 60);
            it.count = A.rec_items[lo];
        }
        it.arch = A.arch_id_of_sub[A.ent_sub[e]];
        it.row = A.ent_row[e];
    }
    uint64_t tot;
    const uint64_t off = wg_scan<NT>(kept ? (uint64_t)len + it.lead : 0, tmp, &tot);
    if (kept && ce == 0) {  // the tile's first kept entry: nothing of the tile is kept before it
        const uint64_t b0 = (uint64_t)blockIdx.x * REC_BLOCKS_PER_TILE;
        sh_t = A.bbytes[b0] + A.gbytes[b0 / REC_TOP_WIDTH] + hdr_incl - it.lead;
    }
    __syncthreads();
    const uint64_t tbase = sh_t;  // the tile's bytes are out[tbase, tbase + tot)
    WalkStack* const stk = &wstk[tid >> 6];
    if (tot > (uint64_t)REC_STAGING_BYTES) {
        Wr w{A.out, tbase + off};
        emit_item(A, kept, it, w, stk);
        return;
    }
    const uint32_t phase = (uint32_t)(((uintptr_t)A.out + tbase) & 15u);
    {
        Wr w{stg, phase + off};
        emit_item(A, kept, it, w, stk);
    }
    __syncthreads();
    store_staged<NT>(A.out + tbase, phase, (uint32_t)tot, stg);
}

// ---- launch (host) ------------------------------------------------------------------------------
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

uint64_t rec_layout(NxgRecArgs& a, uint8_t* p, uint64_t n_ent, uint32_t n_chans) {
    const uint64_t nb = (n_ent + REC_ENTRIES_PER_BLOCK - 1) / REC_ENTRIES_PER_BLOCK;
    const uint64_t ng = (nb + REC_TOP_WIDTH - 1) / REC_TOP_WIDTH;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgRecHead*>(take(256));
    a.len = reinterpret_cast<uint32_t*>(take(4 * n_ent));
    a.bcnt = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.bbytes = reinterpret_cast<uint64_t*>(take(8 * nb));
    a.gcnt = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.gbytes = reinterpret_cast<uint64_t*>(take(8 * ng));
    a.ccnt = reinterpret_cast<uint64_t*>(take(8 * ((uint64_t)n_chans + 1)));
    a.cbytes = reinterpret_cast<uint64_t*>(take(8 * ((uint64_t)n_chans + 1)));
    a.cinfo = reinterpret_cast<uint64_t*>(take(16 * (uint64_t)n_chans));
    return o;
}
}  // namespace

uint64_t nxg_rec_scratch_bytes(uint64_t n_ent, uint32_t n_chans) {
    NxgRecArgs a{};
    return rec_layout(a, nullptr, n_ent, n_chans);
}

// n_ent > 0 (the host answers an empty entry list itself)
hipError_t nxg_launch_record(NxgRecArgs a, uint8_t* scratch, hipStream_t s) {
    const uint64_t n = a.n_ent;
    rec_layout(a, scratch, n, a.n_chans);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgRecHead), s);
    if (e != hipSuccess) return e;
    const uint64_t nb = (n + REC_ENTRIES_PER_BLOCK - 1) / REC_ENTRIES_PER_BLOCK;
    const uint64_t ng = (nb + REC_TOP_WIDTH - 1) / REC_TOP_WIDTH;
    const uint64_t nt = (n + REC_ENTRIES_PER_TILE - 1) / REC_ENTRIES_PER_TILE;
    if (nb == 0 || nb >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nxg_rec_size_kernel, dim3((uint32_t)nb), dim3(REC_ENTRIES_PER_BLOCK), 0, s, a);
    hipLaunchKernelGGL(nxg_rec_top_kernel, dim3((uint32_t)ng), dim3(REC_TOP_WIDTH), 0, s, a, nb);
    hipLaunchKernelGGL(nxg_rec_top2_kernel, dim3(1), dim3(REC_TOP_WIDTH), 0, s, a, ng);
    const uint64_t nk = ((uint64_t)a.n_chans + 1 + 3) / 4;
    hipLaunchKernelGGL(nxg_rec_chan_kernel, dim3((uint32_t)nk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(nxg_rec_plan_kernel, dim3(1), dim3(REC_TOP_WIDTH), 0, s, a);
    if (a.out)
        hipLaunchKernelGGL(nxg_rec_emit_kernel, dim3((uint32_t)nt), dim3(REC_ENTRIES_PER_TILE), 0, s, a);
    return hipGetLastError();
}
