// nxg_route_writes.hip -- a connection's decoded write batch routed on gfx950. Replaces the Write
// and Unsubscribe arms of ClientCtx::handle_batch_inner (netidx/src/publisher/server.rs:497-576)
// and write() (server.rs:171-245) for the rows and control spans nxg_decode_writes produced.
//
// Per Write(id, r, v, wid), row i, in this order (server.rs:201-217):
//   1 "cannot write to unsubscribed value"  cl.subscribed has no id (server.rs:201-202): id >= n_ids,
//     perm_of_id[id] == NXG_NOT_SUBSCRIBED, or an Unsubscribe(id) earlier in the batch
//     (server.rs:562-565 removes it), i.e. a span k with ctl_row[k] <= i
//   2 "write permission denied"             perms lack WRITE = 0x04 (server.rs:203-205, auth.rs:26)
//   3 "writes not accepted"                 no on_write slot, or none of its channels open
//     (server.rs:206-217; the host builds the table from open channels, the retain of 207-214)
//   0 routed: one request per channel of on_write[id] in list order (server.rs:225-240), and
//     (id, wid) onto the wait list when r is set (server.rs:218-224)
// Outcomes 1-3 with r set queue From::WriteResult(id, Error(String(msg)), wid) (server.rs:191-194);
// Unsubscribe(id) always queues From::Unsubscribed(id) (server.rs:565). A row without a WriteId on
// the wire takes fresh_wid + its rank among such rows (WriteId::default() is WriteId::new(),
// netidx-netproto/src/publisher.rs:11-15).
//
// Everything whose place depends on what precedes it comes from block sums scanned by a one-
// workgroup kernel between launches; no kernel waits on another workgroup, and the counts are
// sums of block totals, not shared counters (one atomic per wave on one word cost the classify
// pass 0.40 ms at 10^6 rows, against 0.05 ms for the rows pass). Launches, in order:
//   find      the first Subscribe span at or after ctl_begin (atomicMax of ~k): the call stops there
//   spans     per Unsubscribe span: its Id from the frame, unsub_id[], the first-unsubscribe table
//             (atomicMax of epoch | ~ctl_row: a word of another call's epoch reads as "none", so the
//             table is never cleared), its reply's size and the block sums of the sizes
//   classify  per row: outcome[], the dispatch's row_mode (0 routed, 1 not pushed; rows past the
//             stop: 1), block sums of (rows without a WriteId, rows on the wait list) and of the
//             rows per outcome
//   top       exclusive scans of those block sums, their totals into the head
//   size      per row: its effective WriteId, hence its reply's size; block sums of the sizes and
//             of the replies
//   top       exclusive scan of those
//   rows      WriteResult replies and the wait list. A row's reply sits after the replies of the
//             rows before it and of the spans with ctl_row <= i (ctl_row is sorted: a search)
//   unsubs    Unsubscribed replies: after the spans before it and the rows before ctl_row[k]
//   (the channel fan-out is nxg_launch_dispatch over an NxgSubTable view of the write table)
//   finish    entry rows re-based to the batch, n_entries / next_row / next_ctl into the head
// Wire forms (Value::Error(String) is tag 18, netidx-value/src/lib.rs:437-441):
//   Unsubscribed(id)                       varint(L) 02 varint(id)
//   WriteResult(id, Error(String(m)), wid) varint(L) 06 varint(id) 12 varint(|m|) m varint(wid)
// A body is at most 57 bytes, so L = |body| + 1 is one byte.
#include <algorithm>

#include "nxg_device.h"
#include "nxg_internal.h"

namespace {

constexpr int TPB = kRwBlock;
constexpr uint64_t kRowMask = (1ull << 40) - 1;  // first-unsubscribe word: epoch << 40 | ~row
constexpr uint32_t kWrite = 0x04;                // Permissions::WRITE (resolver_server/auth.rs:26)

// the three messages of or_qwe! (server.rs:201-216), by outcome - 1
__device__ const char kMsg[3][36] = {"cannot write to unsubscribed value", "write permission denied",
                                     "writes not accepted"};
__device__ const uint8_t kMsgLen[3] = {34, 23, 19};

struct Range {
    uint64_t s;        // the first Subscribe span at or after ctl_begin, or n_ctl
    uint64_t row_end;  // rows [row_begin, row_end) are processed
};
NXG_DEV Range range_of(const NxgRwArgs& a) {
    const uint64_t v = a.head->first_sub_inv;
    Range r;
    r.s = v ? ~v : a.n_ctl;
    r.row_end = r.s < a.n_ctl ? a.ctl_row[r.s] : a.n_rows;
    if (r.row_end > a.n_rows) r.row_end = a.n_rows;
    if (r.row_end < a.row_begin) r.row_end = a.row_begin;  // (begins that do not belong together)
    return r;
}

// spans with ctl_row <= row among the call's Unsubscribe spans [ctl_begin, s)
NXG_DEV uint64_t spans_upto(const NxgRwArgs& a, uint64_t n_unsub, uint64_t row) {
    const uint64_t* cr = a.ctl_row + a.ctl_begin;
    uint64_t lo = 0, hi = n_unsub;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cr[mid] <= row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// reply bytes of the first k spans / of the rows before `row`
NXG_DEV uint64_t span_prefix(const NxgRwArgs& a, uint64_t n_unsub, uint64_t k) {
    return k < n_unsub ? a.sblk[k / TPB] + a.sloc[k] : a.head->span_bytes;
}
NXG_DEV uint64_t row_prefix(const NxgRwArgs& a, const Range& g, uint64_t row) {
    if (row <= a.row_begin) return 0;
    if (row >= g.row_end) return a.head->row_bytes;
    const uint64_t j = row - a.row_begin;
    return a.zblk[j / TPB] + a.rloc[j];
}

// bytes go out one at a time behind a capacity check (an overflow is reported from reply_len)
struct Out {
    uint8_t* p;
    uint64_t pos, cap;
    NXG_DEV void put(uint8_t b) {
        if (pos < cap) p[pos] = b;
        pos++;
    }
    NXG_DEV void varint(uint64_t v) {
        while (v >= 0x80) {
            put((uint8_t)(v | 0x80));
            v >>= 7;
        }
        put((uint8_t)v);
    }
};

// a row as the size and rows passes see it
struct RowIn {
    uint64_t id;
    uint32_t fl, oc;
    bool live;
    NXG_DEV bool no_wid() const { return live && (fl & NXG_WRITE_NO_WID); }
    NXG_DEV bool waits() const { return live && oc == NXG_WRITE_ROUTED && (fl & NXG_WRITE_REPLY); }
    NXG_DEV bool replies() const { return live && oc != NXG_WRITE_ROUTED && (fl & NXG_WRITE_REPLY); }
    // (rows without a WriteId, rows on the wait list), one scan for both: a call has < 2^32 rows
    NXG_DEV uint64_t packed() const { return (no_wid() ? 1ull : 0ull) | (waits() ? 1ull << 32 : 0ull); }
};
NXG_DEV RowIn row_in(const NxgRwArgs& a, const Range& g, uint64_t i) {
    RowIn r{0, 0, 0, i < g.row_end};
    if (r.live) {
        r.id = a.id[i];
        r.fl = a.wflags[i];
        r.oc = a.outcome[i];
    }
    return r;
}
// the WriteId the reference's message carries: the wire's, or the next of the caller's block
NXG_DEV uint64_t wid_of(const NxgRwArgs& a, const RowIn& r, uint64_t i, uint64_t fresh_rank) {
    return (r.fl & NXG_WRITE_NO_WID) ? a.fresh_wid + fresh_rank : a.wid[i];
}
// bytes of the WriteResult of a row that replies (outcome 1-3): L, 06, id, 12, |m|, m, wid
NXG_DEV uint32_t result_size(const RowIn& r, uint64_t wid) {
    return 1u + 1u + vl64(r.id) + 2u + kMsgLen[r.oc - 1] + vl64(wid);
}

}  // namespace

__global__ __launch_bounds__(TPB) void nxg_rw_find_kernel(NxgRwArgs a) {
    const uint64_t k = a.ctl_begin + (uint64_t)blockIdx.x * TPB + threadIdx.x;
    const bool sub = k < a.n_ctl && a.ctl_variant[k] == 0;
    const uint64_t m = __ballot(sub);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m))
        atomicMax((unsigned long long*)&a.head->first_sub_inv, (unsigned long long)~k);
}

__global__ __launch_bounds__(TPB) void nxg_rw_spans_kernel(NxgRwArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    uint64_t size = 0;
    if (k < g.s) {
        // varint(L) 01 varint(id), validated by the decode: L may be non-canonical, and bytes
        // after the id inside the wrap are skipped
        uint64_t p = a.ctl_off[k];
        const uint64_t end = p + a.ctl_len[k];
        while (p < end && (a.frame[p] & 0x80)) p++;
        p += 2;  // the length's last byte and the variant
        uint64_t id = 0;
        for (uint32_t sh = 0; sh < 70 && p < end; sh += 7) {
            const uint8_t c = a.frame[p++];
            if (sh < 64) id |= (uint64_t)(c & 0x7f) << sh;
            if (c < 0x80) break;
        }
        a.uid[j] = id;
        if (j < a.cap_unsub) a.unsub_id[j] = id;
        if (id < a.tab.n_ids)
            atomicMax((unsigned long long*)&a.first_unsub[id],
                      ((unsigned long long)a.epoch << 40) | (kRowMask - (a.ctl_row[k] & kRowMask)));
        size = 2 + vl64(id);
    }
    uint64_t total;
    const uint64_t p = block_excl_scan<uint64_t, TPB>(size, tmp, &total);
    if (k < g.s) a.sloc[j] = (uint32_t)p;
    if (threadIdx.x == 0) a.sblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(TPB) void nxg_rw_classify_kernel(NxgRwArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, i = a.row_begin + j;
    RowIn r{0, 0, 0, i < g.row_end};
    if (r.live) {
        r.id = a.id[i];
        r.fl = a.wflags[i];
        const uint32_t perm = r.id < a.tab.n_ids ? a.tab.perm_of_id[r.id] : NXG_NOT_SUBSCRIBED;
        bool unsub = perm == NXG_NOT_SUBSCRIBED;
        if (!unsub) {
            const uint64_t w = a.first_unsub[r.id];
            unsub = (w >> 40) == a.epoch && kRowMask - (w & kRowMask) <= i;
        }
        if (unsub) {
            r.oc = NXG_WRITE_UNSUBSCRIBED;
        } else if (!(perm & kWrite)) {
            r.oc = NXG_WRITE_DENIED;
        } else {
            const uint32_t s = a.tab.slot_of_id[r.id];
            const bool open = s != NXG_NO_SLOT && s < a.tab.n_slots &&
                              a.tab.slot_chan_off[s + 1] > a.tab.slot_chan_off[s];
            r.oc = open ? NXG_WRITE_ROUTED : NXG_WRITE_NOT_ACCEPTED;
        }
        a.outcome[i] = (uint8_t)r.oc;
    }
    if (i < a.n_rows) a.mode[j] = r.live && r.oc == NXG_WRITE_ROUTED ? 0 : 1;
    // six block totals from one scan, 10 bits each (a block has 256 rows): rows without a WriteId,
    // rows on the wait list, rows per outcome. No counter is shared between workgroups.
    const uint64_t six = (r.no_wid() ? 1ull : 0ull) | (r.waits() ? 1ull << 10 : 0ull) |
                         (r.live ? 1ull << (20 + 10 * r.oc) : 0ull);
    uint64_t total;
    (void)block_excl_scan<uint64_t, TPB>(six, tmp, &total);
    if (threadIdx.x == 0) {
        const auto f = [&](int k) { return (total >> (10 * k)) & 0x3ffull; };
        a.cblk[blockIdx.x] = f(0) | f(1) << 32;
        a.oblk[blockIdx.x] = f(2) | f(3) << 32;
        a.oblk[gridDim.x + blockIdx.x] = f(4) | f(5) << 32;
    }
}

// one workgroup: each job's v[0 .. n) scanned in place (exclusive), its total's low 32 bits to
// *lo and the rest to *hi (hi null: the whole total to *lo)
struct NxgRwTop {
    uint64_t* v[4];
    uint64_t n[4];
    uint64_t* lo[4];
    uint64_t* hi[4];
};
__global__ __launch_bounds__(1024) void nxg_rw_top_kernel(NxgRwTop t) {
    __shared__ uint64_t tmp[16];
    __shared__ uint64_t carry;
#pragma unroll 1
    for (int job = 0; job < 4; job++) {
        uint64_t* v = t.v[job];
        const uint64_t n = t.n[job];
        if (!v) continue;
        __syncthreads();
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
#pragma unroll 1
        for (uint64_t b0 = 0; b0 < n; b0 += 1024) {
            const uint64_t i = b0 + threadIdx.x;
            const uint64_t e = i < n ? v[i] : 0;
            uint64_t total;
            const uint64_t p = block_excl_scan<uint64_t, 1024>(e, tmp, &total);
            const uint64_t c = carry;
            if (i < n) v[i] = c + p;
            __syncthreads();
            if (threadIdx.x == 0) carry = c + total;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const uint64_t c = carry;
            if (t.hi[job]) {
                *t.lo[job] = c & 0xffffffffull;
                *t.hi[job] = c >> 32;
            } else {
                *t.lo[job] = c;
            }
        }
    }
}

__global__ __launch_bounds__(TPB) void nxg_rw_size_kernel(NxgRwArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, i = a.row_begin + j;
    const RowIn r = row_in(a, g, i);
    uint64_t total;
    const uint64_t pk = a.cblk[blockIdx.x] + block_excl_scan<uint64_t, TPB>(r.packed(), tmp, &total);
    const uint64_t size = r.replies() ? result_size(r, wid_of(a, r, i, pk & 0xffffffffull)) : 0;
    // (a block's replies are at most 256 * 58 bytes: bytes low, the reply count high)
    const uint64_t p = block_excl_scan<uint64_t, TPB>(size | (size ? 1ull << 32 : 0ull), tmp, &total);
    if (r.live) a.rloc[j] = (uint32_t)p;
    if (threadIdx.x == 0) {
        a.zblk[blockIdx.x] = total & 0xffffffffull;
        a.nblk[blockIdx.x] = total >> 32;
    }
}

__global__ __launch_bounds__(TPB) void nxg_rw_rows_kernel(NxgRwArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, i = a.row_begin + j;
    if ((uint64_t)blockIdx.x * TPB + a.row_begin >= g.row_end) return;  // (block-uniform)
    const RowIn r = row_in(a, g, i);
    uint64_t total;
    const uint64_t pk = a.cblk[blockIdx.x] + block_excl_scan<uint64_t, TPB>(r.packed(), tmp, &total);
    if (!r.live || !(r.fl & NXG_WRITE_REPLY)) return;
    const uint64_t wid = wid_of(a, r, i, pk & 0xffffffffull);
    if (r.oc == NXG_WRITE_ROUTED) {  // wait_write_res.push((id, wid, wait)), server.rs:222
        const uint64_t w = pk >> 32;
        if (w < a.cap_wait) {
            a.wait_row[w] = i;
            a.wait_id[w] = r.id;
            a.wait_wid[w] = wid;
        }
        return;
    }
    const uint64_t n_unsub = g.s - a.ctl_begin;
    Out o{a.reply, a.zblk[blockIdx.x] + a.rloc[j] + span_prefix(a, n_unsub, spans_upto(a, n_unsub, i)),
          a.cap_reply};
    const uint32_t ml = kMsgLen[r.oc - 1];
    o.put((uint8_t)(1u + vl64(r.id) + 2u + ml + vl64(wid) + 1u));  // L = |body| + 1, one byte
    o.put(0x06);
    o.varint(r.id);
    o.put(0x12);
    o.put((uint8_t)ml);
    const char* m = kMsg[r.oc - 1];
    for (uint32_t b = 0; b < ml; b++) o.put((uint8_t)m[b]);
    o.varint(wid);
}

__global__ __launch_bounds__(TPB) void nxg_rw_unsubs_kernel(NxgRwArgs a) {
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    if (k >= g.s) return;
    const uint64_t id = a.uid[j];
    Out o{a.reply, span_prefix(a, g.s - a.ctl_begin, j) + row_prefix(a, g, a.ctl_row[k]), a.cap_reply};
    o.put((uint8_t)(2u + vl64(id)));
    o.put(0x02);
    o.varint(id);
}

// after the fan-out: its entries' rows counted from the batch's first row, and the call's totals
__global__ __launch_bounds__(TPB) void nxg_rw_finish_kernel(NxgRwArgs a, const uint64_t* chan_off,
                                                            uint64_t* ent_row, uint64_t cap_entries) {
    const Range g = range_of(a);
    const uint64_t n = chan_off[a.tab.n_chans];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.head->n_entries = n;
        a.head->next_row = g.row_end;
        a.head->next_ctl = g.s < a.n_ctl ? g.s + 1 : a.n_ctl;
    }
    if (!a.row_begin) return;
    const uint64_t m = n < cap_entries ? n : cap_entries;
    for (uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x; e < m; e += (uint64_t)gridDim.x * TPB)
        ent_row[e] += a.row_begin;
}

uint64_t nxg_rw_scratch_bytes(uint64_t rows, uint64_t spans) {
    const uint64_t nrb = (rows + TPB - 1) / TPB, nsb = (spans + TPB - 1) / TPB;
    // head | cblk, oblk (two halves), zblk, nblk | sblk | uid | rloc | sloc | mode
    return 128 + 5 * nrb * 8 + nsb * 8 + spans * 8 + rows * 4 + spans * 4 + rows + 64;
}

hipError_t nxg_launch_route_writes(NxgRwArgs a, uint8_t* scratch, uint8_t* disp_scratch,
                                   uint64_t* chan_off, uint64_t* ent_sub, uint64_t* ent_row,
                                   uint64_t cap_entries, uint64_t* last_row, int ncu,
                                   hipStream_t s) {
    const uint64_t rows = a.n_rows - a.row_begin, spans = a.n_ctl - a.ctl_begin;
    const uint64_t nrb = (rows + TPB - 1) / TPB, nsb = (spans + TPB - 1) / TPB;
    uint8_t* p = scratch;
    a.head = reinterpret_cast<NxgRwHead*>(p), p += 128;
    a.cblk = reinterpret_cast<uint64_t*>(p), p += nrb * 8;
    a.oblk = reinterpret_cast<uint64_t*>(p), p += 2 * nrb * 8;
    a.zblk = reinterpret_cast<uint64_t*>(p), p += nrb * 8;
    a.nblk = reinterpret_cast<uint64_t*>(p), p += nrb * 8;
    a.sblk = reinterpret_cast<uint64_t*>(p), p += nsb * 8;
    a.uid = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.rloc = reinterpret_cast<uint32_t*>(p), p += rows * 4;
    a.sloc = reinterpret_cast<uint32_t*>(p), p += spans * 4;
    a.mode = p;
    hipError_t e;
    if ((e = hipMemsetAsync(a.head, 0, 128, s)) != hipSuccess) return e;
    if (nsb) {
        hipLaunchKernelGGL(nxg_rw_find_kernel, dim3((uint32_t)nsb), dim3(TPB), 0, s, a);
        hipLaunchKernelGGL(nxg_rw_spans_kernel, dim3((uint32_t)nsb), dim3(TPB), 0, s, a);
    }
    if (nrb) hipLaunchKernelGGL(nxg_rw_classify_kernel, dim3((uint32_t)nrb), dim3(TPB), 0, s, a);
    NxgRwHead* h = a.head;
    if (nrb || nsb) {
        NxgRwTop t{};
        if (nrb) {
            t.v[0] = a.cblk, t.n[0] = nrb, t.lo[0] = &h->n_fresh, t.hi[0] = &h->n_wait;
            t.v[1] = a.oblk, t.n[1] = nrb, t.lo[1] = &h->n_outcome[0], t.hi[1] = &h->n_outcome[1];
            t.v[2] = a.oblk + nrb, t.n[2] = nrb, t.lo[2] = &h->n_outcome[2], t.hi[2] = &h->n_outcome[3];
        }
        if (nsb) t.v[3] = a.sblk, t.n[3] = nsb, t.lo[3] = &h->span_bytes;
        hipLaunchKernelGGL(nxg_rw_top_kernel, dim3(1), dim3(1024), 0, s, t);
    }
    if (nrb) {
        hipLaunchKernelGGL(nxg_rw_size_kernel, dim3((uint32_t)nrb), dim3(TPB), 0, s, a);
        NxgRwTop t{};
        t.v[0] = a.zblk, t.n[0] = nrb, t.lo[0] = &h->row_bytes;
        t.v[1] = a.nblk, t.n[1] = nrb, t.lo[1] = &h->n_row_replies;
        hipLaunchKernelGGL(nxg_rw_top_kernel, dim3(1), dim3(1024), 0, s, t);
        hipLaunchKernelGGL(nxg_rw_rows_kernel, dim3((uint32_t)nrb), dim3(TPB), 0, s, a);
    }
    if (nsb) hipLaunchKernelGGL(nxg_rw_unsubs_kernel, dim3((uint32_t)nsb), dim3(TPB), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the fan-out: channels of on_write[id] in list order (server.rs:225-240), entries tagged with
    // the row's Id (no SubId table), rows the classify pass did not route not pushed
    const NxgSubTable st{a.tab.n_ids, a.tab.slot_of_id, a.tab.n_slots, nullptr, a.tab.slot_chan_off,
                         a.tab.chan,  nullptr,          a.tab.n_chans};
    uint64_t* um = reinterpret_cast<uint64_t*>(disp_scratch);
    if ((e = nxg_launch_dispatch(st, a.id + a.row_begin, rows, disp_scratch + 64, chan_off, ent_sub,
                                 ent_row, cap_entries, last_row, um, ncu, s, a.mode)) != hipSuccess)
        return e;
    const uint64_t want = a.row_begin ? (std::min(rows * 4, cap_entries) + TPB - 1) / TPB : 1;
    const uint32_t fg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ncu * 8));
    hipLaunchKernelGGL(nxg_rw_finish_kernel, dim3(fg), dim3(TPB), 0, s, a, chan_off, ent_row,
                       cap_entries);
    return hipGetLastError();
}
