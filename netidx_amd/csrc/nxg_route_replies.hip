// nxg_route_replies.hip -- a subscriber's mixed batch routed on gfx950. Replaces
// ConnectionCtx::process_batch (netidx/src/subscriber/connection.rs:409-541) and unsubscribe()
// (connection.rs:67-83) for the rows and control spans nxg_decode_updates produced from a frame
// that holds a message other than an Update.
//
// Per message, in message order (span k precedes row ctl_row[k]; equal ctl_row in k order):
//   Update(id, v), row i   subscribed: one entry per stream of the slot, last_row (connection.rs:
//                          419-431); otherwise To::Unsubscribe(id) (:432)
//   Heartbeat, WriteResult reported only (:434-445)
//   NoSuchValue / Denied   pending.remove(path) (:447, :452): FAILED for the first span of the call
//                          that names a pending path
//   Unsubscribed(id)       subscriptions.remove(id) and unsubscribe() (:456-461, :74-80): one
//                          (SubId, NXG_ENT_SPAN | k) entry per stream of the slot
//   Subscribed(path, id)   pending.remove(path) (:463): ORPHAN on a miss (:464-467), else DROPPED
//                          (finished.send failed, :502-505) or SUBSCRIBED (:506-517); an alias
//                          (:468-490) is the host's
// Within one call an Id changes state at most once: the call stops in front of a Subscribed or
// Unsubscribed span whose Id an earlier such span of the call named (stop 1). So what a row's Id
// is subscribed to is one comparison: of the row with ctl_row of the Id's first naming span, whose
// outcome says what changed. That span is found through first_id[], a ctx-owned table of
// epoch << 40 | ~j words (atomicMax; a word of another call's epoch reads as "none", so the table
// is never cleared, as first_unsub of nxg_route_writes.hip). first_q[] does the same per pending
// request: the first span of the call that names its path takes it out of `pending`.
// A path that is not plain, an alias and a hit with an Id outside the table are the host's (stop
// 2). Every stop candidate depends only on the spans before it, so the lowest one (atomicMax of
// ~k) is exact.
//
// Everything whose place depends on what precedes it comes from block sums scanned by a one-
// workgroup kernel between launches; no kernel waits on another workgroup, and no shared counter
// decides an order. Launches, in order:
//   parse    per span: its Id and / or its path's request q (hash, byte-confirmed probe of
//            `pending`), first_id[] / first_q[]; a path that is not plain lowers the stop
//   stops    per span: named twice (1), alias or Id outside the table (2): lowers the stop
//   spans    per span in front of the stop: outcome[], span_q[], span_id[], its reply's size, its
//            item; block sums of reply bytes, replies, SUBSCRIBED and UNSUBSCRIBED spans, and of
//            the spans per outcome
//   rows     per row in front of ctl_row[stop]: the slot its Id has at that point, its item,
//            last_row (atomicMax of row + 1), its reply's size; block sums of bytes and replies
//   top      exclusive scans of those block sums, their totals into the head
//   emit     the spans' replies and the sub / unsub lists; the rows' replies. A row's reply sits
//            after the replies of the rows before it and of the spans with ctl_row <= i (ctl_row is
//            sorted: a search), a span's after the spans before it and the rows before ctl_row[k]
//   (the fan-out is nxg_launch_dispatch over the items: the call's messages in message order,
//   item j + m for the row with j rows and m spans before it, each with its own slot)
//   finish   the entries' item indices replaced by the row or NXG_ENT_SPAN | k, the head's totals
// Wire form: To::Unsubscribe(id) is varint(L) 01 varint(id), L = 2 + vl(id), one byte.
#include <algorithm>

#include "nxg_device.h"
#include "nxg_internal.h"
#include "nxg_path_probe.h"

namespace {

using namespace nxgprobe;

constexpr int TPB = kRwBlock;
constexpr uint64_t kIdxMask = (1ull << 40) - 1;  // first_id / first_q word: epoch << 40 | ~j
constexpr uint8_t kNotPlain = 3;                 // skind[]: stop 2, found by the parse pass

NXG_DEV unsigned long long first_word(const NxgRrArgs& a, uint64_t j) {
    return ((unsigned long long)a.epoch << 40) | (kIdxMask - j);
}
// the span (counted from ctl_begin) a first_id / first_q word names, or ~0
NXG_DEV uint64_t first_of(const NxgRrArgs& a, uint64_t w) {
    return (w >> 40) == a.epoch ? kIdxMask - (w & kIdxMask) : ~0ull;
}

struct Range {
    uint64_t s;        // the span the call stops in front of, or n_ctl
    uint64_t row_end;  // rows [row_begin, row_end) are processed
};
NXG_DEV uint64_t row_of_span(const NxgRrArgs& a, uint64_t k) {  // ctl_row[k] within the call's rows
    const uint64_t r = a.ctl_row[k];
    return r < a.row_begin ? a.row_begin : r > a.n_rows ? a.n_rows : r;
}
NXG_DEV Range range_of(const NxgRrArgs& a) {
    const uint64_t v = a.head->stop_inv;
    Range r;
    r.s = v ? ~v : a.n_ctl;
    r.row_end = r.s < a.n_ctl ? row_of_span(a, r.s) : a.n_rows;
    return r;
}
// spans with ctl_row <= row among spans [ctl_begin, ctl_begin + n)
NXG_DEV uint64_t spans_upto(const NxgRrArgs& a, uint64_t n, uint64_t row) {
    const uint64_t* cr = a.ctl_row + a.ctl_begin;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cr[mid] <= row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
NXG_DEV uint32_t slot_of(const NxgRrArgs& a, uint64_t id) {
    return id < a.subs.n_ids ? a.subs.slot_of_id[id] : NXG_NO_SLOT;
}

// a varint at p (validated by the decode), p moved past it
NXG_DEV uint64_t varint_at(const uint8_t* f, uint64_t& p, uint64_t end) {
    uint64_t v = 0;
    for (uint32_t sh = 0; sh < 70 && p < end; sh += 7) {
        const uint8_t c = f[p++];
        if (sh < 64) v |= (uint64_t)(c & 0x7f) << sh;
        if (c < 0x80) break;
    }
    return v;
}

// To::Unsubscribe(id) at reply[pos ...), behind a capacity check (an overflow is reported from
// reply_len)
NXG_DEV void put_unsubscribe(const NxgRrArgs& a, uint64_t pos, uint64_t id) {
    const auto put = [&](uint8_t b) {
        if (pos < a.cap_reply) a.reply[pos] = b;
        pos++;
    };
    put((uint8_t)(2u + vl64(id)));
    put(0x01);
    while (id >= 0x80) {
        put((uint8_t)(id | 0x80));
        id >>= 7;
    }
    put((uint8_t)id);
}

// a span's place in the scans: reply bytes | replies << 16 | SUBSCRIBED << 32 | UNSUBSCRIBED << 48
// before it within its block (a block's replies are at most 256 * 12 bytes)
NXG_DEV uint64_t span_prefix(const NxgRrArgs& a, uint64_t n_spans, uint64_t j) {
    return j < n_spans ? a.zblk[j / TPB] + (a.sloc[j] & 0xffffull) : a.head->span_bytes;
}
NXG_DEV uint64_t row_prefix(const NxgRrArgs& a, const Range& g, uint64_t row) {
    if (row <= a.row_begin) return 0;
    if (row >= g.row_end) return a.head->row_bytes;
    const uint64_t j = row - a.row_begin;
    return a.rzblk[j / TPB] + (a.rloc[j] & 0x7fffffffu);
}

}  // namespace

__global__ __launch_bounds__(TPB) void nxg_rr_parse_kernel(NxgRrArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    if (k >= a.n_ctl) return;
    const uint32_t var = a.ctl_variant[k];
    uint64_t id = NXG_NO_ID, q = NXG_NO_ID;
    uint8_t kind = 0;
    if (var <= 3) {
        // varint(L) variant [varint(|p|) p] [varint(id)], validated by the decode: L may be
        // non-canonical, and bytes after the last field inside the wrap are skipped
        uint64_t p = a.ctl_off[k];
        const uint64_t end = p + a.ctl_len[k];
        while (p < end && (a.frame[p] & 0x80)) p++;
        p += 2;  // the length's last byte and the variant
        if (var != 2) {
            const uint64_t plen = varint_at(a.frame, p, end);
            bool plain = false;
            uint64_t hv = 0;
            const GSrc src{a.frame};
            if (p <= end && plen <= end - p) hv = path_hash(src, p, (uint32_t)plen, &plain);
            if (!plain) {
                kind = kNotPlain;
                atomicMax((unsigned long long*)&a.head->stop_inv, (unsigned long long)~k);
            } else {
                const uint64_t s = pt_find(a.pending, src, p, (uint32_t)plen, hv);
                if (s != ~0ull) {
                    q = a.pending.id[s];
                    // the lowest such span and its cause travel in one word (k < 2^56)
                    const uint32_t bad = q >= a.n_pending                  ? 1u
                                         : a.pend_slot[q] >= a.subs.n_slots ? 2u
                                                                            : 0u;
                    if (bad) {
                        atomicMax((unsigned long long*)&a.head->bad_inv,
                                  (unsigned long long)(~k << 8 | bad));
                        q = NXG_NO_ID;
                    } else {
                        atomicMax((unsigned long long*)&a.first_q[q], first_word(a, j));
                    }
                }
                p += plen;
            }
        }
        if (var >= 2 && kind != kNotPlain) {
            id = varint_at(a.frame, p, end);
            if (id < a.subs.n_ids) atomicMax((unsigned long long*)&a.first_id[id], first_word(a, j));
        }
    }
    a.sid[j] = id;
    a.sq[j] = q;
    a.skind[j] = kind;
}

__global__ __launch_bounds__(TPB) void nxg_rr_stops_kernel(NxgRrArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    if (k >= a.n_ctl || a.skind[j] == kNotPlain) return;
    const uint32_t var = a.ctl_variant[k];
    if (var != 2 && var != 3) return;
    const uint64_t id = a.sid[j], q = a.sq[j];
    uint8_t kind = 0;
    if (id < a.subs.n_ids && first_of(a, a.first_id[id]) != j) {
        kind = 1;  // an earlier Subscribed / Unsubscribed span of the call named the Id
    } else if (var == 3 && q != NXG_NO_ID && first_of(a, a.first_q[q]) == j &&
               (id >= a.subs.n_ids || slot_of(a, id) != NXG_NO_SLOT)) {
        kind = 2;  // a subscription the table has no room for, or an alias (connection.rs:468-490)
    }
    if (kind) {
        a.skind[j] = kind;
        atomicMax((unsigned long long*)&a.head->stop_inv, (unsigned long long)~k);
    }
}

__global__ __launch_bounds__(TPB) void nxg_rr_spans_kernel(NxgRrArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    const bool live = k < g.s;
    uint32_t oc = NXG_REPLY_NONE, slot = NXG_NO_SLOT;
    uint64_t size = 0;
    if (live) {
        const uint32_t var = a.ctl_variant[k];
        const uint64_t id = a.sid[j];
        uint64_t q = a.sq[j];
        if (q != NXG_NO_ID && first_of(a, a.first_q[q]) != j) q = NXG_NO_ID;  // named before
        if (var == 6) {
            oc = NXG_REPLY_WRITE_RESULT;
        } else if (var <= 1) {
            if (q != NXG_NO_ID) oc = NXG_REPLY_FAILED;
        } else if (var == 2) {
            slot = slot_of(a, id);
            if (slot != NXG_NO_SLOT) oc = NXG_REPLY_UNSUBSCRIBED;
        } else if (var == 3) {
            oc = q == NXG_NO_ID                          ? NXG_REPLY_ORPHAN
                 : a.pend_alive && !a.pend_alive[q] ? NXG_REPLY_DROPPED
                                                    : NXG_REPLY_SUBSCRIBED;
            if (oc != NXG_REPLY_SUBSCRIBED) size = 2 + vl64(id);
        }
        a.outcome[k] = (uint8_t)oc;
        a.span_id[k] = id;
        a.span_q[k] = oc == NXG_REPLY_FAILED || oc == NXG_REPLY_DROPPED || oc == NXG_REPLY_SUBSCRIBED
                          ? q
                          : NXG_NO_ID;
    }
    if (k < a.n_ctl) {  // the span's item: after the spans before it and the rows before ctl_row[k]
        const uint64_t it = j + (row_of_span(a, k) - a.row_begin);
        a.item_slot[it] = slot;
        a.item_val[it] = NXG_ENT_SPAN | k;
    }
    const uint64_t four = size | (size ? 1ull << 16 : 0ull) |
                          (oc == NXG_REPLY_SUBSCRIBED ? 1ull << 32 : 0ull) |
                          (oc == NXG_REPLY_UNSUBSCRIBED ? 1ull << 48 : 0ull);
    uint64_t total;
    const uint64_t p = block_excl_scan<uint64_t, TPB>(four, tmp, &total);
    if (live) a.sloc[j] = p;
    // the spans per outcome: seven block totals from one scan, 9 bits each (a block has 256 spans)
    uint64_t seven;
    (void)block_excl_scan<uint64_t, TPB>(live ? 1ull << (9 * oc) : 0ull, tmp, &seven);
    if (threadIdx.x == 0) {
        const uint64_t nb = gridDim.x;
        const auto f = [&](int o) { return (seven >> (9 * o)) & 0x1ffull; };
        a.zblk[blockIdx.x] = total & 0xffffull;
        a.nblk[blockIdx.x] = (total >> 16) & 0xffffull;
        a.sblk[blockIdx.x] = (total >> 32) & 0xffffull;
        a.ublk[blockIdx.x] = total >> 48;
        a.oblk[blockIdx.x] = f(0) | f(1) << 32;
        a.oblk[nb + blockIdx.x] = f(2) | f(3) << 32;
        a.oblk[2 * nb + blockIdx.x] = f(4) | f(5) << 32;
        a.oblk[3 * nb + blockIdx.x] = f(6);
    }
}

__global__ __launch_bounds__(TPB) void nxg_rr_rows_kernel(NxgRrArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const Range g = range_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, i = a.row_begin + j;
    const bool live = i < g.row_end;
    uint32_t slot = NXG_NO_SLOT;
    uint64_t size = 0;
    if (live) {
        const uint64_t id = a.id[i];
        slot = slot_of(a, id);
        if (id < a.subs.n_ids) {
            // the Id's one change of state in this call, if it lies in front of this row
            const uint64_t f = first_of(a, a.first_id[id]);
            if (f != ~0ull && a.ctl_begin + f < g.s && a.ctl_row[a.ctl_begin + f] <= i) {
                const uint32_t oc = a.outcome[a.ctl_begin + f];
                if (oc == NXG_REPLY_UNSUBSCRIBED) slot = NXG_NO_SLOT;
                else if (oc == NXG_REPLY_SUBSCRIBED) slot = a.pend_slot[a.span_q[a.ctl_begin + f]];
            }
        }
        if (slot == NXG_NO_SLOT) size = 2 + vl64(id);
        else if (a.subs.slot_has_last[slot])
            atomicMax((unsigned long long*)&a.last_row[slot], (unsigned long long)(i + 1));
    }
    if (i < a.n_rows) {  // the row's item: after the rows before it and the spans with ctl_row <= i
        const uint64_t it = j + spans_upto(a, a.n_ctl - a.ctl_begin, i);
        a.item_slot[it] = slot;
        a.item_val[it] = i;
    }
    uint64_t total;
    const uint64_t p = block_excl_scan<uint64_t, TPB>(size | (size ? 1ull << 32 : 0ull), tmp, &total);
    if (live) a.rloc[j] = (uint32_t)(p & 0x7fffffffu) | (size ? 1u << 31 : 0u);
    if (threadIdx.x == 0) {
        a.rzblk[blockIdx.x] = total & 0xffffffffull;
        a.rnblk[blockIdx.x] = total >> 32;
    }
}

// one workgroup: each job's v[0 .. n) scanned in place (exclusive), its total's low 32 bits to
// *lo and the rest to *hi (hi null: the whole total to *lo)
struct NxgRrTop {
    uint64_t* v[10];
    uint64_t n[10];
    uint64_t* lo[10];
    uint64_t* hi[10];
};
__global__ __launch_bounds__(1024) void nxg_rr_top_kernel(NxgRrTop t) {
    __shared__ uint64_t tmp[16];
    __shared__ uint64_t carry;
#pragma unroll 1
    for (int job = 0; job < 10; job++) {
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

// the replies and lists of the spans (blocks [0, nsb)) and the replies of the rows (the others)
__global__ __launch_bounds__(TPB) void nxg_rr_emit_kernel(NxgRrArgs a, uint32_t nsb) {
    const Range g = range_of(a);
    const uint64_t n_spans = g.s - a.ctl_begin;
    if (blockIdx.x < nsb) {
        const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
        if (k >= g.s) return;
        const uint32_t oc = a.outcome[k];
        const uint64_t loc = a.sloc[j], id = a.sid[j];
        if (oc == NXG_REPLY_ORPHAN || oc == NXG_REPLY_DROPPED) {
            put_unsubscribe(a, span_prefix(a, n_spans, j) + row_prefix(a, g, row_of_span(a, k)), id);
        } else if (oc == NXG_REPLY_SUBSCRIBED) {
            const uint64_t r = a.sblk[blockIdx.x] + ((loc >> 32) & 0xffffull);
            if (r < a.cap_sub) {
                a.sub_span[r] = k;
                a.sub_q[r] = a.sq[j];
                a.sub_id[r] = id;
            }
        } else if (oc == NXG_REPLY_UNSUBSCRIBED) {
            const uint64_t r = a.ublk[blockIdx.x] + (loc >> 48);
            if (r < a.cap_unsub) {
                a.unsub_id[r] = id;
                a.unsub_slot[r] = slot_of(a, id);
            }
        }
        return;
    }
    const uint32_t b = blockIdx.x - nsb;
    const uint64_t j = (uint64_t)b * TPB + threadIdx.x, i = a.row_begin + j;
    if (i >= g.row_end) return;
    const uint32_t loc = a.rloc[j];
    if (!(loc >> 31)) return;
    put_unsubscribe(a, a.rzblk[b] + (loc & 0x7fffffffu) + span_prefix(a, n_spans, spans_upto(a, n_spans, i)),
                    a.id[i]);
}

// after the fan-out: an entry's item replaced by what the item stands for, and the call's totals
__global__ __launch_bounds__(TPB) void nxg_rr_finish_kernel(NxgRrArgs a, const uint64_t* chan_off,
                                                            uint64_t* ent_row, uint64_t cap_entries) {
    const Range g = range_of(a);
    const uint64_t n = chan_off[a.subs.n_chans];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        NxgRrHead* h = a.head;
        h->n_entries = n;
        h->next_row = g.row_end;
        h->next_ctl = g.s;
        h->stopped = g.s < a.n_ctl ? (a.skind[g.s - a.ctl_begin] == 1 ? 1u : 2u) : 0u;
    }
    const uint64_t m = n < cap_entries ? n : cap_entries;
    for (uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x; e < m; e += (uint64_t)gridDim.x * TPB)
        ent_row[e] = a.item_val[ent_row[e]];
}

namespace {
uint64_t up8(uint64_t x) { return (x + 7) & ~7ull; }
}  // namespace

uint64_t nxg_rr_scratch_bytes(uint64_t rows, uint64_t spans) {
    const uint64_t nrb = (rows + TPB - 1) / TPB, nsb = (spans + TPB - 1) / TPB;
    // head | sid, sq, sloc | zblk, nblk, sblk, ublk, oblk (four) | rzblk, rnblk | item_val |
    // item_slot | rloc | skind
    return sizeof(NxgRrHead) + spans * 3 * 8 + nsb * 8 * 8 + nrb * 2 * 8 + (rows + spans) * 8 +
           up8((rows + spans) * 4) + up8(rows * 4) + up8(spans) + 64;
}

hipError_t nxg_launch_route_replies(NxgRrArgs a, uint8_t* scratch, uint8_t* disp_scratch,
                                    uint64_t* chan_off, uint64_t* ent_sub, uint64_t* ent_row,
                                    uint64_t cap_entries, int ncu, hipStream_t s) {
    const uint64_t rows = a.n_rows - a.row_begin, spans = a.n_ctl - a.ctl_begin;
    const uint64_t nrb = (rows + TPB - 1) / TPB, nsb = (spans + TPB - 1) / TPB;
    uint8_t* p = scratch;
    a.head = reinterpret_cast<NxgRrHead*>(p), p += sizeof(NxgRrHead);
    a.sid = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.sq = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.sloc = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.zblk = reinterpret_cast<uint64_t*>(p), p += nsb * 8;
    a.nblk = reinterpret_cast<uint64_t*>(p), p += nsb * 8;
    a.sblk = reinterpret_cast<uint64_t*>(p), p += nsb * 8;
    a.ublk = reinterpret_cast<uint64_t*>(p), p += nsb * 8;
    a.oblk = reinterpret_cast<uint64_t*>(p), p += 4 * nsb * 8;
    a.rzblk = reinterpret_cast<uint64_t*>(p), p += nrb * 8;
    a.rnblk = reinterpret_cast<uint64_t*>(p), p += nrb * 8;
    a.item_val = reinterpret_cast<uint64_t*>(p), p += (rows + spans) * 8;
    a.item_slot = reinterpret_cast<uint32_t*>(p), p += up8((rows + spans) * 4);
    a.rloc = reinterpret_cast<uint32_t*>(p), p += up8(rows * 4);
    a.skind = p;
    hipError_t e;
    if ((e = hipMemsetAsync(a.head, 0, sizeof(NxgRrHead), s)) != hipSuccess) return e;
    if (a.subs.n_slots &&
        (e = hipMemsetAsync(a.last_row, 0, a.subs.n_slots * 8, s)) != hipSuccess)
        return e;
    if (nsb) {
        const dim3 g((uint32_t)nsb), b(TPB);
        hipLaunchKernelGGL(nxg_rr_parse_kernel, g, b, 0, s, a);
        hipLaunchKernelGGL(nxg_rr_stops_kernel, g, b, 0, s, a);
        hipLaunchKernelGGL(nxg_rr_spans_kernel, g, b, 0, s, a);
    }
    if (nrb) hipLaunchKernelGGL(nxg_rr_rows_kernel, dim3((uint32_t)nrb), dim3(TPB), 0, s, a);
    NxgRrHead* h = a.head;
    if (nrb || nsb) {
        NxgRrTop t{};
        if (nsb) {
            t.v[0] = a.zblk, t.n[0] = nsb, t.lo[0] = &h->span_bytes;
            t.v[1] = a.nblk, t.n[1] = nsb, t.lo[1] = &h->n_span_replies;
            t.v[2] = a.sblk, t.n[2] = nsb, t.lo[2] = &h->n_sub;
            t.v[3] = a.ublk, t.n[3] = nsb, t.lo[3] = &h->n_unsub;
            for (int o = 0; o < 4; o++) {
                t.v[4 + o] = a.oblk + o * nsb, t.n[4 + o] = nsb, t.lo[4 + o] = &h->n_outcome[2 * o];
                if (o < 3) t.hi[4 + o] = &h->n_outcome[2 * o + 1];
            }
        }
        if (nrb) {
            t.v[8] = a.rzblk, t.n[8] = nrb, t.lo[8] = &h->row_bytes;
            t.v[9] = a.rnblk, t.n[9] = nrb, t.lo[9] = &h->n_unmatched;
        }
        hipLaunchKernelGGL(nxg_rr_top_kernel, dim3(1), dim3(1024), 0, s, t);
        hipLaunchKernelGGL(nxg_rr_emit_kernel, dim3((uint32_t)(nsb + nrb)), dim3(TPB), 0, s, a,
                           (uint32_t)nsb);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the fan-out over the items: one entry per stream of the item's slot, in message order (the
    // dispatch reads no Id in slot mode; item_val stands in where it wants a readable array)
    uint64_t* um = reinterpret_cast<uint64_t*>(disp_scratch);
    if ((e = nxg_launch_dispatch(a.subs, a.item_val, rows + spans, disp_scratch + 64, chan_off, ent_sub,
                                 ent_row, cap_entries, nullptr, um, ncu, s, nullptr, nullptr,
                                 a.item_slot)) != hipSuccess)
        return e;
    const uint64_t want = (std::min((rows + spans) * 4, cap_entries) + TPB - 1) / TPB;
    const uint32_t fg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ncu * 8));
    hipLaunchKernelGGL(nxg_rr_finish_kernel, dim3(fg), dim3(TPB), 0, s, a, chan_off, ent_row,
                       cap_entries);
    return hipGetLastError();
}
