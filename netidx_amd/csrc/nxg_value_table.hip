// nxg_value_table.hip -- committed values folded into a device-resident table (NxgValueTable).
//
// UpdateBatch::commit ends each arm with `pbl.current = v` (publisher/mod.rs:796, 809) and a
// subscription that keeps `last` stores the event it delivers; the routing calls only report
// which row that is (last_row[slot] = 1 + row). Here the table takes those values: slot s gets the
// value of batch row src_row[s] - 1, with its text / Decimal / Abstract bytes appended to the
// table's heap and its child subtree appended to the table's child columns, `fixed` re-based.
//
// A subtree is written as `Layout` (tests/test_publish_values_cpu.py) writes it: a container's
// elements contiguous, blocks handed out in depth-first preorder (when the container is visited),
// payload bytes in visit order. The walk is restated here (as nxg_route_subscribes.hip restates
// the encoder's) because it carries a destination cursor per level next to the source's.
//
// Passes, none of which waits on another workgroup:
//   size    one lane per slot: validates the new value (and, in place, the old one) and sizes it:
//           heap bytes, child slots, heap-borne leaves. Scalars cost nothing, flat containers are
//           walked in registers, nested ones on the wave's LDS stack, one lane at a time. Per-slot
//           prefixes within the block of VT_SLOTS_PER_BLOCK slots, block sums.
//   top     one workgroup: the three block sums scanned VT_TOP_WIDTH at a time, the totals, and
//           the verdict (head.ok): no refused slot and everything fits. Nothing was written so far.
//   place   the same walk again at the scanned positions: rows, child slots, and one segment
//           (where to, from where) per heap-borne leaf. Slots in order and leaves in walk order:
//           the list is sorted by destination.
//   copy    a dense segmented copy over the new heap range: each lane owns one destination-aligned
//           block of VT_COPY_BLOCK bytes, finds its segment (the wave narrows the list to its
//           1 KiB by wave_lower_bound, the lane bisects that), and moves the block with one
//           unaligned load and one aligned store when it lies inside one segment, byte by byte at
//           segment edges and at both ends of the range.
// An F64 table (no tag column) has its own two small kernels: a check of the selected rows and the
// gather fixed[s] = batch.fixed[src_row[s] - 1].
#include "nxg_device.h"
#include "nxg_internal.h"

namespace {

constexpr int VT_SLOTS_PER_BLOCK = 256;  // = kVtBlock
constexpr int VT_TOP_WIDTH = 1024;       // block sums scanned per step of the top kernel
constexpr int VT_COPY_BLOCK = 16;        // bytes per lane of the copy kernel
constexpr int VT_WAVES = VT_SLOTS_PER_BLOCK / 64;
constexpr int VT_MAX_DEPTH = NXG_MAX_DEPTH;
static_assert(VT_SLOTS_PER_BLOCK == kVtBlock, "block size");

// cursors of a walk: sizes when they start at 0, positions when they start at the scanned bases
struct Pos {
    uint64_t heap, kid, leaf;
};

NXG_DEV void slot_at(const NxgVtSrc& s, bool child, uint64_t i, uint32_t& t, uint64_t& f,
                     uint32_t& a) {
    if (child) {
        t = s.ctag[i];
        f = s.cfixed[i];
        a = s.caux[i];
    } else {
        t = s.tag ? s.tag[i] : 9u;
        f = s.fixed[i];
        a = s.aux ? s.aux[i] : 0u;
    }
}

NXG_DEV bool is_container(uint32_t t) { return t == 19 || t == 21 || t == 22; }

// kind 0: the value is its slot; 1: n payload bytes at heap + f; 2: n child slots from f
NXG_DEV uint32_t classify(const NxgVtSrc& S, uint32_t t, uint64_t f, uint32_t a, uint32_t& kind,
                          uint64_t& n) {
    kind = 0;
    n = 0;
    if (t > 27 && t != NXG_TAG_UNSUBSCRIBED) return kVtTag;
    if (t == 12 || t == 13 || t == 18 || t == 20 || t == 27) {
        kind = 1;
        n = t == 20 ? 16ull : (uint64_t)a;
        return (f > S.heap_len || n > S.heap_len - f) ? kVtHeap : 0u;
    }
    if (is_container(t)) {
        kind = 2;
        n = t == 19 ? (uint64_t)a : t == 21 ? 2ull * a : 1ull;
        if (n == 0) return 0;
        if (!S.ctag) return kVtNoKids;
        return (f > S.n_children || n > S.n_children - f) ? kVtKids : 0u;
    }
    return 0;
}

template <bool PLACE>
NXG_DEV void put(const NxgVtDst& D, bool child, uint64_t d, uint32_t t, uint64_t f, uint32_t a) {
    if constexpr (PLACE) {
        if (child) {
            D.ctag[d] = (uint8_t)t;
            D.cfixed[d] = f;
            D.caux[d] = a;
        } else {
            D.tag[d] = (uint8_t)t;
            D.fixed[d] = f;
            D.aux[d] = a;
        }
    }
}

// one value: checked, its payload taken from the cursors, written (PLACE) at row / child slot d.
// A container leaves its child count in n and its block in base.
template <bool PLACE>
NXG_DEV uint32_t node(const NxgVtArgs& A, const NxgVtSrc& S, uint32_t t, uint64_t f, uint32_t a,
                      bool dchild, uint64_t d, Pos& p, uint64_t& n, uint64_t& base) {
    uint32_t kind;
    const uint32_t c = classify(S, t, f, a, kind, n);
    if (c) return c;
    uint64_t nf = f;
    if (kind == 1) {
        nf = p.heap;
        if (n) {  // an empty payload is no segment
            if constexpr (PLACE) {
                A.seg_dst[p.leaf] = p.heap;
                A.seg_src[p.leaf] = (uint64_t)(uintptr_t)(S.heap + f);
            }
            p.leaf++;
            p.heap += n;
        }
        n = 0;
    } else if (kind == 2) {
        nf = base = p.kid;
        p.kid += n;
    }
    put<PLACE>(A.dst, dchild, d, t, nf, a);
    return 0;
}

// The value at row `row` of S, to slot `dslot`. Without a stack (stk null) a flat container is
// walked in registers and a nested one sets `more` (the caller restarts with its saved cursors
// and the wave's stack). With one: 3 * VT_MAX_DEPTH words, frame k holding the pending children
// at level k + 1 (left, next source slot, next destination slot). Returns the cause of the first
// refusal in walk order, 0 for none.
template <bool PLACE>
NXG_DEV uint32_t walk(const NxgVtArgs& A, const NxgVtSrc& S, uint64_t row, uint64_t dslot, Pos& p,
                      uint64_t* stk, bool& more) {
    uint32_t t, a;
    uint64_t f, n = 0, base = 0;
    more = false;
    slot_at(S, false, row, t, f, a);
    uint32_t c = node<PLACE>(A, S, t, f, a, false, dslot, p, n, base);
    if (c || n == 0) return c;
    if (!stk) {
        const uint64_t s0 = f, d0 = base;
#pragma unroll 1
        for (uint64_t k = 0; k < n; k++) {
            uint64_t m = 0, b2 = 0;
            slot_at(S, true, s0 + k, t, f, a);
            if (is_container(t)) {
                more = true;
                return 0;
            }
            c = node<PLACE>(A, S, t, f, a, true, d0 + k, p, m, b2);
            if (c) return c;
        }
        return 0;
    }
    uint64_t* srem = stk;
    uint64_t* ssrc = stk + VT_MAX_DEPTH;
    uint64_t* sdst = stk + 2 * VT_MAX_DEPTH;
    int sp = 1;
    srem[0] = n, ssrc[0] = f, sdst[0] = base;
#pragma unroll 1
    while (sp > 0) {
        const int k = sp - 1;
        if (srem[k] == 0) {
            sp--;
            continue;
        }
        srem[k]--;
        const uint64_t cs = ssrc[k]++, cd = sdst[k]++;
        slot_at(S, true, cs, t, f, a);
        n = 0;
        c = node<PLACE>(A, S, t, f, a, true, cd, p, n, base);
        if (c) return c;
        if (n) {  // a container at level sp: its children sit at level sp + 1
            if (sp >= VT_MAX_DEPTH) return kVtDepth;
            srem[sp] = n, ssrc[sp] = f, sdst[sp] = base, sp++;
        }
    }
    return 0;
}

// flat first, then (one lane at a time) on the wave's stack
template <bool PLACE>
NXG_DEV uint32_t walk_value(const NxgVtArgs& A, const NxgVtSrc& S, bool want, uint64_t row,
                            uint64_t dslot, Pos& p, uint64_t* stk) {
    uint32_t c = 0;
    bool more = false;
    const Pos p0 = p;
    if (want) c = walk<PLACE>(A, S, row, dslot, p, nullptr, more);
    one_lane_at_a_time(more, [&] {
        bool m2;
        p = p0;
        c = walk<PLACE>(A, S, row, dslot, p, stk, m2);
    });
    return c;
}

// where slot s takes its value from: 0 nowhere (it keeps its value), 1 batch row `row`,
// 2 row `row` of old, 3 Null; kVtRow when src_row names no row of the batch
NXG_DEV uint32_t source_of(const NxgVtArgs& A, uint64_t s, uint32_t& mode, uint64_t& row) {
    mode = 0;
    row = 0;
    const uint64_t r = (A.src_row && s < A.n_sel) ? A.src_row[s] : 0;
    if (r) {
        if (r - 1 >= A.batch.n_rows) return kVtRow;
        mode = 1;
        row = r - 1;
    } else if (A.rebuild) {
        mode = s < A.n_sel ? 2u : 3u;
        row = s;
    }
    return 0;
}

// batch or old, field by field (a reference chosen at run time would be a private copy)
NXG_DEV NxgVtSrc pick(const NxgVtArgs& A, bool b) {
    NxgVtSrc S;
    S.tag = b ? A.batch.tag : A.old.tag;
    S.fixed = b ? A.batch.fixed : A.old.fixed;
    S.aux = b ? A.batch.aux : A.old.aux;
    S.ctag = b ? A.batch.ctag : A.old.ctag;
    S.cfixed = b ? A.batch.cfixed : A.old.cfixed;
    S.caux = b ? A.batch.caux : A.old.caux;
    S.heap = b ? A.batch.heap : A.old.heap;
    S.n_rows = b ? A.batch.n_rows : A.old.n_rows;
    S.n_children = b ? A.batch.n_children : A.old.n_children;
    S.heap_len = b ? A.batch.heap_len : A.old.heap_len;
    return S;
}

NXG_DEV void refuse(NxgVtHead* h, uint64_t slot, uint32_t cause) {
    atomicMax((unsigned long long*)&h->err_inv, (unsigned long long)((~slot << 8) | cause));
}

}  // namespace

__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_size_kernel(NxgVtArgs A) {
    __shared__ uint64_t stks[VT_WAVES][3 * VT_MAX_DEPTH];
    __shared__ uint64_t tmp[VT_WAVES];
    __shared__ uint64_t red[3][VT_WAVES];
    const uint64_t s = (uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x;
    const bool in = s < A.dst.n_slots;
    uint64_t* stk = stks[threadIdx.x >> 6];
    uint32_t mode = 0, cause = 0;
    uint64_t row = 0;
    if (in) cause = source_of(A, s, mode, row);
    const bool sel = in && A.src_row && s < A.n_sel && A.src_row[s] != 0;
    Pos nw{0, 0, 0}, od{0, 0, 0};
    {
        const NxgVtSrc S = pick(A, mode == 1);
        const uint32_t c = walk_value<false>(A, S, mode == 1 || mode == 2, row, s, nw, stk);
        if (c) cause = c | (mode == 2 ? kVtOld : 0u);
    }
    if (!A.rebuild) {  // in place: the replaced value leaves the live counts
        const uint32_t c = walk_value<false>(A, A.old, sel && !cause, s, s, od, stk);
        if (c) cause = c | kVtOld;
    }
    if (cause) {
        refuse(A.head, s, cause);
        nw = Pos{0, 0, 0};
        od = Pos{0, 0, 0};
    }
    uint64_t tot;
    const uint64_t eb = block_excl_scan<uint64_t, VT_SLOTS_PER_BLOCK>(nw.heap, tmp, &tot);
    if (threadIdx.x == 0) A.bbytes[blockIdx.x] = tot;
    const uint64_t ek = block_excl_scan<uint64_t, VT_SLOTS_PER_BLOCK>(nw.kid, tmp, &tot);
    if (threadIdx.x == 0) A.bkids[blockIdx.x] = tot;
    const uint64_t el = block_excl_scan<uint64_t, VT_SLOTS_PER_BLOCK>(nw.leaf, tmp, &tot);
    if (threadIdx.x == 0) A.bleaves[blockIdx.x] = tot;
    if (in) {
        A.lbytes[s] = eb;
        A.lkids[s] = ek;
        A.lleaves[s] = el;
    }
    // the replaced payload and the selected slots, per block (a counter word that every wave of
    // the grid adds to would make its L2 channel the kernel's bound)
    const uint64_t ob = wave_sum<uint64_t>(od.heap), ok = wave_sum<uint64_t>(od.kid);
    const uint64_t na = (uint64_t)__popcll(__ballot(sel));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][w] = ob, red[1][w] = ok, red[2][w] = na;
    __syncthreads();
    if (threadIdx.x < 3) {
        uint64_t t = 0;
#pragma unroll
        for (int i = 0; i < VT_WAVES; i++) t += red[threadIdx.x][i];
        A.bold[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

namespace {
// exclusive scan over the VT_TOP_WIDTH threads of the top kernel: the waves' sums are scanned by
// wave 0; tmp: VT_TOP_WIDTH / 64 + 1 words
NXG_DEV uint64_t top_scan(uint64_t v, uint64_t* tmp, uint64_t* total) {
    constexpr uint32_t NW = VT_TOP_WIDTH / 64;
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
}  // namespace

__global__ __launch_bounds__(VT_TOP_WIDTH) void nxg_vt_top_kernel(NxgVtArgs A, uint64_t nb) {
    __shared__ uint64_t tmp[VT_TOP_WIDTH / 64 + 1];
    uint64_t cb = 0, ck = 0, cl = 0, pob = 0, pok = 0, pna = 0;
#pragma unroll 1
    for (uint64_t b0 = 0; b0 < nb; b0 += VT_TOP_WIDTH) {
        const uint64_t b = b0 + threadIdx.x;
        const bool in = b < nb;
        uint64_t tot;
        if (in) pob += A.bold[b], pok += A.bold[nb + b], pna += A.bold[2 * nb + b];
        const uint64_t eb = top_scan(in ? A.bbytes[b] : 0, tmp, &tot);
        if (in) A.bbytes[b] = cb + eb;
        cb += tot;
        const uint64_t ek = top_scan(in ? A.bkids[b] : 0, tmp, &tot);
        if (in) A.bkids[b] = ck + ek;
        ck += tot;
        const uint64_t el = top_scan(in ? A.bleaves[b] : 0, tmp, &tot);
        if (in) A.bleaves[b] = cl + el;
        cl += tot;
    }
    uint64_t tob, tok, tna;
    top_scan(pob, tmp, &tob);
    top_scan(pok, tmp, &tok);
    top_scan(pna, tmp, &tna);
    if (threadIdx.x == 0) {
        NxgVtHead* h = A.head;
        h->old_bytes = tob;
        h->old_children = tok;
        h->n_applied = tna;
        h->need_bytes = cb;
        h->need_children = ck;
        h->n_leaves = cl;
        const bool fits = cb <= A.dst.cap_bytes - A.dst.heap_used &&
                          ck <= A.dst.cap_children - A.dst.child_used;
        h->seg_short = cl > A.seg_cap;
        const bool ok = !h->err_inv && fits && cl <= A.seg_cap;
        if (ok) A.seg_dst[cl] = A.dst.heap_used + cb;  // the list's end
        h->ok = ok;
    }
}

__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_place_kernel(NxgVtArgs A) {
    __shared__ uint64_t stks[VT_WAVES][3 * VT_MAX_DEPTH];
    if (!A.head->ok) return;
    const uint64_t s = (uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x;
    const bool in = s < A.dst.n_slots;
    uint32_t mode = 0;
    uint64_t row = 0;
    if (in) source_of(A, s, mode, row);
    Pos p{0, 0, 0};
    if (in) {
        p.heap = A.dst.heap_used + A.bbytes[blockIdx.x] + A.lbytes[s];
        p.kid = A.dst.child_used + A.bkids[blockIdx.x] + A.lkids[s];
        p.leaf = A.bleaves[blockIdx.x] + A.lleaves[s];
    }
    const NxgVtSrc S = pick(A, mode == 1);
    walk_value<true>(A, S, mode == 1 || mode == 2, row, s, p, stks[threadIdx.x >> 6]);
    if (mode == 3) put<true>(A.dst, false, s, 16u, 0, 0);  // Value::Null
}

namespace {
struct __attribute__((packed, aligned(1))) Bytes16 {
    uint32_t w[4];
};
}  // namespace

__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_copy_kernel(NxgVtArgs A) {
    const NxgVtHead* h = A.head;
    if (!h->ok || !h->need_bytes) return;
    const uint64_t lo = A.dst.heap_used, hi = lo + h->need_bytes, nseg = h->n_leaves;
    uint8_t* heap = A.dst.heap;
    // blocks by address: block b covers heap offsets [b * 16 - ph, b * 16 - ph + 16)
    const uint64_t ph = (uint64_t)(uintptr_t)heap & (VT_COPY_BLOCK - 1);
    const uint64_t b_first = (lo + ph) / VT_COPY_BLOCK, b_end = (hi + ph + VT_COPY_BLOCK - 1) / VT_COPY_BLOCK;
    const uint64_t n_chunks = (b_end - b_first + 63) / 64;
    const uint32_t lane = lane_id();
#pragma unroll 1
    for (uint64_t ch = (uint64_t)blockIdx.x * VT_WAVES + (threadIdx.x >> 6); ch < n_chunks;
         ch += (uint64_t)gridDim.x * VT_WAVES) {
        const uint64_t cb0 = b_first + ch * 64;
        // the wave's bytes [w_lo, w_hi) and the segments that touch them [i0, i1)
        const uint64_t c_lo = cb0 * VT_COPY_BLOCK, c_hi = c_lo + 64 * VT_COPY_BLOCK;
        const uint64_t w_lo = c_lo > lo + ph ? c_lo - ph : lo;
        const uint64_t w_hi = c_hi < hi + ph ? c_hi - ph : hi;
        const uint64_t i0 = wave_lower_bound(A.seg_dst, nseg, w_lo + 1) - 1;  // seg_dst[0] = lo
        const uint64_t i1 = wave_lower_bound(A.seg_dst, nseg, w_hi);
        const uint64_t a_lo = (cb0 + lane) * VT_COPY_BLOCK, a_hi = a_lo + VT_COPY_BLOCK;
        if (a_lo >= hi + ph || a_hi <= lo + ph) continue;  // (after the wave's collective calls)
        const uint64_t b_lo = a_lo > lo + ph ? a_lo - ph : lo;
        const uint64_t b_hi = a_hi < hi + ph ? a_hi - ph : hi;
        uint64_t l = i0, r = i1;  // seg_dst[l] <= b_lo; the block's first segment is in [l, r)
#pragma unroll 1
        while (r - l > 1) {
            const uint64_t m = l + (r - l) / 2;
            if (A.seg_dst[m] <= b_lo) l = m;
            else r = m;
        }
        uint64_t s_lo = A.seg_dst[l], s_hi = A.seg_dst[l + 1];
        const uint8_t* src = (const uint8_t*)(uintptr_t)A.seg_src[l];
        if (b_hi - b_lo == VT_COPY_BLOCK && s_hi >= b_hi) {
            const Bytes16 v = *reinterpret_cast<const Bytes16*>(src + (b_lo - s_lo));
            *reinterpret_cast<uint4*>(heap + b_lo) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
        } else {
#pragma unroll 1
            for (uint64_t q = b_lo; q < b_hi; q++) {
                while (q >= s_hi) {  // no segment is empty and the last ends at hi
                    l++;
                    s_lo = s_hi;
                    s_hi = A.seg_dst[l + 1];
                    src = (const uint8_t*)(uintptr_t)A.seg_src[l];
                }
                heap[q] = src[q - s_lo];
            }
        }
    }
}

// ---- an F64 table: only `fixed` ------------------------------------------------------------
__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_f64_check_kernel(NxgVtArgs A) {
    // a bounded grid strides over the slots, so that the counter is added to once per wave of the
    // grid, not once per 64 slots
    uint64_t na = 0;
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll 1
    for (uint64_t s = (uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x;
         s - lane < A.dst.n_slots; s += (uint64_t)gridDim.x * VT_SLOTS_PER_BLOCK) {
        uint64_t r = 0;
        if (s < A.dst.n_slots && A.src_row && s < A.n_sel) r = A.src_row[s];
        if (r) {
            if (r - 1 >= A.batch.n_rows) refuse(A.head, s, kVtRow);
            else if (A.batch.tag && A.batch.tag[r - 1] != 9) refuse(A.head, s, kVtNotF64);
        }
        na += (uint64_t)__popcll(__ballot(r != 0));
    }
    if (lane == 0 && na)
        atomicAdd((unsigned long long*)&A.head->n_applied, (unsigned long long)na);
}

// fixed[s] = batch.fixed[src_row[s] - 1], two slots per lane: 16-byte accesses of src_row and of
// fixed where both arrays are 16-byte aligned (and, in place, where both slots are selected)
__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_f64_gather_kernel(NxgVtArgs A) {
    if (A.head->err_inv) return;
    const uint64_t s = 2 * ((uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x);
    const uint64_t n = A.dst.n_slots;
    if (s >= n) return;
    const bool two = s + 1 < n;
    const bool wide = two && s + 1 < A.n_sel && A.src_row &&
                      ((((uintptr_t)A.src_row | (uintptr_t)A.dst.fixed) & 15) == 0);
    uint64_t r[2] = {0, 0};
    if (wide) {
        const ulonglong2 rr = *reinterpret_cast<const ulonglong2*>(A.src_row + s);
        r[0] = rr.x, r[1] = rr.y;
    } else if (A.src_row) {
        if (s < A.n_sel) r[0] = A.src_row[s];
        if (two && s + 1 < A.n_sel) r[1] = A.src_row[s + 1];
    }
    uint64_t v[2];
    bool w[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint64_t sk = s + k;
        w[k] = (k == 0 || two) && (r[k] != 0 || A.rebuild);
        v[k] = 0;
        if (r[k]) v[k] = A.batch.fixed[r[k] - 1];
        else if (w[k] && sk < A.n_sel) v[k] = A.old.fixed[sk];
    }
    if (wide && w[0] && w[1]) {
        *reinterpret_cast<ulonglong2*>(A.dst.fixed + s) = make_ulonglong2(v[0], v[1]);
    } else {
        if (w[0]) A.dst.fixed[s] = v[0];
        if (w[1]) A.dst.fixed[s + 1] = v[1];
    }
}

// ---- set_unsubscribed -------------------------------------------------------------------------
// the named slots' old values leave the live counts, each slot once (its bit in the zeroed bitmap)
__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_unsub_size_kernel(
    NxgVtArgs A, const uint32_t* __restrict__ slot, uint64_t n) {
    __shared__ uint64_t stks[VT_WAVES][3 * VT_MAX_DEPTH];
    const uint64_t i = (uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x;
    bool first = false;
    uint64_t s = 0;
    if (i < n) {
        s = slot[i];
        if (s >= A.dst.n_slots) refuse(A.head, s, kVtSlot);
        else first = !(atomicOr(&A.bitmap[s >> 5], 1u << (s & 31)) & (1u << (s & 31)));
    }
    Pos od{0, 0, 0};
    const uint32_t c = walk_value<false>(A, A.old, first, s, s, od, stks[threadIdx.x >> 6]);
    if (c) {
        refuse(A.head, s, c | kVtOld);
        od = Pos{0, 0, 0};
    }
    const uint64_t ob = wave_sum<uint64_t>(od.heap), ok = wave_sum<uint64_t>(od.kid);
    const uint32_t na = (uint32_t)__popcll(__ballot(first));
    if ((threadIdx.x & 63) == 0) {
        if (ob) atomicAdd((unsigned long long*)&A.head->old_bytes, (unsigned long long)ob);
        if (ok) atomicAdd((unsigned long long*)&A.head->old_children, (unsigned long long)ok);
        if (na) atomicAdd((unsigned long long*)&A.head->n_applied, (unsigned long long)na);
    }
}

__global__ __launch_bounds__(VT_SLOTS_PER_BLOCK) void nxg_vt_unsub_place_kernel(
    NxgVtArgs A, const uint32_t* __restrict__ slot, uint64_t n) {
    if (A.head->err_inv) return;
    const uint64_t i = (uint64_t)blockIdx.x * VT_SLOTS_PER_BLOCK + threadIdx.x;
    if (i < n) put<true>(A.dst, false, slot[i], NXG_TAG_UNSUBSCRIBED, 0, 0);
}

// ---- launch (host) ------------------------------------------------------------------------------
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

// Each path gets the scratch it uses, after the 256 bytes of the head: the mixed passes their
// per-slot prefixes, block arrays and segment list; set_unsubscribed its bitmap; an F64 table
// nothing. Returns the bytes laid out.
uint64_t vt_layout(NxgVtArgs& a, uint8_t* p, uint64_t n_slots, uint64_t seg_cap, int path) {
    const uint64_t nb = (n_slots + kVtBlock - 1) / kVtBlock;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgVtHead*>(take(256));
    a.seg_cap = seg_cap;
    if (path == kVtPathMixed) {
        a.lbytes = reinterpret_cast<uint64_t*>(take(8 * n_slots));
        a.lkids = reinterpret_cast<uint64_t*>(take(8 * n_slots));
        a.lleaves = reinterpret_cast<uint64_t*>(take(8 * n_slots));
        a.bbytes = reinterpret_cast<uint64_t*>(take(8 * nb));
        a.bkids = reinterpret_cast<uint64_t*>(take(8 * nb));
        a.bleaves = reinterpret_cast<uint64_t*>(take(8 * nb));
        a.bold = reinterpret_cast<uint64_t*>(take(3 * 8 * nb));
        a.seg_dst = reinterpret_cast<uint64_t*>(take(8 * (seg_cap + 1)));
        a.seg_src = reinterpret_cast<uint64_t*>(take(8 * seg_cap));
    } else if (path == kVtPathUnsub) {
        a.bitmap = reinterpret_cast<uint32_t*>(take(4 * ((n_slots + 31) / 32)));
    }
    return o;
}
}  // namespace

uint64_t nxg_vt_scratch_bytes(uint64_t n_slots, uint64_t seg_cap, int path) {
    NxgVtArgs a{};
    return vt_layout(a, nullptr, n_slots, seg_cap, path);
}

#ifndef NXG_VT_COPY_GCAP
#define NXG_VT_COPY_GCAP 16  // the copy kernel's workgroups per CU (a bounded grid over the range)
#endif
hipError_t nxg_launch_vt_apply(NxgVtArgs a, uint8_t* scratch, int ncu, hipStream_t s) {
    const uint64_t n = a.dst.n_slots;
    vt_layout(a, scratch, n, a.seg_cap, a.dst.tag ? kVtPathMixed : kVtPathF64);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgVtHead), s);
    if (e != hipSuccess || n == 0) return e;
    const uint32_t nb = (uint32_t)((n + kVtBlock - 1) / kVtBlock);
    if (!a.dst.tag) {
        const uint32_t gc = nb < (uint32_t)ncu * 8u ? nb : (uint32_t)ncu * 8u;
        hipLaunchKernelGGL(nxg_vt_f64_check_kernel, dim3(gc), dim3(kVtBlock), 0, s, a);
        hipLaunchKernelGGL(nxg_vt_f64_gather_kernel, dim3((nb + 1) / 2), dim3(kVtBlock), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(nxg_vt_size_kernel, dim3(nb), dim3(kVtBlock), 0, s, a);
    hipLaunchKernelGGL(nxg_vt_top_kernel, dim3(1), dim3(VT_TOP_WIDTH), 0, s, a, (uint64_t)nb);
    hipLaunchKernelGGL(nxg_vt_place_kernel, dim3(nb), dim3(kVtBlock), 0, s, a);
    // the new heap range is known only on the device: a bounded grid strides over it
    const uint64_t room = a.dst.cap_bytes - a.dst.heap_used;
    const uint64_t chunks = (room + 1023) / 1024 + 1;
    const uint64_t want = (chunks + VT_WAVES - 1) / VT_WAVES;
    const uint32_t g = (uint32_t)(want < (uint64_t)ncu * NXG_VT_COPY_GCAP
                                      ? want : (uint64_t)ncu * NXG_VT_COPY_GCAP);
    if (room) hipLaunchKernelGGL(nxg_vt_copy_kernel, dim3(g), dim3(kVtBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t nxg_launch_vt_unsub(NxgVtArgs a, const uint32_t* slot, uint64_t n, uint8_t* scratch,
                               hipStream_t s) {
    vt_layout(a, scratch, a.dst.n_slots, 0, kVtPathUnsub);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgVtHead), s);
    if (e != hipSuccess || n == 0) return e;
    if ((e = hipMemsetAsync(a.bitmap, 0, 4 * ((a.dst.n_slots + 31) / 32), s)) != hipSuccess)
        return e;
    const uint32_t g = (uint32_t)((n + kVtBlock - 1) / kVtBlock);
    hipLaunchKernelGGL(nxg_vt_unsub_size_kernel, dim3(g), dim3(kVtBlock), 0, s, a, slot, n);
    hipLaunchKernelGGL(nxg_vt_unsub_place_kernel, dim3(g), dim3(kVtBlock), 0, s, a, slot, n);
    return hipGetLastError();
}
