// nxg_record_walk.h -- an Event of the archive's batch items (logfile/mod.rs:188-205: 0x40 for
// Unsubscribed, else the bare Value) sized and written from columns with every child range checked
// before it is read, and the workgroup scan and the writer that go with it. Shared by the kernels
// of nxg_record_entries (nxg_record.hip) and nxg_oneshot_pack_deltas (nxg_oneshot.hip). Device only.
#pragma once
#include "nxg_device.h"
#include "nxg_record.h"
#include "nxg_value_enc.h"

namespace nxgrec {

using namespace nxgenc;

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

// nxgenc::scalar_len with the text kinds' 1 + vl(len) + len summed in 64 bits: a u32 length near
// 2^32 must reach the item bound (kRecBig) and not wrap to a few bytes
NXG_DEV uint64_t scalar_len64(const Slot& s) {
    if (s.tag == 12 || s.tag == 13 || s.tag == 18) return 1ull + vl64(s.aux) + (uint64_t)s.aux;
    return scalar_len(s);
}

// a container's child range [f, f + n): 0, or the cause it is refused for
NXG_DEV uint32_t kids_ok(const ColsDesc& c, uint64_t f, uint64_t n) {
    if (n == 0) return 0;
    if (!c.ctag) return kRecNoKids;
    return (f > c.n_children || n > c.n_children - f) ? kRecKids : 0u;
}

// |Value| of the array row s when no element is a container, in registers. `deep`: an element is
// one (the stack walk sizes the row). 0 with *cause set: refused.
NXG_DEV uint64_t arr_len_flat(const ColsDesc& c, const Slot& s, uint32_t* cause, bool* deep) {
    if ((uint64_t)s.aux * 16 > kMaxVec) {
        *cause = kRecBig;
        return 0;
    }
    if ((*cause = kids_ok(c, s.fixed, s.aux))) return 0;
    uint64_t total = 1 + vl64(s.aux);
#pragma unroll 1
    for (uint64_t k = 0; k < s.aux; k++) {
        const Slot e = get_slot(c, false, s.fixed + k);
        if (is_container(e.tag)) {
            *deep = true;
            return 0;
        }
        const uint64_t l = scalar_len64(e);
        if (!l) {
            *cause = kRecTag;
            return 0;
        }
        total += l;
    }
    return total;
}

// |Value| of row `row`, children included, on the wave's stack (one lane at a time): the walk of
// nxgenc::value_len with every child range checked before it is read. 0 with *cause set: the
// first refusal in walk order.
NXG_DEV uint64_t walk_len(const ColsDesc& c, uint64_t row, uint32_t* cause, WalkStack* stk) {
    uint64_t* frem = stk->rem;
    uint64_t* fslot = stk->slot;
    int top = -1, depth = 0;
    bool is_row = true;
    uint64_t cur = row, total = 0;
#pragma unroll 1
    for (;;) {
        if (depth > NXG_MAX_DEPTH) {
            *cause = kRecDepth;
            return 0;
        }
        const Slot s = get_slot(c, is_row, cur);
        uint64_t kids = 0;
        if (is_container(s.tag)) {
            if (s.tag != 22 && (uint64_t)s.aux * (s.tag == 19 ? 16 : 32) > kMaxVec) {
                *cause = kRecBig;
                return 0;
            }
            kids = s.tag == 19 ? (uint64_t)s.aux : s.tag == 21 ? 2ull * s.aux : 1ull;
            if ((*cause = kids_ok(c, s.fixed, kids))) return 0;
            total += s.tag == 22 ? 1 : 1 + vl64(s.aux);
        } else {
            const uint64_t l = scalar_len64(s);
            if (!l) {
                *cause = kRecTag;
                return 0;
            }
            total += l;
        }
        if (kids) {
            ++top;
            frem[top] = kids;
            fslot[top] = s.fixed;
        }
        while (top >= 0 && frem[top] == 0) top--;
        if (top < 0) return total;
        frem[top]--;
        cur = fslot[top]++;
        is_row = false;
        depth = top + 1;
    }
}

// |Event| of a kept entry: `unsub` (no row is read) or row `row` of c (tag null: F64 layout).
// Scalars and text from the row, flat arrays in registers, everything else one lane at a time on
// the wave's stack. 0 with *cause set: refused. Called by every lane of the workgroup (`kept`
// false: 0), since the stack walk takes the wave's lanes in turn.
NXG_DEV uint64_t event_len(const ColsDesc& c, bool kept, bool unsub, uint64_t row, uint32_t* cause,
                           WalkStack* stk) {
    uint64_t vlen = 0;
    bool deep = false;
    if (kept) {
        if (unsub) {
            vlen = 1;
        } else if (row >= c.n_rows) {
            *cause = kRecRow;
        } else if (!c.tag) {
            vlen = 9;
        } else {
            const Slot s = get_slot(c, true, row);
            if (s.tag == NXG_TAG_UNSUBSCRIBED) {
                vlen = 1;
            } else if (!is_container(s.tag)) {
                vlen = scalar_len64(s);
                if (!vlen) *cause = kRecTag;
            } else if (s.tag == 19) {
                vlen = arr_len_flat(c, s, cause, &deep);
            } else {
                deep = true;
            }
        }
    }
    one_lane_at_a_time(deep, [&] { vlen = walk_len(c, row, cause, stk); });
    return vlen;
}

// the emit kernels' writer: to the LDS staging or straight to the output
struct Wr {
    uint8_t* o;
    uint64_t p;
    NXG_DEV void b(uint32_t x) { o[p++] = (uint8_t)x; }
    NXG_DEV void be(uint64_t v, int n) {
        for (int i = n - 1; i >= 0; i--) o[p++] = (uint8_t)(v >> (8 * i));
    }
    NXG_DEV void var(uint64_t v) {
        while (v >= 0x80) {
            o[p++] = (uint8_t)((v & 0x7f) | 0x80);
            v >>= 7;
        }
        o[p++] = (uint8_t)v;
    }
    // heap bytes. Up to 44: the covering aligned dwords loaded together (a dword-aligned read
    // never leaves the page of the bytes it covers), realigned, then written byte by byte.
    NXG_DEV void copy(const uint8_t* src, uint64_t n) {
        constexpr int NW = 12;
        if (n <= 4 * NW - 4) {
            const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
            const uint32_t* w = reinterpret_cast<const uint32_t*>((uintptr_t)src & ~(uintptr_t)3);
            const uint32_t nw = (uint32_t)((sh + n + 3) >> 2);
            uint32_t d[NW + 1];
#pragma unroll
            for (int i = 0; i < NW; i++) d[i] = (uint32_t)i < nw ? w[i] : 0u;
            d[NW] = 0u;
#pragma unroll
            for (int i = 0; i < NW - 1; i++) {
                const uint32_t e = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if ((uint64_t)(4 * i + k) < n) o[p + 4 * i + k] = (uint8_t)(e >> (8 * k));
            }
            p += n;
            return;
        }
#pragma unroll 1
        for (uint64_t i = 0; i < n; i++) o[p++] = src[i];
    }
};

// The emit kernels' staged tile: `n` bytes that lie in stg[phase, phase + n) go to dst, phase =
// dst & 15, so that staging block b is the 16 bytes at the aligned address dst - phase + 16 b: whole
// blocks as aligned 16-byte stores, bytes at both edges. Called by the NT threads of the workgroup
// after the barrier that publishes stg. Nothing outside [dst, dst + n) is written.
template <int NT>
NXG_DEV void store_staged(uint8_t* dst, uint32_t phase, uint32_t n, const uint8_t* stg) {
    uint8_t* const g0 = reinterpret_cast<uint8_t*>((uintptr_t)dst - phase);
    const uint32_t end = phase + n, nblk = (end + 15) >> 4;
    for (uint32_t b = threadIdx.x; b < nblk; b += NT) {
        if (16 * b >= phase && 16 * b + 16 <= end) {
            *reinterpret_cast<uint4*>(g0 + 16ull * b) = *reinterpret_cast<const uint4*>(stg + 16 * b);
        } else {
            for (uint32_t k = 16 * b; k < 16 * b + 16; k++)
                if (k >= phase && k < end) g0[k] = stg[k];
        }
    }
}

// The Event of a kept entry at w: `unsub`, or row `row` of c (checked by event_len before).
// Called by every lane of the workgroup (`kept` false: nothing written), as event_len is.
NXG_DEV void emit_event(const ColsDesc& c, const uint8_t* heap, bool kept, bool unsub, uint64_t row,
                        Wr& w, WalkStack* stk) {
    bool deep = false;
    if (kept) {
        if (unsub) {
            w.b(NXG_TAG_UNSUBSCRIBED);
        } else if (!c.tag) {
            w.b(9);
            w.be(c.fixed[row], 8);
        } else {
            const Slot s = get_slot(c, true, row);
            if (s.tag == NXG_TAG_UNSUBSCRIBED) {
                w.b(NXG_TAG_UNSUBSCRIBED);
            } else if (!is_container(s.tag)) {
                scalar_write(s, heap, w);
            } else if (s.tag == 19) {
                // flat when no element is a container (their tags first: one byte each)
#pragma unroll 1
                for (uint64_t k = 0; k < s.aux && !deep; k++) deep = is_container(c.ctag[s.fixed + k]);
                if (!deep) {
                    w.b(19);
                    w.var(s.aux);
#pragma unroll 1
                    for (uint64_t k = 0; k < s.aux; k++)
                        scalar_write(get_slot(c, false, s.fixed + k), heap, w);
                }
            } else {
                deep = true;
            }
        }
    }
    one_lane_at_a_time(deep, [&] { value_write(c, heap, true, row, w, stk); });
}

}  // namespace nxgrec
