// nxg_value_enc.h -- Value::encode (netidx-value/src/lib.rs:361-468) over columns, on the device:
// the sizing and emit walks shared by the update / write / archive encoder
// (nxg_encode_general.hip) and the Subscribed replies of nxg_route_subscribes.hip. ValArray
// (array.rs:583-593), Map (pack.rs:1212-1223) and Abstract (abstract_type.rs:272-278) included.
//
// A value is a Slot (tag, fixed, aux) of the row columns or of the child columns of a ColsDesc;
// text, Decimal and Abstract bytes are at heap + fixed, a container's elements at child slots
// fixed .. . The emit walks write through any W with b(byte), be(value, n bytes big endian),
// var(varint) and copy(src, n).
#pragma once
#include "nxg_device.h"

namespace nxgenc {

constexpr uint64_t kMaxVec = 2ull * 1024 * 1024 * 1024;

struct Slot {
    uint32_t tag;
    uint64_t fixed;
    uint32_t aux;
};

NXG_DEV Slot get_slot(const ColsDesc& c, bool row, uint64_t i) {
    if (row) return Slot{c.tag[i], c.fixed[i], c.aux[i]};
    return Slot{c.ctag[i], c.cfixed[i], c.caux[i]};
}

NXG_DEV bool is_container(uint32_t tag) { return tag == 19 || tag == 21 || tag == 22; }

// |Value| of a non-container value (tags other than 19, 21, 22); 0 => unknown tag
NXG_DEV uint64_t scalar_len(const Slot& s) {
    switch (s.tag) {
    case 0: case 2: case 8: return 5;
    case 1: return 1 + vl64((uint32_t)s.fixed);
    case 3: return 1 + vl64(zz32((int32_t)(uint32_t)s.fixed));
    case 4: case 6: case 9: return 9;
    case 5: return 1 + vl64(s.fixed);
    case 7: return 1 + vl64(zz64((int64_t)s.fixed));
    case 10: case 11: return 13;
    case 12: case 13: case 18: return 1 + vl64(s.aux) + s.aux;
    case 14: case 15: case 16: return 1;
    case 20: return 17;
    case 23: case 24: return 2;
    case 25: case 26: return 3;
    case 27: return 1 + lwlen(s.aux);
    default: return 0;
    }
}

// The general walk's stack: kStk levels of (children left, next child slot), in LDS, one stack
// per wave (the walk runs one lane at a time: one_lane_at_a_time). Kept out of registers and
// scratch: a dynamically indexed private array would be scratch memory in every wave.
constexpr int kStk = NXG_MAX_DEPTH + 2;
struct WalkStack {
    uint64_t rem[kStk];
    uint64_t slot[kStk];
};

// |Value| for the value in (row?, slot), children included; 0 => error (*err set). The value is
// at nesting level `level` of the Value it belongs to (0: it is the root; a caller that sizes a
// container's root itself walks the elements from level 1): a value at a level past
// NXG_MAX_DEPTH is error 6, so the stack holds at most NXG_MAX_DEPTH + 1 - level frames.
NXG_DEV uint64_t value_len(const ColsDesc& c, bool row, uint64_t slot, uint32_t* err,
                           WalkStack* stk, int level = 0) {
    uint64_t* frem = stk->rem;
    uint64_t* fslot = stk->slot;
    int top = -1, depth = level;
    bool is_row = row;
    uint64_t cur = slot, total = 0;
    for (;;) {
        if (depth > NXG_MAX_DEPTH) {
            *err = 6;
            return 0;
        }
        const Slot s = get_slot(c, is_row, cur);
        uint64_t kids = 0;
        switch (s.tag) {
        case 0: case 2: case 8: total += 5; break;
        case 1: total += 1 + vl64((uint32_t)s.fixed); break;
        case 3: total += 1 + vl64(zz32((int32_t)(uint32_t)s.fixed)); break;
        case 4: case 6: case 9: total += 9; break;
        case 5: total += 1 + vl64(s.fixed); break;
        case 7: total += 1 + vl64(zz64((int64_t)s.fixed)); break;
        case 10: case 11: total += 13; break;
        case 12: case 13: case 18: total += 1 + vl64(s.aux) + s.aux; break;
        case 14: case 15: case 16: total += 1; break;
        case 19:
        case 21:
            if ((uint64_t)s.aux * (s.tag == 19 ? 16 : 32) > kMaxVec) {  // encode guard
                *err = 2;
                return 0;
            }
            total += 1 + vl64(s.aux);
            kids = s.tag == 19 ? s.aux : 2ull * s.aux;
            break;
        case 20: total += 17; break;
        case 22: total += 1; kids = 1; break;
        case 23: case 24: total += 2; break;
        case 25: case 26: total += 3; break;
        case 27: total += 1 + lwlen(s.aux); break;
        default:
            *err = 1;
            return 0;
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
        depth = level + top + 1;
    }
}

template <typename W>
NXG_DEV void value_write(const ColsDesc& c, const uint8_t* heap, bool row, uint64_t slot, W& w,
                         WalkStack* stk) {
    uint64_t* frem = stk->rem;
    uint64_t* fslot = stk->slot;
    int top = -1;
    bool is_row = row;
    uint64_t cur = slot;
    for (;;) {
        const Slot s = get_slot(c, is_row, cur);
        uint64_t kids = 0;
        w.b(s.tag);
        switch (s.tag) {
        case 0: case 2: case 8: w.be(s.fixed, 4); break;
        case 1: w.var((uint32_t)s.fixed); break;
        case 3: w.var(zz32((int32_t)(uint32_t)s.fixed)); break;
        case 4: case 6: case 9: w.be(s.fixed, 8); break;
        case 5: w.var(s.fixed); break;
        case 7: w.var(zz64((int64_t)s.fixed)); break;
        case 10: case 11: w.be(s.fixed, 8); w.be(s.aux, 4); break;
        case 12: case 13: case 18: w.var(s.aux); w.copy(heap + s.fixed, s.aux); break;
        case 19: case 21:
            w.var(s.aux);
            kids = s.tag == 19 ? s.aux : 2ull * s.aux;
            break;
        case 20: w.copy(heap + s.fixed, 16); break;
        case 22: kids = 1; break;
        case 23: case 24: w.be(s.fixed, 1); break;
        case 25: case 26: w.be(s.fixed, 2); break;
        case 27: w.var(lwlen(s.aux)); w.copy(heap + s.fixed, s.aux); break;
        default: break;
        }
        if (kids) {
            ++top;
            frem[top] = kids;
            fslot[top] = s.fixed;
        }
        while (top >= 0 && frem[top] == 0) top--;
        if (top < 0) return;
        frem[top]--;
        cur = fslot[top]++;
        is_row = false;
    }
}

// Writes a non-container value (tag byte included).
template <typename W>
NXG_DEV void scalar_write(const Slot& s, const uint8_t* heap, W& w) {
    w.b(s.tag);
    switch (s.tag) {
    case 0: case 2: case 8: w.be(s.fixed, 4); break;
    case 1: w.var((uint32_t)s.fixed); break;
    case 3: w.var(zz32((int32_t)(uint32_t)s.fixed)); break;
    case 4: case 6: case 9: w.be(s.fixed, 8); break;
    case 5: w.var(s.fixed); break;
    case 7: w.var(zz64((int64_t)s.fixed)); break;
    case 10: case 11: w.be(s.fixed, 8); w.be(s.aux, 4); break;
    case 12: case 13: case 18: w.var(s.aux); w.copy(heap + s.fixed, s.aux); break;
    case 20: w.copy(heap + s.fixed, 16); break;
    case 23: case 24: w.be(s.fixed, 1); break;
    case 25: case 26: w.be(s.fixed, 2); break;
    case 27: w.var(lwlen(s.aux)); w.copy(heap + s.fixed, s.aux); break;
    default: break;
    }
}

}  // namespace nxgenc
