// nxg_path_probe.h -- how the kernels read a path and probe an NxgPtView with it: bytes taken
// eight at a time from the covering aligned words (an aligned read never leaves the page of the
// bytes it covers), the hash of nxg_path_hash.h with the plain-path check folded in, and the
// byte-confirmed lookup. Shared by nxg_route_subscribes.hip (by_path) and nxg_route_replies.hip
// (the subscriber's pending requests).
#pragma once
#include "nxg_device.h"
#include "nxg_internal.h"
#include "nxg_path_hash.h"

namespace nxgprobe {

// up to 8 bytes from two adjacent aligned words: bytes sh .. sh + n of (lo, hi), zero above n
NXG_DEV uint64_t take8(uint64_t lo, uint64_t hi, uint32_t sh, uint32_t n) {
    const uint64_t v = sh ? (lo >> (8 * sh)) | (hi << (64 - 8 * sh)) : lo;
    return n >= 8 ? v : v & ((1ull << (8 * n)) - 1ull);
}

// bytes in global memory
struct GSrc {
    const uint8_t* g;
    NXG_DEV uint64_t word(uint64_t p, uint32_t n) const {  // n in 0..8
        if (!n) return 0;
        const uintptr_t a = (uintptr_t)(g + p);
        const uint64_t* w = reinterpret_cast<const uint64_t*>(a & ~(uintptr_t)7);
        const uint32_t sh = (uint32_t)(a & 7u);
        return take8(w[0], sh + n > 8 ? w[1] : 0ull, sh, n);
    }
    NXG_DEV uint32_t byte(uint64_t p) const { return g[p]; }
};

// 0x80 in every byte of x that equals c
NXG_DEV uint64_t eq_bytes(uint64_t x, uint8_t c) {
    const uint64_t k7 = 0x7f7f7f7f7f7f7f7full;
    x ^= 0x0101010101010101ull * c;
    return ~(((x & k7) + k7) | x | k7);
}

// the hash of path bytes [p, p + len) (nxg_path_hash.h), and whether the path is plain
template <typename S>
NXG_DEV uint64_t path_hash(const S& s, uint64_t p, uint32_t len, bool* plain) {
    uint64_t h = nxgpath::kSeed ^ len;
    uint64_t bad = 0, prev_slash = 0, w = 0;
    for (uint32_t i = 0; i < len; i += 8) {
        w = s.word(p + i, len - i < 8 ? len - i : 8);
        h = nxgpath::mix(h, w);
        const uint64_t sl = eq_bytes(w, '/');
        bad |= eq_bytes(w, '\\') | (sl & (sl >> 8)) | (sl & prev_slash);
        prev_slash = sl >> 56;  // the word's last byte, as the next word's byte 0 sees it
    }
    if (plain) {
        const uint32_t last = len ? (uint32_t)(w >> (8 * ((len - 1) & 7))) & 0xffu : 0u;
        *plain = len && !bad && (last != '/' || len == 1);
    }
    return nxgpath::finish_hash(h);
}
// a's bytes [pa, pa + n) == b's bytes [pb, pb + n)
template <typename A, typename B>
NXG_DEV bool bytes_eq(const A& a, uint64_t pa, const B& b, uint64_t pb, uint32_t n) {
    uint64_t d = 0;
    for (uint32_t i = 0; i < n && !d; i += 8) {
        const uint32_t m = n - i < 8 ? n - i : 8;
        d = a.word(pa + i, m) ^ b.word(pb + i, m);
    }
    return !d;
}

// the slot of the key s[p ..+len) with hash h, or ~0
template <typename S>
NXG_DEV uint64_t pt_find(const NxgPtView& t, const S& s, uint64_t p, uint32_t len, uint64_t h) {
    const GSrc heap{t.heap};
    uint64_t i = h & t.mask;
    for (uint64_t n = 0; n <= t.mask; n++, i = (i + 1) & t.mask) {
        const uint64_t w = t.hash[i];
        if (w == 0) return ~0ull;
        if (w == h && t.key_len[i] == len && bytes_eq(s, p, heap, t.key_off[i], len)) return i;
    }
    return ~0ull;
}

}  // namespace nxgprobe
