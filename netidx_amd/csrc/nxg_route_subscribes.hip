// nxg_route_subscribes.hip -- a connection's Subscribe bursts answered on gfx950: the device-
// resident by_path (NxgPathTable) and the Subscribe arm of ClientCtx::handle_batch_inner plus
// subscribe() (netidx/src/publisher/server.rs:60-137, 506-549) for one run of consecutive Subscribe
// spans of a decoded To frame.
//
// The path table: open addressing, linear probing, one 64-bit hash word per slot (0 empty, 1
// tombstone, else the key's hash). A hit is a hash match confirmed by every byte of the key. Keys
// are hashed and compared eight bytes at a time from the covering aligned words (an aligned read
// never leaves the page of the bytes it covers; the table's own heap has 16 spare bytes).
//   insert  hash   the path's hash, and whether the table already has it (it then keeps its Id)
//           claim  the call's remaining paths meet in a scratch table of indices: equal paths find
//                  the same word, and atomicMin leaves the lowest index there
//           place  an index that still owns its word is a winner and takes the first free slot of
//                  its chain (CAS); the winners are distinct, so they never compare keys. Which
//                  slot a key gets depends on scheduling; what a lookup answers does not.
//   remove  the slot's hash word goes to 1 by CAS: of two removals of one path, one finds it
//   rehash  the live entries into fresh arrays (the host does this when tombstones pile up)
//
// Routing, per Subscribe span k of the run, in the reference's order (server.rs:68-135):
//   2 Denied          span_perm[k] == NXG_SUB_PERM_DENY (server.rs:520-535), or the path resolves,
//                     by_id has the Id and allow_of_id[id] == 0 (server.rs:98-106)
//   3 deferred        not in by_path, the greatest base <= path is a byte prefix of it, and fewer
//                     than deferred_room spans of the call were deferred before (server.rs:74-87)
//   1 NoSuchValue     not in by_path, otherwise (the `_` arm, server.rs:88-91)
//   4 ignored         in by_path, but by_id has no such Id (server.rs:97)
//   0 Subscribed      otherwise: Subscribed(path, id, current) (server.rs:125-126)
// The run ends in front of the first span that is no Subscribe, has a Write row in front of it
// (ctl_row != row_begin), or whose path is not plain (a `\`, empty, `//`, a trailing `/`).
//
// Everything whose place depends on what precedes it comes from block sums scanned by a one-
// workgroup kernel between launches; no kernel waits on another workgroup. Launches, in order:
//   find     the first span at or after ctl_begin that is no Subscribe of this row (atomicMax of ~k)
//   resolve  per span: the path's place in the frame, plain or not (a span that is not lowers the
//            stop), its hash, the table probe, the verdict (deferral candidates undecided), the
//            current value's size; block sums of the candidates
//   top      exclusive scan of those
//   size     per span of the run: candidate -> deferred (rank < deferred_room) or NoSuchValue, the
//            reply's size; block sums of bytes, replies, Subscribed spans and spans per outcome
//   top      exclusive scans of those, totals into the head
//   emit     outcome[], span_id[], sub_id[] / sub_perm[], deferred[], the replies
// resolve and emit read frame bytes per span: a workgroup first copies the bytes of its spans
// (adjacent in the frame: a run has no rows in between) into LDS with dense aligned loads, and the
// lanes read their paths from there (24 KiB; what lies past that window is read from global
// memory). Measured against lanes reading global memory throughout, 10^6 Subscribes with paths of
// 24-40 bytes: 0.427 ms against 0.468 ms for the whole call.
// Wire forms, L = lw(|body|):
//   NoSuchValue(path)            varint(L) 00 varint(|p|) p
//   Denied(path)                 varint(L) 01 varint(|p|) p
//   Subscribed(path, id, value)  varint(L) 03 varint(|p|) p varint(id) Value
#include <algorithm>

#include "nxg_device.h"
#include "nxg_internal.h"
#include "nxg_path_probe.h"
#include "nxg_value_enc.h"

namespace {

using namespace nxgenc;
using namespace nxgprobe;  // GSrc, path_hash, bytes_eq, pt_find

constexpr int TPB = kRwBlock;
constexpr uint32_t kStage = 24 * 1024;  // LDS bytes for a workgroup's span bytes
constexpr uint8_t kRsCandidate = 5;     // pre[]: not in by_path, its base is a prefix
constexpr uint8_t kRsNone = 0xff;       // pre[]: not a span of the run
constexpr uint64_t kEmptyIdx = ~0ull;

// frame bytes, the window [a0, a0 + nb) of addresses from LDS
struct LSrc {
    const uint8_t* g;
    const uint64_t* lds;
    uintptr_t a0;  // 8-byte aligned
    uint32_t nb;   // a multiple of 8
    NXG_DEV uint64_t word(uint64_t p, uint32_t n) const {
        if (!n) return 0;
        const uintptr_t a = (uintptr_t)(g + p);
        const uint32_t sh = (uint32_t)(a & 7u);
        if (a >= a0 && a + n <= a0 + nb) {
            const uint32_t i = (uint32_t)((a - a0) >> 3);
            return take8(lds[i], sh + n > 8 ? lds[i + 1] : 0ull, sh, n);
        }
        const uint64_t* w = reinterpret_cast<const uint64_t*>(a & ~(uintptr_t)7);
        return take8(w[0], sh + n > 8 ? w[1] : 0ull, sh, n);
    }
    NXG_DEV uint32_t byte(uint64_t p) const { return (uint32_t)word(p, 1); }
};

// byte order of a[pa ..+la) against b[pb ..+lb): < 0, 0, > 0 (a shorter prefix is smaller)
template <typename A, typename B>
NXG_DEV int bytes_cmp(const A& a, uint64_t pa, uint32_t la, const B& b, uint64_t pb, uint32_t lb) {
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; i += 8) {
        const uint32_t m = n - i < 8 ? n - i : 8;
        const uint64_t x = a.word(pa + i, m), y = b.word(pb + i, m);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// bytes go out one at a time behind a capacity check (an overflow is reported from reply_len)
struct CapOut {
    uint8_t* o;
    uint64_t p, cap;
    NXG_DEV void b(uint32_t x) {
        if (p < cap) o[p] = (uint8_t)x;
        p++;
    }
    NXG_DEV void be(uint64_t v, int n) {
        for (int i = n - 1; i >= 0; i--) b((uint32_t)(v >> (8 * i)));
    }
    NXG_DEV void var(uint64_t v) {
        while (v >= 0x80) {
            b((uint32_t)((v & 0x7f) | 0x80));
            v >>= 7;
        }
        b((uint32_t)v);
    }
    NXG_DEV void copy(const uint8_t* src, uint64_t n) {
        for (uint64_t i = 0; i < n; i++) b(src[i]);
    }
};

// the stop as the kernels after `find` (s0) and after `resolve` (final) read it
NXG_DEV uint64_t stop_of(const NxgRsArgs& a) {
    const uint64_t v = a.head->stop_inv;
    return v ? ~v : a.n_ctl;
}

// The workgroup's spans [k0, k1) staged: their frame bytes from the first span's start, kStage
// at most, copied with dense aligned 8-byte loads. Block-wide (contains __syncthreads).
NXG_DEV LSrc stage_spans(const NxgRsArgs& a, uint64_t k0, uint64_t k1, uint64_t* lds) {
    LSrc s{a.frame, lds, 0, 0};
    if (k0 < k1) {
        const uintptr_t b = (uintptr_t)(a.frame + a.ctl_off[k0]);
        const uintptr_t e = (uintptr_t)(a.frame + a.ctl_off[k1 - 1] + a.ctl_len[k1 - 1]);
        s.a0 = b & ~(uintptr_t)7;
        const uintptr_t e8 = (e + 7) & ~(uintptr_t)7;
        s.nb = e8 <= s.a0 ? 0u : e8 - s.a0 < kStage ? (uint32_t)(e8 - s.a0) : kStage;
        const uint64_t* w = reinterpret_cast<const uint64_t*>(s.a0);
        for (uint32_t i = threadIdx.x; i < s.nb / 8; i += TPB) lds[i] = w[i];
    }
    __syncthreads();
    return s;
}

// the current value of a Subscribed span: its root slot from the table's columns
NXG_DEV Slot cur_slot(const NxgRsArgs& a, uint32_t slot) {
    return Slot{a.cur.tag ? a.cur.tag[slot] : 9u, a.cur.fixed[slot], a.cur.aux ? a.cur.aux[slot] : 0u};
}
NXG_DEV uint64_t kids_of(const Slot& v) { return v.tag == 22 ? 1ull : v.tag == 19 ? v.aux : 2ull * v.aux; }

}  // namespace

// ---- the path table ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void nxg_pt_hash_kernel(NxgPtView t, uint64_t heap_base,
                                                          const uint64_t* off, uint64_t n,
                                                          uint64_t* h, uint8_t* state) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const GSrc s{t.heap};
    const uint64_t p = heap_base + off[i];
    const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
    const uint64_t hv = path_hash(s, p, len, nullptr);
    h[i] = hv;
    state[i] = pt_find(t, s, p, len, hv) != ~0ull ? 1 : 0;  // 1: the table has it
}

__global__ __launch_bounds__(TPB) void nxg_pt_claim_kernel(NxgPtView t, uint64_t heap_base,
                                                           const uint64_t* off, uint64_t n,
                                                           const uint64_t* h, const uint8_t* state,
                                                           uint64_t* tmp, uint64_t tmp_mask,
                                                           uint64_t* tslot) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n || state[i]) return;
    const GSrc s{t.heap};
    const uint64_t p = heap_base + off[i], hv = h[i];
    const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
    uint64_t q = hv & tmp_mask;
    for (uint64_t probes = 0; probes <= tmp_mask; probes++, q = (q + 1) & tmp_mask) {
        unsigned long long cur = tmp[q];
        if (cur == kEmptyIdx) {
            cur = atomicCAS((unsigned long long*)&tmp[q], (unsigned long long)kEmptyIdx,
                            (unsigned long long)i);
            if (cur == kEmptyIdx) break;  // the word is this path's (so far)
        }
        // the word holds an index of a path of this call: the same path, or another
        const uint64_t j = cur;
        if (h[j] == hv && (uint32_t)(off[j + 1] - off[j]) == len &&
            bytes_eq(s, p, s, heap_base + off[j], len)) {
            atomicMin((unsigned long long*)&tmp[q], (unsigned long long)i);
            break;
        }
    }
    tslot[i] = q;
}

__global__ __launch_bounds__(TPB) void nxg_pt_place_kernel(NxgPtView t, uint64_t heap_base,
                                                           const uint64_t* off, const uint64_t* id,
                                                           uint64_t n, const uint64_t* h,
                                                           const uint8_t* state, const uint64_t* tmp,
                                                           const uint64_t* tslot, NxgPtHead* head) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    bool dup = false, fresh = false;
    if (i < n) {
        dup = state[i] || tmp[tslot[i]] != i;
        if (!dup) {
            const uint64_t hv = h[i];
            uint64_t q = hv & t.mask;
            for (uint64_t probes = 0; probes <= t.mask; probes++, q = (q + 1) & t.mask) {
                unsigned long long w = t.hash[q];
                if (w > 1) continue;
                const unsigned long long old = atomicCAS((unsigned long long*)&t.hash[q], w,
                                                         (unsigned long long)hv);
                if (old == w) {
                    t.key_off[q] = heap_base + off[i];
                    t.key_len[q] = (uint32_t)(off[i + 1] - off[i]);
                    t.id[q] = id[i];
                    fresh = w == 0;
                    break;
                }
            }
        }
    }
    const uint64_t md = __ballot(dup), mf = __ballot(fresh);
    if ((threadIdx.x & 63) == 0) {
        if (md) atomicAdd((unsigned long long*)&head->n_dup, (unsigned long long)__popcll(md));
        if (mf) atomicAdd((unsigned long long*)&head->n_fresh, (unsigned long long)__popcll(mf));
    }
}

__global__ __launch_bounds__(TPB) void nxg_pt_remove_kernel(NxgPtView t, const uint8_t* keys,
                                                            const uint64_t* off, uint64_t n,
                                                            NxgPtHead* head) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    bool missing = false;
    if (i < n) {
        const GSrc s{keys};
        const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
        const uint64_t hv = path_hash(s, off[i], len, nullptr);
        const uint64_t q = pt_find(t, s, off[i], len, hv);
        // of several removals of one path, one swaps the hash out
        missing = q == ~0ull || atomicCAS((unsigned long long*)&t.hash[q], (unsigned long long)hv,
                                          1ull) != hv;
    }
    const uint64_t mm = __ballot(missing);
    if ((threadIdx.x & 63) == 0 && mm)
        atomicAdd((unsigned long long*)&head->n_missing, (unsigned long long)__popcll(mm));
}

__global__ __launch_bounds__(TPB) void nxg_pt_lookup_kernel(NxgPtView t, const uint8_t* heap,
                                                            const uint64_t* off, const uint32_t* len,
                                                            uint64_t n, uint64_t* id_out) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const GSrc s{heap};
    const uint64_t hv = path_hash(s, off[i], len[i], nullptr);
    const uint64_t q = pt_find(t, s, off[i], len[i], hv);
    id_out[i] = q == ~0ull ? NXG_NO_ID : t.id[q];
}

__global__ __launch_bounds__(TPB) void nxg_pt_rehash_kernel(NxgPtView from, NxgPtView to) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i > from.mask) return;
    const uint64_t hv = from.hash[i];
    if (hv < 2) return;
    uint64_t q = hv & to.mask;
    for (uint64_t probes = 0; probes <= to.mask; probes++, q = (q + 1) & to.mask) {
        if (to.hash[q]) continue;
        if (atomicCAS((unsigned long long*)&to.hash[q], 0ull, (unsigned long long)hv) == 0ull) {
            to.key_off[q] = from.key_off[i];
            to.key_len[q] = from.key_len[i];
            to.id[q] = from.id[i];
            return;
        }
    }
}

static uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + TPB - 1) / TPB); }

hipError_t nxg_launch_pt_insert(const NxgPtView& t, uint64_t heap_base, const uint64_t* off,
                                const uint64_t* id, uint64_t n, uint64_t* h, uint64_t* tmp,
                                uint64_t tmp_mask, uint64_t* tslot, uint8_t* state,
                                NxgPtHead* head, hipStream_t s) {
    if (!n) return hipSuccess;
    const dim3 g(blocks_of(n)), b(TPB);
    hipLaunchKernelGGL(nxg_pt_hash_kernel, g, b, 0, s, t, heap_base, off, n, h, state);
    hipLaunchKernelGGL(nxg_pt_claim_kernel, g, b, 0, s, t, heap_base, off, n, h, state, tmp,
                       tmp_mask, tslot);
    hipLaunchKernelGGL(nxg_pt_place_kernel, g, b, 0, s, t, heap_base, off, id, n, h, state, tmp,
                       tslot, head);
    return hipGetLastError();
}
hipError_t nxg_launch_pt_remove(const NxgPtView& t, const uint8_t* keys, const uint64_t* off,
                                uint64_t n, NxgPtHead* head, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(nxg_pt_remove_kernel, dim3(blocks_of(n)), dim3(TPB), 0, s, t, keys, off, n,
                       head);
    return hipGetLastError();
}
hipError_t nxg_launch_pt_lookup(const NxgPtView& t, const uint8_t* heap, const uint64_t* off,
                                const uint32_t* len, uint64_t n, uint64_t* id_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(nxg_pt_lookup_kernel, dim3(blocks_of(n)), dim3(TPB), 0, s, t, heap, off, len,
                       n, id_out);
    return hipGetLastError();
}
hipError_t nxg_launch_pt_rehash(const NxgPtView& from, const NxgPtView& to, hipStream_t s) {
    hipLaunchKernelGGL(nxg_pt_rehash_kernel, dim3(blocks_of(from.mask + 1)), dim3(TPB), 0, s, from,
                       to);
    return hipGetLastError();
}

// ---- routing ----------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void nxg_rs_find_kernel(NxgRsArgs a) {
    const uint64_t k = a.ctl_begin + (uint64_t)blockIdx.x * TPB + threadIdx.x;
    const bool end = k < a.n_ctl && (a.ctl_variant[k] != 0 || a.ctl_row[k] != a.row_begin);
    const uint64_t m = __ballot(end);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m))
        atomicMax((unsigned long long*)&a.head->stop_inv, (unsigned long long)~k);
}

namespace {
template <typename S>
NXG_DEV void rs_resolve(const NxgRsArgs& a, const S& src, uint64_t s0, uint64_t* tmp,
                        WalkStack* stk) {
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    const bool live = k < s0;
    uint8_t pre = kRsNone;
    uint64_t id = NXG_NO_ID, vlen = 0;
    Slot v{0, 0, 0};
    bool walk = false;
    if (live) {
        // varint(L) 00 varint(|p|) p ..., validated by the decode (L may be non-canonical)
        uint64_t p = a.ctl_off[k];
        const uint64_t end = p + a.ctl_len[k];
        while (p < end && (src.byte(p) & 0x80)) p++;
        p += 2;  // the length's last byte and the variant
        uint64_t plen = 0;
        for (uint32_t sh = 0; sh < 70 && p < end; sh += 7) {
            const uint32_t c = src.byte(p++);
            if (sh < 64) plen |= (uint64_t)(c & 0x7f) << sh;
            if (c < 0x80) break;
        }
        bool plain = false;
        uint64_t hv = 0;
        if (p <= end && plen <= end - p) hv = path_hash(src, p, (uint32_t)plen, &plain);
        a.poff[j] = p;
        a.plen[j] = (uint32_t)plen;
        if (!plain) {
            atomicMax((unsigned long long*)&a.head->stop_inv, (unsigned long long)~k);
        } else if (a.span_perm && a.span_perm[k] == NXG_SUB_PERM_DENY) {
            pre = NXG_SUB_DENIED;
        } else {
            const uint64_t q = pt_find(a.paths, src, p, (uint32_t)plen, hv);
            if (q == ~0ull) {
                // the greatest base <= path alone is examined (server.rs:74-93)
                const GSrc dh{a.default_heap};
                uint64_t lo = 0, hi = a.n_defaults;
                while (lo < hi) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    const uint64_t b = a.default_off[mid];
                    if (bytes_cmp(dh, b, (uint32_t)(a.default_off[mid + 1] - b), src, p,
                                  (uint32_t)plen) <= 0)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                pre = NXG_SUB_NO_SUCH_VALUE;
                if (lo) {
                    const uint64_t b = a.default_off[lo - 1];
                    const uint64_t bl = a.default_off[lo] - b;
                    if (bl <= plen && bytes_eq(dh, b, src, p, (uint32_t)bl)) pre = kRsCandidate;
                }
            } else {
                id = a.paths.id[q];
                const uint32_t slot = id < a.n_ids ? a.slot_of_id[id] : NXG_NO_SLOT;
                if (slot == NXG_NO_SLOT || slot >= a.n_slots) {
                    pre = NXG_SUB_IGNORED;
                } else if (a.allow_of_id && !a.allow_of_id[id]) {
                    pre = NXG_SUB_DENIED;
                } else {
                    pre = NXG_SUB_SUBSCRIBED;
                    v = cur_slot(a, slot);
                    walk = is_container(v.tag);
                    if (!walk) vlen = scalar_len(v);
                }
            }
        }
    }
    // containers: the root here (level 0, as the encoder counts it), each element's subtree by the
    // shared walk from level 1 (one lane at a time on the wave's LDS stack)
    uint32_t err = 0;
    one_lane_at_a_time(walk, [&] {
        if (!a.cur.ctag || (v.tag != 22 && (uint64_t)v.aux * (v.tag == 19 ? 16 : 32) > kMaxVec)) {
            err = 2;
            return;
        }
        vlen = 1 + (v.tag == 22 ? 0 : vl64(v.aux));
        const uint64_t nk = kids_of(v);
        for (uint64_t c = 0; c < nk && !err; c++)
            vlen += value_len(a.cur, false, v.fixed + c, &err, stk, 1);
    });
    if (live && pre == NXG_SUB_SUBSCRIBED && (err || !vlen)) {
        vlen = 0;
        // the lowest such span wins, and its cause travels in the same word (k < 2^56)
        atomicMax((unsigned long long*)&a.head->bad_inv,
                  (unsigned long long)(~k << 8 | (err ? err : 1u)));
    }
    if (live) {
        a.pre[j] = pre;
        a.sid[j] = id;
        a.vlen[j] = vlen;
    }
    uint64_t total;
    const uint64_t r = block_excl_scan<uint64_t, TPB>(pre == kRsCandidate ? 1ull : 0ull, tmp, &total);
    if (live) a.cloc[j] = (uint32_t)r;
    if (threadIdx.x == 0) a.cblk[blockIdx.x] = total;
}
}  // namespace

__global__ __launch_bounds__(TPB) void nxg_rs_resolve_kernel(NxgRsArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    __shared__ WalkStack wstk[TPB / 64];
    __shared__ uint64_t img[kStage / 8 + 1];
    const uint64_t s0 = stop_of(a), k0 = a.ctl_begin + (uint64_t)blockIdx.x * TPB;
    if (k0 >= s0) return;  // (block-uniform)
    const LSrc src = stage_spans(a, k0, k0 + TPB < s0 ? k0 + TPB : s0, img);
    rs_resolve(a, src, s0, tmp, &wstk[threadIdx.x >> 6]);
}

// one workgroup: each job's v[0 .. nb) scanned in place (exclusive), nb = the blocks that hold
// spans of the run; its total's low 32 bits to *lo and the rest to *hi (hi null: all of it to *lo)
struct NxgRsTop {
    uint64_t* v[5];
    uint64_t* lo[5];
    uint64_t* hi[5];
};
__global__ __launch_bounds__(1024) void nxg_rs_top_kernel(NxgRsArgs a, NxgRsTop t) {
    __shared__ uint64_t tmp[16];
    __shared__ uint64_t carry;
    const uint64_t n = (stop_of(a) - a.ctl_begin + TPB - 1) / TPB;
#pragma unroll 1
    for (int job = 0; job < 5; job++) {
        uint64_t* v = t.v[job];
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
        if (threadIdx.x == 0 && t.lo[job]) {
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

namespace {
// the span's outcome once the candidates before it are known
NXG_DEV uint32_t outcome_of(const NxgRsArgs& a, uint64_t j, uint8_t pre) {
    if (pre != kRsCandidate) return pre;
    return a.cblk[j / TPB] + a.cloc[j] < a.deferred_room ? NXG_SUB_DEFERRED : NXG_SUB_NO_SUCH_VALUE;
}
// |body| of the span's reply (0: none)
NXG_DEV uint64_t body_of(const NxgRsArgs& a, uint64_t j, uint64_t k, uint32_t oc) {
    if (oc == NXG_SUB_DEFERRED || oc == NXG_SUB_IGNORED) return 0;
    const uint64_t pl = a.plen[j];
    uint64_t body = 1 + vl64(pl) + pl;
    if (oc == NXG_SUB_SUBSCRIBED) {
        const uint64_t vlen = a.vlen[j];
        if (!vlen) return 0;  // (the call fails: bad_inv)
        body += vl64(a.sid[j]) + vlen;
    }
    return body;
}
}  // namespace

__global__ __launch_bounds__(TPB) void nxg_rs_size_kernel(NxgRsArgs a) {
    __shared__ uint64_t tmp[TPB / 64];
    const uint64_t stop = stop_of(a);
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    if (a.ctl_begin + (uint64_t)blockIdx.x * TPB >= stop) return;  // (block-uniform)
    const bool live = k < stop;
    uint32_t oc = 0;
    uint64_t size = 0;
    if (live) {
        oc = outcome_of(a, j, a.pre[j]);
        const uint64_t body = body_of(a, j, k, oc);
        size = body ? lwlen(body) : 0;
    }
    // (a block's replies are below 2^40 bytes: a message is at most MAX_BATCH) bytes | replies |
    // Subscribed spans
    const uint64_t sub = live && oc == NXG_SUB_SUBSCRIBED ? 1ull << 52 : 0ull;
    uint64_t total;
    const uint64_t p = block_excl_scan<uint64_t, TPB>(size | (size ? 1ull << 40 : 0ull) | sub, tmp,
                                                      &total);
    if (live) {
        a.zloc[j] = p & ((1ull << 40) - 1);
        a.sloc[j] = (uint32_t)(p >> 52);
    }
    uint64_t five;
    (void)block_excl_scan<uint64_t, TPB>(live ? 1ull << (10 * oc) : 0ull, tmp, &five);
    if (threadIdx.x == 0) {
        const uint64_t nb = gridDim.x;
        const auto f = [&](int q) { return (five >> (10 * q)) & 0x3ffull; };
        a.zblk[blockIdx.x] = total & ((1ull << 40) - 1);
        a.nblk[blockIdx.x] = ((total >> 40) & 0xfffull) | (total >> 52) << 32;
        a.oblk[blockIdx.x] = f(0) | f(1) << 32;
        a.oblk[nb + blockIdx.x] = f(2) | f(3) << 32;
        a.oblk[2 * nb + blockIdx.x] = f(4);
    }
}

namespace {
template <typename S>
NXG_DEV void rs_emit(const NxgRsArgs& a, const S& src, uint64_t stop, WalkStack* stk) {
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x, k = a.ctl_begin + j;
    const bool live = k < stop;
    uint32_t oc = 0;
    uint64_t body = 0, id = NXG_NO_ID;
    Slot v{0, 0, 0};
    CapOut o{a.reply, 0, a.cap_reply};
    if (live) {
        oc = outcome_of(a, j, a.pre[j]);
        a.outcome[k] = (uint8_t)oc;
        a.span_id[k] = a.sid[j];
        body = body_of(a, j, k, oc);
        if (oc == NXG_SUB_DEFERRED) {
            const uint64_t r = a.cblk[j / TPB] + a.cloc[j];
            if (r < a.cap_deferred) a.deferred[r] = k;
        }
        if (oc == NXG_SUB_SUBSCRIBED) {
            id = a.sid[j];
            const uint64_t r = (a.nblk[blockIdx.x] >> 32) + a.sloc[j];
            if (r < a.cap_sub) {
                a.sub_id[r] = id;
                a.sub_perm[r] = a.span_perm ? a.span_perm[k] : 0x3fu;  // Permissions::all()
            }
        }
    }
    bool walk = false;
    if (body) {
        o.p = a.zblk[blockIdx.x] + a.zloc[j];
        const uint32_t pl = a.plen[j];
        const uint64_t pp = a.poff[j];
        o.var(body + vl64(body + vl64(body)));  // L = lw(|body|)
        o.b(oc == NXG_SUB_SUBSCRIBED ? 3u : oc == NXG_SUB_DENIED ? 1u : 0u);
        o.var(pl);
        for (uint32_t i = 0; i < pl; i += 8) {
            const uint32_t m = pl - i < 8 ? pl - i : 8;
            uint64_t w = src.word(pp + i, m);
            for (uint32_t b = 0; b < m; b++, w >>= 8) o.b((uint32_t)w & 0xffu);
        }
        if (oc == NXG_SUB_SUBSCRIBED) {
            o.var(id);
            v = cur_slot(a, a.slot_of_id[id]);
            walk = is_container(v.tag);
            if (!walk) scalar_write(v, a.cur_heap, o);
        }
    }
    one_lane_at_a_time(walk, [&] {
        o.b(v.tag);
        if (v.tag != 22) o.var(v.aux);
        const uint64_t nk = kids_of(v);
        for (uint64_t c = 0; c < nk; c++) value_write(a.cur, a.cur_heap, false, v.fixed + c, o, stk);
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        NxgRsHead* h = a.head;
        h->next_ctl = stop;
        h->stopped = stop >= a.n_ctl ? 0u
                     : a.ctl_variant[stop] == 0 && a.ctl_row[stop] == a.row_begin ? 2u
                                                                                  : 1u;
    }
}
}  // namespace

__global__ __launch_bounds__(TPB) void nxg_rs_emit_kernel(NxgRsArgs a) {
    __shared__ WalkStack wstk[TPB / 64];
    __shared__ uint64_t img[kStage / 8 + 1];
    const uint64_t stop = stop_of(a), k0 = a.ctl_begin + (uint64_t)blockIdx.x * TPB;
    if (k0 >= stop && blockIdx.x) return;  // (block-uniform; block 0 writes the head)
    const LSrc src = stage_spans(a, k0, k0 + TPB < stop ? k0 + TPB : stop, img);
    rs_emit(a, src, stop, &wstk[threadIdx.x >> 6]);
}

uint64_t nxg_rs_scratch_bytes(uint64_t spans) {
    const uint64_t nb = (spans + TPB - 1) / TPB;
    // head | poff, vlen, zloc, sid | plen, cloc, sloc | pre | cblk, zblk, nblk, oblk (three)
    return 128 + spans * (4 * 8 + 3 * 4 + 1) + 8 + nb * 6 * 8 + 64;
}

hipError_t nxg_launch_route_subscribes(NxgRsArgs a, uint8_t* scratch, hipStream_t s) {
    const uint64_t spans = a.n_ctl - a.ctl_begin, nb = (spans + TPB - 1) / TPB;
    uint8_t* p = scratch;
    a.head = reinterpret_cast<NxgRsHead*>(p), p += 128;
    a.poff = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.vlen = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.zloc = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.sid = reinterpret_cast<uint64_t*>(p), p += spans * 8;
    a.cblk = reinterpret_cast<uint64_t*>(p), p += nb * 8;
    a.zblk = reinterpret_cast<uint64_t*>(p), p += nb * 8;
    a.nblk = reinterpret_cast<uint64_t*>(p), p += nb * 8;
    a.oblk = reinterpret_cast<uint64_t*>(p), p += 3 * nb * 8;
    a.plen = reinterpret_cast<uint32_t*>(p), p += spans * 4;
    a.cloc = reinterpret_cast<uint32_t*>(p), p += spans * 4;
    a.sloc = reinterpret_cast<uint32_t*>(p), p += spans * 4;
    a.pre = p;
    hipError_t e;
    if ((e = hipMemsetAsync(a.head, 0, 128, s)) != hipSuccess) return e;
    const dim3 g((uint32_t)std::max<uint64_t>(nb, 1)), b(TPB);
    if (nb) {
        hipLaunchKernelGGL(nxg_rs_find_kernel, g, b, 0, s, a);
        hipLaunchKernelGGL(nxg_rs_resolve_kernel, g, b, 0, s, a);
        NxgRsHead* h = a.head;
        NxgRsTop t{};
        t.v[0] = a.cblk;
        hipLaunchKernelGGL(nxg_rs_top_kernel, dim3(1), dim3(1024), 0, s, a, t);
        hipLaunchKernelGGL(nxg_rs_size_kernel, g, b, 0, s, a);
        t = NxgRsTop{};
        t.v[0] = a.zblk, t.lo[0] = &h->reply_bytes;
        t.v[1] = a.nblk, t.lo[1] = &h->n_replies, t.hi[1] = &h->n_sub;
        t.v[2] = a.oblk, t.lo[2] = &h->n_outcome[0], t.hi[2] = &h->n_outcome[1];
        t.v[3] = a.oblk + nb, t.lo[3] = &h->n_outcome[2], t.hi[3] = &h->n_outcome[3];
        t.v[4] = a.oblk + 2 * nb, t.lo[4] = &h->n_outcome[4];
        hipLaunchKernelGGL(nxg_rs_top_kernel, dim3(1), dim3(1024), 0, s, a, t);
    }
    hipLaunchKernelGGL(nxg_rs_emit_kernel, g, b, 0, s, a);
    return hipGetLastError();
}
