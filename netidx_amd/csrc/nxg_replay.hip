// nxg_replay.hip -- a decoded archive window (or its image) as publisher update rows
// (nxg_replay_window, nxg_replay_image).
//
// Replaces the playback loop of the recorder's publish session (netidx-archive/src/recorder/
// publish/session_shard.rs:196-245, process_batch) and reimage (session_shard.rs:375-409): each
// BatchItem(id, ev) is looked up in `published` (pub_id_of_arch, with the session's filter folded
// in), dropped when it has no path or the filter refuses it, and otherwise becomes the update
// (publisher Id, value) with Event::Unsubscribed as Value::Null. A row the host has to publish
// first (a miss) stops the window in front of its record.
//
// A position is a window row (window) or an entry of `order` (image). Passes, separate launches,
// none of which waits on another workgroup:
//   classify  tiles of RP_TILE positions, one per lane: the table gather, the class (kept, drop,
//             miss), the kept lanes of each wave as one 64-bit word, the tile's kept count. The
//             tile's records from wave_lower_bound over rend, each position's by bisection between
//             them: position r is in record c iff c is the first record with rend[c] > r, and
//             rbeg[c] <= r. An empty or failed record has rend[c] == rend[c - 1], so it is never
//             that first record, wherever it stands. The lowest record with a miss by one
//             atomicMax per wave that has one.
//   scan      nxg_scan_u32 over the tile counts. They do not depend on where the window stops:
//             kept rows of later records only sit behind the ones that are emitted.
//   bound     one thread per record boundary: rec_off from the tile's sum and the kept words in
//             front of the boundary, clamped to n_done; n_rows, n_done and the verdict head.ok.
//   emit      gated on head.ok and per position on its being in front of record n_done. The kept
//             words and mbcnt give the rank; the tile's rows are staged in LDS and stored as one
//             contiguous range, consecutive lanes consecutive rows (8-byte stores; the tags as
//             aligned dwords, bytes at both edges).
//   list      only when a record missed: one workgroup lists the stopping record's miss rows (the
//             image: every missing position) in order.
#include "nxg_device.h"
#include "nxg_replay.h"

namespace {

constexpr int RP_TILE = 512;     // positions per workgroup of the classify and emit kernels
constexpr int RP_LIST_NT = 1024; // threads of the list kernel
constexpr uint64_t RP_DROP = NXG_REPLAY_DROP, RP_MISS = NXG_REPLAY_MISS;
constexpr uint32_t kNone = 0, kKept = 1, kDrop = 2, kMiss = 3;
static_assert(RP_TILE % 64 == 0, "a tile is whole waves");

// the Id of position x
NXG_DEV uint64_t arch_id(const NxgRpArgs& A, uint64_t x) {
    return A.order ? (uint64_t)A.order[x] : A.id[A.first + x];
}

// the class of an Id that belongs to a record
NXG_DEV uint32_t class_of(const NxgRpArgs& A, uint64_t a, uint64_t* pub) {
    const uint64_t t = a < A.n_ids ? A.pub_id_of_arch[a] : RP_MISS;
    *pub = t;
    return t == RP_DROP ? kDrop : t == RP_MISS ? kMiss : kKept;
}

// the record of window row r, between the records lo <= hi of the tile's first and last row; false:
// r lies in front of that record's rows (it belongs to none)
NXG_DEV bool record_of(const NxgRpArgs& A, uint64_t r, uint64_t lo, uint64_t hi, uint64_t* rec) {
#pragma unroll 1
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (A.rend[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    *rec = lo;
    return lo < A.n_recs && A.rbeg[lo] <= r;
}

// n_done and the first position that is not emitted
NXG_DEV uint64_t done_of(const NxgRpArgs& A, uint64_t* lim) {
    const uint64_t inv = A.head->stop_inv;
    const uint64_t nd = (!A.order && inv) ? ~inv : (uint64_t)A.n_recs;
    *lim = nd < A.n_recs ? A.rbeg[nd] - A.first : A.n;
    return nd;
}

}  // namespace

__global__ __launch_bounds__(RP_TILE) void nxg_replay_classify_kernel(NxgRpArgs A, uint64_t nt) {
    constexpr int NWAVE = RP_TILE / 64;
    __shared__ uint64_t sh_c[2];
    __shared__ uint32_t sh_cnt[NWAVE];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t x0 = (uint64_t)blockIdx.x * RP_TILE, x = x0 + tid;
    const uint64_t x_end = x0 + RP_TILE < A.n ? x0 + RP_TILE : A.n;
    if (tid < 128) {  // the records of the tile's first and last row
        const uint64_t r = A.first + (tid < 64 ? x0 : x_end - 1);
        const uint64_t c = wave_lower_bound(A.rend, A.n_recs, r + 1);
        if (lane == 0) sh_c[w] = c;
    }
    __syncthreads();
    uint32_t cls = kNone;
    uint64_t rec = 0;
    if (x < A.n && record_of(A, A.first + x, sh_c[0], sh_c[1], &rec)) {
        uint64_t pub;
        cls = class_of(A, arch_id(A, x), &pub);
    }
    const uint64_t km = __ballot(cls == kKept), mm = __ballot(cls == kMiss);
    if (lane == 0) {
        A.kmask[(uint64_t)blockIdx.x * NWAVE + w] = km;
        sh_cnt[w] = (uint32_t)__popcll(km);
    }
    // records rise with the rows: the wave's first miss lane has its lowest record
    if (mm && lane == (uint32_t)__builtin_ctzll(mm))
        atomicMax((unsigned long long*)&A.head->stop_inv, (unsigned long long)~rec);
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < NWAVE; i++) t += sh_cnt[i];
        A.cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) A.cnt[nt] = 0;
    }
}

// boundary k <= n_recs: the kept rows in front of record min(k, n_done)
__global__ __launch_bounds__(256) void nxg_replay_bound_kernel(NxgRpArgs A) {
    constexpr int NWAVE = RP_TILE / 64;
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > A.n_recs) return;
    uint64_t lim;
    const uint64_t nd = done_of(A, &lim);
    const uint64_t x = k < nd ? A.rbeg[k] - A.first : lim;
    const uint64_t t = x / RP_TILE;
    const uint32_t full = (uint32_t)(x % RP_TILE) / 64, rem = (uint32_t)(x % 64);
    uint64_t c = A.off[t];
    for (uint32_t i = 0; i < full; i++) c += (uint64_t)__popcll(A.kmask[t * NWAVE + i]);
    if (rem) c += (uint64_t)__popcll(A.kmask[t * NWAVE + full] & ((1ull << rem) - 1));
    A.rec_off[k] = c;
    if (k == A.n_recs) {
        A.head->n_rows = c;
        A.head->n_done = nd;
        A.head->ok = c <= A.cap_rows;
    }
}

__global__ __launch_bounds__(RP_TILE) void nxg_replay_emit_kernel(NxgRpArgs A) {
    constexpr int NWAVE = RP_TILE / 64;
    __shared__ uint64_t s_id[RP_TILE], s_fixed[RP_TILE], s_src[RP_TILE];
    __shared__ uint32_t s_aux[RP_TILE];
    __shared__ __attribute__((aligned(4))) uint8_t s_tag[RP_TILE + 4];
    __shared__ uint32_t s_w[NWAVE];
    if (!A.head->ok) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t x0 = (uint64_t)blockIdx.x * RP_TILE, xw = x0 + 64ull * w, x = xw + lane;
    uint64_t lim;
    done_of(A, &lim);
    if (lim <= x0) return;
    // the wave's kept positions in front of the stop
    uint64_t km = A.kmask[(uint64_t)blockIdx.x * NWAVE + w];
    km &= lim <= xw ? 0ull : lim - xw >= 64 ? ~0ull : (1ull << (lim - xw)) - 1;
    const bool kept = (km >> lane) & 1;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
    if (lane == 0) s_w[w] = (uint32_t)__popcll(km);
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NWAVE; i++) {
        const uint32_t c = s_w[i];
        if ((uint32_t)i < w) wbase += c;
        tot += c;
    }
    if (tot == 0) return;
    const uint64_t base = A.off[blockIdx.x];  // the tile's rows are out[base, base + tot)
    const uint32_t phase = (uint32_t)(((uintptr_t)A.otag + base) & 3u);
    if (kept) {
        const uint64_t a = arch_id(A, x);
        uint64_t src = A.first + x;
        bool have = true;
        if (A.order) {  // the image's row of this Id
            uint64_t lo = 0, hi = A.n_img;
#pragma unroll 1
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (A.img_id[mid] < a) lo = mid + 1;
                else hi = mid;
            }
            have = lo < A.n_img && A.img_id[lo] == a;
            src = lo;
        }
        uint32_t tg = 16, ax = 0;  // Value::Null
        uint64_t fx = 0;
        if (have) {
            tg = A.tag[src];
            if (tg == NXG_TAG_UNSUBSCRIBED) {
                tg = 16;
                have = false;
            } else {
                fx = A.fixed[src];
                ax = A.aux[src];
            }
        }
        const uint32_t j = wbase + rank;
        s_id[j] = A.pub_id_of_arch[a];
        s_fixed[j] = fx;
        s_aux[j] = ax;
        s_tag[phase + j] = (uint8_t)tg;
        s_src[j] = (A.order && !have) ? ~0ull : src;
    }
    __syncthreads();
    for (uint32_t j = tid; j < tot; j += RP_TILE) {
        A.oid[base + j] = s_id[j];
        A.ofixed[base + j] = s_fixed[j];
        A.osrc[base + j] = s_src[j];
        A.oaux[base + j] = s_aux[j];
    }
    // tag block b is the 4 bytes at the aligned address otag + base - phase + 4 b
    uint8_t* const g0 = reinterpret_cast<uint8_t*>((uintptr_t)A.otag + base - phase);
    const uint32_t end = phase + tot, nblk = (end + 3) >> 2;
    for (uint32_t b = tid; b < nblk; b += RP_TILE) {
        if (4 * b >= phase && 4 * b + 4 <= end) {
            *reinterpret_cast<uint32_t*>(g0 + 4ull * b) = *reinterpret_cast<const uint32_t*>(s_tag + 4 * b);
        } else {
            for (uint32_t k = 4 * b; k < 4 * b + 4; k++)
                if (k >= phase && k < end) g0[k] = s_tag[k];
        }
    }
}

// the misses of record `rec`, in order (one workgroup)
__global__ __launch_bounds__(RP_LIST_NT) void nxg_replay_list_kernel(NxgRpArgs A, uint32_t rec) {
    __shared__ uint64_t tmp[RP_LIST_NT / 64];
    const uint64_t xb = A.rbeg[rec] - A.first, xe = A.rend[rec] - A.first;
    uint64_t n = 0;
#pragma unroll 1
    for (uint64_t x0 = xb; x0 < xe; x0 += RP_LIST_NT) {
        const uint64_t x = x0 + threadIdx.x;
        uint64_t pub;
        const bool miss = x < xe && class_of(A, arch_id(A, x), &pub) == kMiss;
        uint64_t tot;
        const uint64_t at = n + block_excl_scan<uint64_t, RP_LIST_NT>(miss ? 1 : 0, tmp, &tot);
        if (miss && at < A.cap_miss) A.miss_row[at] = A.first + x;
        n += tot;
    }
    if (threadIdx.x == 0) A.head->n_miss = n;
}

// ---- launch (host) ------------------------------------------------------------------------------
namespace {
uint64_t up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

uint64_t rp_layout(NxgRpArgs& a, uint8_t* p, uint64_t n, uint32_t n_recs) {
    const uint64_t nt = (n + RP_TILE - 1) / RP_TILE;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t* q = p ? p + o : nullptr;
        o += up256(bytes);
        return q;
    };
    a.head = reinterpret_cast<NxgRpHead*>(take(sizeof(NxgRpHead)));
    a.rbeg = reinterpret_cast<uint64_t*>(take(8 * ((uint64_t)n_recs + 1)));
    a.rend = reinterpret_cast<uint64_t*>(take(8 * (uint64_t)n_recs));
    a.cnt = reinterpret_cast<uint32_t*>(take(4 * (nt + 1)));
    a.off = reinterpret_cast<uint64_t*>(take(8 * (nt + 1)));
    a.bsum = reinterpret_cast<uint64_t*>(take(8 * ((nt + 1) / 4096 + 2)));
    a.kmask = reinterpret_cast<uint64_t*>(take(8 * nt * (RP_TILE / 64)));
    return o;
}
}  // namespace

uint64_t nxg_rp_scratch_bytes(uint64_t n, uint32_t n_recs) {
    NxgRpArgs a{};
    return rp_layout(a, nullptr, n, n_recs);
}

hipError_t nxg_launch_replay(NxgRpArgs a, uint8_t* scratch, const uint64_t* hbeg,
                             const uint64_t* hend, hipStream_t s) {
    const uint64_t n = a.n, nt = (n + RP_TILE - 1) / RP_TILE;
    if (n == 0 || a.n_recs == 0 || nt >= (1ull << 31)) return hipErrorInvalidValue;
    rp_layout(a, scratch, n, a.n_recs);
    hipError_t e = hipMemsetAsync(a.head, 0, sizeof(NxgRpHead), s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(a.rbeg, hbeg, 8 * ((uint64_t)a.n_recs + 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(a.rend, hend, 8 * (uint64_t)a.n_recs, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nxg_replay_classify_kernel, dim3((uint32_t)nt), dim3(RP_TILE), 0, s, a, nt);
    e = nxg_scan_u32(a.cnt, nt + 1, a.off, a.bsum, s);
    if (e != hipSuccess) return e;
    const uint64_t nk = ((uint64_t)a.n_recs + 1 + 255) / 256;
    hipLaunchKernelGGL(nxg_replay_bound_kernel, dim3((uint32_t)nk), dim3(256), 0, s, a);
    if (a.cap_rows)
        hipLaunchKernelGGL(nxg_replay_emit_kernel, dim3((uint32_t)nt), dim3(RP_TILE), 0, s, a);
    return hipGetLastError();
}

hipError_t nxg_launch_replay_misses(NxgRpArgs a, uint8_t* scratch, uint32_t rec, hipStream_t s) {
    rp_layout(a, scratch, a.n, a.n_recs);
    hipLaunchKernelGGL(nxg_replay_list_kernel, dim3(1), dim3(RP_LIST_NT), 0, s, a, rec);
    return hipGetLastError();
}
