// nxg_replay.h -- nxg_replay_window / nxg_replay_image: what their kernels (nxg_replay.hip) and
// the host calls (nxg_api_archive.cpp) share. Not ABI.
#pragma once
#include "nxg_internal.h"

struct NxgRpHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t stop_inv;  // ~record of the lowest record that holds a miss (atomicMax; 0: none)
    uint64_t n_rows;    // the bound kernel: kept rows of records [0, n_done)
    uint64_t n_done;    // the bound kernel
    uint64_t n_miss;    // the list kernel
    uint32_t ok;        // the bound kernel: n_rows <= cap_rows, the emit kernel writes
    uint32_t pad0;
    uint64_t pad[3];
};
static_assert(sizeof(NxgRpHead) == 64, "NxgRpHead layout");
struct NxgRpArgs {
    // the source. Window: position x is window row first + x, Id id[first + x], value tag / fixed /
    // aux of that row. Image (order != null, first = 0): position x is order[x], its value the
    // image row found by bisection over img_id[0 .. n_img) (ascending), tag / fixed / aux the image's.
    const uint64_t* id;
    const uint32_t* order;
    const uint64_t* img_id;
    uint64_t n_img;
    const uint8_t* tag;
    const uint64_t* fixed;
    const uint32_t* aux;
    uint64_t first, n;  // positions [0, n)
    uint32_t n_recs;    // image: 1
    const uint64_t* pub_id_of_arch;
    uint64_t n_ids;
    // the caller's outputs
    uint64_t cap_rows;
    uint64_t* oid;
    uint8_t* otag;
    uint64_t* ofixed;
    uint32_t* oaux;
    uint64_t* osrc;
    uint64_t* rec_off;
    uint64_t* miss_row;
    uint64_t cap_miss;
    // scratch, placed by the launcher
    NxgRpHead* head;
    uint64_t* rbeg;   // [n_recs + 1] record c's rows are [rbeg[c], rend[c]) (window rows); the
    uint64_t* rend;   // [n_recs]     last rbeg is first + n. Uploaded by the host.
    uint32_t* cnt;    // [tiles + 1] kept positions per tile (the last: 0)
    uint64_t* off;    // [tiles + 1] their exclusive sums
    uint64_t* bsum;   // nxg_scan_u32's
    uint64_t* kmask;  // per 64 positions: the kept ones
};
// `scratch` holds nxg_rp_scratch_bytes(n, n_recs) bytes. The launcher places the arrays, zeroes the
// head (at the start of scratch) and copies hbeg[0 .. n_recs] / hend[0 .. n_recs) up; n > 0.
uint64_t nxg_rp_scratch_bytes(uint64_t n, uint32_t n_recs);
hipError_t nxg_launch_replay(NxgRpArgs a, uint8_t* scratch, const uint64_t* hbeg,
                             const uint64_t* hend, hipStream_t s);
// the second, rare launch: the misses of record `rec` (image: of every position) listed in order
hipError_t nxg_launch_replay_misses(NxgRpArgs a, uint8_t* scratch, uint32_t rec, hipStream_t s);
