// nxg_record.h -- nxg_record_entries: what its kernels (nxg_record.hip) and the host call
// (nxg_api_archive.cpp) share. Not ABI.
#pragma once
#include "nxg_internal.h"

// causes of a refused entry (the low byte of NxgRecHead.err_inv)
enum : uint32_t {
    kRecRow = 1, kRecTag = 2, kRecBig = 3, kRecKids = 4, kRecNoKids = 5, kRecDepth = 6
};
struct NxgRecHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t err_inv;  // ~entry << 8 | cause of the lowest refused entry (atomicMax; 0: none)
    uint64_t n_items, item_bytes;  // kept entries and their items' bytes (the top kernels)
    uint64_t n_bytes, n_dropped;   // the plan kernel
    uint32_t chan_bad;  // 1 + the lowest channel at which chan_off is not a dispatch's (0: none)
    uint32_t vec_bad;   // 1 + the first channel whose items exceed MAX_VEC (0: none)
    uint32_t ok;        // nothing refused, the records fit and there is an `out`: the emit kernel writes
    uint32_t pad0;
    uint64_t pad[9];
};
static_assert(sizeof(NxgRecHead) == 128, "NxgRecHead layout");
struct NxgRecArgs {
    ColsDesc cols;  // the batch (tag null: F64 layout)
    const uint8_t* heap;
    const uint64_t* ent_sub;
    const uint64_t* ent_row;
    const uint64_t* chan_off;  // [n_chans + 1]
    uint64_t n_ent;
    uint32_t n_chans;
    const uint32_t* arch_id_of_sub;
    uint64_t n_subs;
    uint8_t* out;  // null: size only
    uint64_t cap;
    uint64_t* rec_off;
    uint64_t* rec_items;
    // scratch, placed by the launcher
    NxgRecHead* head;
    uint32_t* len;     // per entry: its item's bytes (0: not kept)
    uint64_t* bcnt;    // per block of entries: kept entries, then (top kernels) those before it in
    uint64_t* bbytes;  // its group of blocks; likewise the items' bytes
    uint64_t* gcnt;    // per group of blocks: the same, then those before the group
    uint64_t* gbytes;
    uint64_t* ccnt;    // [n_chans + 1] kept entries / item bytes in front of entry chan_off[c]
    uint64_t* cbytes;
    uint64_t* cinfo;   // [2 * n_chans]: ccnt[c], and count-varint bytes of channels 0..c | width << 60
};
// `scratch` holds nxg_rec_scratch_bytes(n_ent, n_chans) bytes; only the head (at its start) is
// initialised, by the launcher. a.head is at `scratch` afterwards.
uint64_t nxg_rec_scratch_bytes(uint64_t n_ent, uint32_t n_chans);
hipError_t nxg_launch_record(NxgRecArgs a, uint8_t* scratch, hipStream_t s);
