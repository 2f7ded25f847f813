// nxg_oneshot.h -- the oneshot calls (nxg_oneshot_pack_pathmap, nxg_oneshot_pack_deltas): what
// their kernels (nxg_oneshot.hip) and the host calls (nxg_api_oneshot.cpp) share. Not ABI.
#pragma once
#include "nxg_internal.h"

// HashMap<Id, Path>::encode's guard (pack.rs:1115): len * (size_of::<Id>() + size_of::<Path>()),
// 4 + 8 (Path is one ArcStr, one pointer)
constexpr uint64_t kOsPathmapEntrySize = 12;

// ---- the pathmap section ------------------------------------------------------------------------
struct NxgOsPmHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t bad_inv;  // ~a of the lowest Id a with path_off[a + 1] < path_off[a] (atomicMax; 0: none)
    uint64_t n_sel, item_bytes;  // selected Ids and their items' bytes (the plan kernel)
    uint64_t n_bytes;  // the section: varint(n_sel) and the items
    uint32_t vec_bad;  // n_sel * 12 exceeds MAX_VEC
    uint32_t ok;       // nothing refused, the section fits and there is an `out`: the emit kernel writes
    uint64_t pad[11];
};
static_assert(sizeof(NxgOsPmHead) == 128, "NxgOsPmHead layout");
struct NxgOsPmArgs {
    const uint64_t* path_off;  // [n_ids + 1]
    const uint8_t* path_bytes;
    const uint8_t* keep;  // [n_ids]
    uint64_t n_ids;       // > 0
    uint8_t* sel;         // [n_ids]
    uint8_t* out;         // null: size only
    uint64_t cap;
    // scratch, placed by the launcher
    NxgOsPmHead* head;
    uint64_t* bcnt;    // per block of Ids: selected Ids, then (top kernel) those before it in its
    uint64_t* bbytes;  // group of blocks; likewise the items' bytes
    uint64_t* gcnt;    // per group of blocks: the same, then (plan kernel) those before the group
    uint64_t* gbytes;
};
// `scratch` holds nxg_os_pm_scratch_bytes(n_ids) bytes; only the head (at its start) is
// initialised, by the launcher. a.head is at `scratch` afterwards.
uint64_t nxg_os_pm_scratch_bytes(uint64_t n_ids);
hipError_t nxg_launch_os_pathmap(NxgOsPmArgs a, uint8_t* scratch, hipStream_t s);

// ---- the deltas elements of one window ----------------------------------------------------------
struct NxgOsDlHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t err_inv;  // ~row << 8 | cause (nxg_record.h) of the lowest refused window row (atomicMax; 0: none)
    uint64_t n_items, item_bytes;   // kept rows and their items' bytes (the top kernels)
    uint64_t n_bytes, n_kept_recs;  // the plan kernel
    uint32_t vec_bad;  // 1 + the first record whose items exceed MAX_VEC (0: none)
    uint32_t ok;       // nothing refused, the elements fit and there is an `out`: the emit kernel writes
    uint64_t pad[10];
};
static_assert(sizeof(NxgOsDlHead) == 128, "NxgOsDlHead layout");
struct NxgOsDlArgs {
    ColsDesc cols;  // the window (MIXED layout)
    const uint8_t* heap;
    const uint8_t* sel;  // [n_ids]
    uint64_t n_ids;
    uint64_t first, n;  // the records lie in window rows [first, first + n); entry e is row first + e
    uint32_t n_recs;
    uint8_t* out;  // null: size only
    uint64_t cap;
    uint64_t* rec_off;
    uint64_t* rec_items;
    // scratch, placed by the launcher
    NxgOsDlHead* head;
    uint64_t* rbeg;    // [n_recs + 1] record k's first entry; rbeg[n_recs] == n
    uint64_t* rend;    // [n_recs] the entry behind record k's last (<= rbeg[k + 1])
    uint64_t* secs;    // [n_recs] the timestamps
    uint64_t* nanos;
    uint32_t* len;     // per entry: its item's bytes (0: not kept)
    uint64_t* bcnt;    // per block of entries: kept entries, then (top kernel) those before it in
    uint64_t* bbytes;  // its group of blocks; likewise the items' bytes
    uint64_t* gcnt;    // per group of blocks: the same, then those before the group
    uint64_t* gbytes;
    uint64_t* ccnt;    // [n_recs + 1] kept entries / item bytes in front of entry rbeg[k]
    uint64_t* cbytes;
    uint64_t* cinfo;   // [2 * n_recs]: ccnt[k], and lead bytes of records 0..k | record k's lead << 56
};
uint64_t nxg_os_dl_scratch_bytes(uint64_t n, uint32_t n_recs);
hipError_t nxg_launch_os_deltas(NxgOsDlArgs a, uint8_t* scratch, const uint64_t* up, hipStream_t s);
