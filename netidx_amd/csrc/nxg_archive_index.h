// nxg_archive_index.h -- nxg_archive_index_records and nxg_archive_scan_index: what their kernels
// (nxg_archive_index.hip) and the host calls (nxg_api_archive.cpp) share. Not ABI.
#pragma once
#include "nxg_internal.h"

// ---- the writer's index -----------------------------------------------------------------------
constexpr uint64_t kAixMaxVecIds = kMaxVecBytes / 4;  // Vec<Id>::encode's guard: count * 4 <= MAX_VEC
constexpr uint64_t kAixMaxKeys = 1ull << 28;          // positions of one call (a 6 GiB table)
struct NxgAixHead {  // device, zeroed per call, copied back whole after the last launch
    uint64_t wide_inv;  // ~p of the lowest position whose Id is >= 2^32 (atomicMax; 0: none)
    uint64_t n_ids, id_bytes;  // distinct (record, Id) pairs and their varints' bytes (the top kernels)
    uint64_t n_bytes;          // the plan kernel
    uint32_t seg_bad;  // 1 + the lowest record at which seg_off decreases or leaves the keys (0: none)
    uint32_t vec_bad;  // 1 + the first record whose Ids exceed MAX_VEC (0: none)
    uint32_t ok;       // nothing refused, the indexes fit and there is an `out`: the emit kernel writes
    uint32_t pad0;
    uint64_t pad[10];
};
static_assert(sizeof(NxgAixHead) == 128, "NxgAixHead layout");
struct NxgAixArgs {
    const uint64_t* key;      // [n_keys]
    const uint64_t* seg_off;  // [n_recs + 1]
    uint64_t n_keys;
    uint32_t n_recs;
    uint32_t translate;  // key is a SubId (else the Id itself)
    const uint32_t* arch_id_of_sub;
    uint64_t n_subs;
    uint8_t* out;  // null: size only
    uint64_t cap;
    uint64_t* idx_off;
    uint64_t* idx_ids;
    // the table (the ctx's own buffer): keys then minima, all bytes 0xFF before the claim pass
    unsigned long long* tkey;  // [slots] record << 32 | Id
    uint32_t* tmin;            // [slots] the lowest position that holds the key
    uint32_t slot_bits;        // slots = 1 << slot_bits
    // scratch, placed by the launcher
    NxgAixHead* head;
    uint32_t* rec;     // per position: its record
    uint32_t* slot;    // per position: its key's slot (kAixNoSlot: not kept)
    uint8_t* len;      // per position: vl(Id) when it is its key's first occurrence, else 0
    uint64_t* bcnt;    // per block of positions: firsts, then (top kernels) those before it in its
    uint64_t* bbytes;  // group of blocks; likewise their varints' bytes
    uint64_t* gcnt;    // per group of blocks: the same, then those before the group
    uint64_t* gbytes;
    uint64_t* ccnt;    // [n_recs + 1] firsts / varint bytes in front of position seg_off[c]
    uint64_t* cbytes;
    uint64_t* cinfo;   // [3 * n_recs]: ccnt[c]; lead bytes of records 0..c | width << 60; L
};
constexpr uint32_t kAixNoSlot = 0xFFFFFFFFu;
// slots of the table for n_keys positions (a power of two >= 2 * n_keys), and its bytes
uint32_t nxg_aix_slot_bits(uint64_t n_keys);
uint64_t nxg_aix_table_bytes(uint32_t slot_bits);
// `scratch` holds nxg_aix_scratch_bytes(n_keys, n_recs) bytes; only the head (at its start) is
// initialised, by the launcher, which also clears `table` (nxg_aix_table_bytes(a.slot_bits) bytes)
// with one hipMemsetAsync. a.head is at `scratch` afterwards. n_keys > 0.
uint64_t nxg_aix_scratch_bytes(uint64_t n_keys, uint32_t n_recs);
hipError_t nxg_launch_aix_index(NxgAixArgs a, uint8_t* scratch, uint8_t* table, hipStream_t s);

// ---- the reader's scan ------------------------------------------------------------------------
// Record i's result word: ~0 (nothing found), or (the byte's offset from idx_off[i]) << 2 | code of
// the lowest varint that hit (NXG_INDEX_MATCH) or failed (NXG_INDEX_ERR_*), by atomicMin.
// The staging the host uploads in one copy, all arrays of u64: off[n], end[n], pbase[n + 1] (the
// pieces in front of record i), res[n] (all ones).
uint64_t nxg_aix_scan_pieces(uintptr_t dbuf, uint64_t off, uint64_t end);  // an upper bound
hipError_t nxg_launch_aix_scan(const uint8_t* dbuf, const uint64_t* off, const uint64_t* end,
                               const uint64_t* pbase, uint32_t n, uint64_t n_pieces,
                               const uint8_t* keep, uint64_t n_ids, unsigned long long* res,
                               hipStream_t s);
