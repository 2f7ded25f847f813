// nxg_path_hash.h -- the path table's hash, shared by the kernels of nxg_route_subscribes.hip
// (which read a path eight bytes at a time) and the host's nxg_path_hash (nxg_api_route.cpp).
//
// A path of len bytes is hashed over its little-endian 8-byte words w_0, w_1, ... (the last one
// zero above the path's end): h = kSeed ^ len; h = mix(h, w_i) for each word; finish_hash(h).
// Stored hash words 0 and 1 mean "empty" and "tombstone", so finish_hash moves a raw 0 or 1 to 2
// and 3. Every step is a bijection of the 64-bit state for a given word (tests/path_table_cases.py
// inverts them to build paths with chosen hashes).
#pragma once
#include <stdint.h>

#define NXG_HD __host__ __device__ __forceinline__

namespace nxgpath {

constexpr uint64_t kSeed = 0x243F6A8885A308D3ull;

NXG_HD uint64_t mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
NXG_HD uint64_t finish_hash(uint64_t h) {
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 29;
    return h < 2 ? h + 2 : h;  // 0 and 1 mark empty slots and tombstones
}

}  // namespace nxgpath
