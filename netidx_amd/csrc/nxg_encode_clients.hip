// nxg_encode_clients.hip -- a commit's per-client batches in one encode (nxg_encode_clients).
//
// UpdateBatch::commit (publisher/mod.rs:776-845) leaves client c the entries
// [chan_off[c], chan_off[c+1]) of (Id, row), sorted by client and in batch order within one. The
// concatenation of every client's payload, in client order, is therefore the encode of the entry
// list taken as one stream of From::Update(id[row], value[row]) messages, and client c's payload
// starts at the byte offset of entry chan_off[c]. So the call is one launch of a tile encoder
// that reads its rows through ent_row: nxg_enc_f64_gather_kernel (nxg_encode_f64.hip) for F64
// columns, nxg_enc_rows_gather_kernel (nxg_encode_general.hip) for mixed ones. Each tile finds
// the clients that start in it (wave_lower_bound over chan_off, then a walk) and stores their
// offsets once the look-back has given its base (store_client_offs, nxg_device.h): no per-entry
// offset array is written.
#include "nxg_device.h"

uint64_t nxg_enc_clients_tiles(bool f64, uint64_t n_ent) {
    return f64 ? nxg_enc_f64_gather_tiles(n_ent) : nxg_enc_rows_gather_tiles(n_ent);
}

hipError_t nxg_launch_enc_clients(bool f64, const ColsDesc& cols, const uint8_t* heap,
                                  const NxgGather& g, uint8_t* out, uint64_t cap, uint64_t* tstat,
                                  uint32_t epoch, DevStatus* st, int grid_f64, int grid_gen,
                                  hipStream_t s) {
    if (f64)
        return nxg_launch_enc_f64_gather(cols.id, cols.fixed, cols.n_rows, g, out, cap, tstat,
                                         epoch, st, grid_f64, s);
    return nxg_launch_enc_rows_gather(cols, heap, g, out, cap, tstat, epoch, st, grid_gen, s);
}
