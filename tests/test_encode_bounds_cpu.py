"""The frames of the encoder bounds tests (tests/encode_bounds_cases.py), checked on the oracle
alone: whether a tile is staged or written row by row rests on its byte count, so the counts are
pinned here, on each side of the kernels' thresholds, for every frame that
tests/test_gpu_encode_bounds.py names as staged or as row by row."""
import numpy as np

import encode_bounds_cases as ebc
import nxo

UPDATE_N = (1, 2, 1023, 1024, 1025, 3000)
ARCHIVE_N = (1, 200, 20000)
WRITES_N = (1, 1024, 1025, 2600)
F64_N = (1, 2047, 2048, 2049, 5000)


def _row_tiles(wire, n):
    lens = ebc.message_lengths(wire)
    assert len(lens) == n
    return ebc.tile_sums(lens, ebc.GEN_TILE)


def test_general_encoder_frames_reach_their_paths():
    # Update rows: no control span, every tile within the staging
    for n in UPDATE_N:
        w = ebc.mixed_rows_wire(n)
        assert nxo.decode(w).s.n_ctl == 0
        tiles = _row_tiles(w, n)
        assert len(tiles) == -(-n // ebc.GEN_TILE) and max(tiles) <= ebc.GEN_STAGED, (n, tiles)
    # a 40000-byte value in tiles 0, 1, 2 and 4: row by row, then staged, then row by row
    w = ebc.past_the_staging_wire()
    assert nxo.decode(w).s.n_ctl == 0
    past = [t > ebc.GEN_STAGED for t in _row_tiles(w, 5000)]
    assert past == [True, True, True, False, True]
    # control spans: every tile row by row, one span behind the last row
    o = nxo.decode(ebc.heartbeats_wire()).trim()
    assert len(o["id"]) == 2500 and len(o["ctl_row"]) > 50 and o["ctl_row"][-1] == 2500
    assert o["n_heartbeat"] >= 50


def test_archive_batches_reach_their_paths():
    from netidx_amd import synth
    for n, seed in [(n, 600 + n) for n in ARCHIVE_N] + [(3000, 61)]:
        m = synth.archive_columns(n, seed=seed)
        tiles = ebc.archive_tile_bytes(m)
        assert len(tiles) == -(-n // ebc.GEN_TILE) and max(tiles) <= ebc.GEN_STAGED, (n, tiles)
        assert sum(tiles) + ebc.varint_len(n) == len(ebc.archive_ref(m))
    assert [ebc.varint_len(n) for n in ARCHIVE_N] == [1, 2, 3]
    tiles = ebc.archive_tile_bytes(ebc.long_text_archive(3000))
    assert len(tiles) == 3 and min(tiles) > ebc.GEN_STAGED, tiles


def test_write_frames_reach_their_paths():
    for n in WRITES_N:
        w, e = ebc.writes_wire(n, False)
        assert len(e.rows) == n and not e.ctl
        tiles = _row_tiles(w, n)
        assert max(tiles) <= ebc.GEN_STAGED, (n, tiles)
        w, e = ebc.writes_wire(n, True)
        assert len(e.rows) == n and len(e.ctl) >= 2
        assert e.ctl[-1][0] == n  # a control span behind the last row


def test_tiled_f64_batches_reach_their_paths():
    assert 16 * ebc.F64_EDGE_WIDE + 14 * (ebc.F64_TILE - ebc.F64_EDGE_WIDE) == ebc.F64_STAGED
    for n in F64_N:
        # ids >= 2^28: the tiles of 2047 and 2048 records (16 * 2047 > F64_STAGED) are past the
        # staging; the last tiles of 1, 1 and 904 records (21 * 904 < F64_STAGED) are staged
        t = ebc.f64_tile_paths(ebc.f64_ids(n, True, 800 + n))
        want = [min(ebc.F64_TILE, n - i * ebc.F64_TILE) >= 2047 for i in range(len(t))]
        assert [p for _, p in t] == want and want[0] == (n > 1), (n, t)
    mixed = {n: ebc.f64_tile_paths(ebc.f64_ids(n, False, 800 + n)) for n in F64_N}
    assert mixed[1] == [(16, False)]
    assert mixed[2047] == [(ebc.F64_STAGED - 14, False)]
    assert mixed[2048] == [(ebc.F64_STAGED, False)]  # the staging filled to its last byte
    assert mixed[2049] == [(ebc.F64_STAGED, False), (13, False)]
    # staged, row by row (from phase 0), staged (from phase 13)
    assert mixed[5000] == [(ebc.F64_STAGED, False), (13 + 16 * 2047, True), (16 * 904, False)]
    assert 13 + 16 * 2047 > ebc.F64_STAGED and (ebc.F64_STAGED + 13 + 16 * 2047) % 16 == 13
    # the short-buffer shapes
    ids = np.random.default_rng(62).integers(0, 2**21, 5000, dtype=np.uint64)
    assert [p for _, p in ebc.f64_tile_paths(ids)] == [False, False, False]
    assert [p for _, p in ebc.f64_tile_paths(ebc.f64_ids(5000, True, 63))] == [True, True, False]
