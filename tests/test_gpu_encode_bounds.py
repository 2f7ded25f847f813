"""Encoders at any offset of their output and at short buffers: include/nxg_codec.h promises that
an encode writes nothing outside [out, out + cap), whether it succeeds or fails.

Every encode here goes into a guarded buffer (tests/guards.py: 4096 sentinel bytes on both sides,
the output at any 16-byte phase `off`); the bytes written equal the oracle's or the twin's frame,
and no byte outside changed.

  general encoder (nxg_encode_general.hip), a tile is 1024 rows, staged in LDS at 28 bytes per
  row and written out as aligned 16-byte stores plus byte stores for the two edge blocks; a tile
  with control spans, with more bytes than the staging or past `cap` writes row by row:
    Update frames   1 .. 3000 short mixed rows; a 40000-byte value between staged tiles;
                    Heartbeats and a control span after the last row (ctl_write)
    archive batch   1, 200 and 20000 rows: the count's varint of 1, 2, 3 bytes shifts every tile
    To::Write       with and without control spans
  tiled f64 encoder (NXG_F64_ENC=tile, nxg_encode_f64.hip), 2048 records a tile, staged at 15
  bytes a record: ids >= 2^28 make records of 16 bytes and more, which leave the staging; mixed
  ids tile by tile: a staged tile filled to its last byte, a row-by-row one, a staged one
The frames are built in tests/encode_bounds_cases.py; tests/test_encode_bounds_cpu.py checks on
the oracle alone that each reaches the path named here.
  short buffers     every mode at a staged and at a row-by-row shape: cap = len succeeds, cap =
                    len - 1 and len // 2 fail ("too small"); bytes inside [out, out + cap) may be
                    anything then, bytes outside are untouched
  persistent grid   NXG_PERSISTENT=1: every workgroup loops over tiles and reuses its staging;
                    batches of more tiles than the grid can have workgroups
"""
import os

import numpy as np
import pytest

import encode_bounds_cases as ebc
import nxo
from encode_bounds_cases import (archive_ref, f64_ids, heartbeats_wire, long_text_archive,
                                 mixed_rows_wire, past_the_staging_wire, writes_wire)
from guards import assert_outside_untouched, guarded_buffer, out_ptr, written

pytestmark = pytest.mark.gpu


def _codec(**env):
    """A context made with `env` set (read at creation); the environment is as before after."""
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return netidx_amd.Codec(0)
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def codec():
    c = _codec()
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile_codec():
    c = _codec(NXG_F64_ENC="tile")
    yield c
    c.close()


def dev(b):
    import torch
    a = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
    return torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).cuda()


def check_encode(encode, ref, off, cap=None):
    """encode(buf, off, cap) -> length writes at byte margin + off of the guarded `buf`. cap >=
    len(ref): the bytes are `ref`; below: it fails with "too small". Either way nothing outside
    [out, out + min(cap, len)) changed."""
    from netidx_amd import CodecError
    ref = np.frombuffer(bytes(ref), np.uint8) if not isinstance(ref, np.ndarray) else ref
    n = len(ref)
    cap = n if cap is None else cap
    buf = guarded_buffer(n, off)
    if cap >= n:
        assert encode(buf, off, cap) == n
        got = written(buf, off, n)
        diff = np.flatnonzero(got != ref)
        assert len(diff) == 0, f"off={off}: {len(diff)} bytes differ, the first at {int(diff[0])}"
        assert_outside_untouched(buf, off, n)
    else:
        with pytest.raises(CodecError, match="too small"):
            encode(buf, off, cap)
        assert_outside_untouched(buf, off, cap)


def short_caps(n):
    return (n, n - 1, n // 2)


# ---- general encoder: Update frames -----------------------------------------------------------
def update_job(codec, wire):
    """An Update frame's columns (the oracle's decode of it) on the device, heap = the frame."""
    import netidx_amd
    o = nxo.decode(wire).trim()
    assert o["err_kind"] == 0
    cols = netidx_amd.columns_from_arrays(
        o["id"], o["fixed"], o["tag"], o["aux"], o["ctag"], o["cfixed"], o["caux"], o["ctl_row"],
        o["ctl_off"], o["ctl_len"], o["ctl_variant"])
    heap = dev(wire)
    assert codec.encoded_len(cols, heap) == len(wire)
    return lambda buf, off, cap: codec.encode_into(cols, heap, out_ptr(buf, off), cap)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3000])
def test_update_rows_at_every_phase(codec, n):
    wire = mixed_rows_wire(n)
    enc = update_job(codec, wire)
    for off in ((0, 1, 7, 8, 15) if n == 3000 else (0, 9)):
        check_encode(enc, wire, off)


def test_update_tiles_past_the_staging(codec):
    wire = past_the_staging_wire()
    enc = update_job(codec, wire)
    for off in (0, 5):
        check_encode(enc, wire, off)


def test_update_heartbeats_and_a_last_control_span(codec):
    wire = heartbeats_wire()
    assert nxo.decode(wire).s.n_ctl > 50
    enc = update_job(codec, wire)
    for off in (0, 11):
        check_encode(enc, wire, off)


# ---- general encoder: archive batches ---------------------------------------------------------
def archive_job(codec, m):
    import netidx_amd
    cols = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
    heap = dev(m.heap)

    def enc(buf, off, cap):
        lo = buf.guard_margin + off
        return codec.encode_archive(cols, heap, out=buf[lo: lo + cap])
    return enc


@pytest.mark.parametrize("n", [1, 200, 20000])
def test_archive_rows_at_every_phase(codec, n):
    from netidx_amd import synth
    m = synth.archive_columns(n, seed=600 + n)
    ref = archive_ref(m)
    assert ref[0] == (n if n < 128 else (n & 0x7F) | 0x80)
    enc = archive_job(codec, m)
    for off in (0, 3, 15):
        check_encode(enc, ref, off)


# ---- general encoder: To::Write frames --------------------------------------------------------
def writes_job(codec, wire, e):
    from test_gpu_writes import encode_from
    cols, wc, heap = encode_from(codec, e, wire)
    assert codec.encoded_writes_len(cols, wc, heap) == len(wire)
    return lambda buf, off, cap: codec.encode_writes_into(cols, wc, heap, out_ptr(buf, off), cap)


@pytest.mark.parametrize("ctl", [False, True], ids=["rows_only", "control_spans"])
@pytest.mark.parametrize("n", [1, 1024, 1025, 2600])
def test_writes_at_two_phases(codec, n, ctl):
    wire, e = writes_wire(n, ctl)
    assert len(e.rows) == n and bool(e.ctl) == ctl
    enc = writes_job(codec, wire, e)
    for off in (0, 6):
        check_encode(enc, wire, off)


# ---- tiled f64 encoder ------------------------------------------------------------------------
def f64_job(codec, ids, vals):
    import netidx_amd
    cols = netidx_amd.columns_from_arrays(ids, vals)
    return lambda buf, off, cap: codec.encode_into(cols, None, out_ptr(buf, off), cap)


@pytest.mark.parametrize("wide", [True, False], ids=["ids_past_2_28", "ids_mixed"])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 5000])
def test_tiled_f64_at_every_phase(tile_codec, n, wide):
    from netidx_amd import synth
    ids = f64_ids(n, wide, 800 + n)
    vals = synth.f64_columns(n, 801 + n)[1]
    ref = nxo.encode_f64(ids, vals)
    enc = f64_job(tile_codec, ids, vals)
    for off in (0, 1, 15):
        check_encode(enc, ref, off)
        assert tile_codec.last_encode_kernel() == "tile"


# ---- short buffers ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["staged", "row_by_row"])
def test_update_short_buffer(codec, shape):
    wire = mixed_rows_wire(3000) if shape == "staged" else heartbeats_wire()
    enc = update_job(codec, wire)
    for cap in short_caps(len(wire)):
        check_encode(enc, wire, 5, cap)


@pytest.mark.parametrize("shape", ["staged", "row_by_row"])
def test_archive_short_buffer(codec, shape):
    from netidx_amd import synth
    m = synth.archive_columns(3000, seed=61) if shape == "staged" else long_text_archive(3000)
    ref = archive_ref(m)
    if shape == "row_by_row":
        assert len(ref) > 3000 * 40  # past 28 bytes a row
    enc = archive_job(codec, m)
    for cap in short_caps(len(ref)):
        check_encode(enc, ref, 5, cap)


@pytest.mark.parametrize("shape", ["staged", "row_by_row"])
def test_writes_short_buffer(codec, shape):
    wire, e = writes_wire(2600, shape == "row_by_row")
    enc = writes_job(codec, wire, e)
    for cap in short_caps(len(wire)):
        check_encode(enc, wire, 5, cap)


@pytest.mark.parametrize("shape", ["staged", "row_by_row"])
def test_tiled_f64_short_buffer(tile_codec, shape):
    from netidx_amd import synth
    n = 5000
    rng = np.random.default_rng(62)
    ids = rng.integers(0, 2**21, n, dtype=np.uint64) if shape == "staged" else f64_ids(n, True, 63)
    vals = synth.f64_columns(n, 64)[1]
    ref = nxo.encode_f64(ids, vals)
    enc = f64_job(tile_codec, ids, vals)
    for cap in short_caps(len(ref)):
        check_encode(enc, ref, 5, cap)


# ---- persistent grid --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def persistent_codec():
    c = _codec(NXG_PERSISTENT="1", NXG_F64_ENC="tile")
    yield c
    c.close()


LDS_PER_CU = 160 * 1024


def assert_more_tiles_than_workgroups(tiles, staging):
    """The persistent grid is CUs * (workgroups per CU - 1) (nxg_ctx.cpp). A workgroup's LDS is
    more than its staging, so LDS alone bounds the workgroups per CU, whatever the occupancy
    query answers: with fewer workgroups than tiles some of them loop and reuse their staging.
    How many take a second tile is not known here (MI355X, 256 CUs: at most 1024 workgroups for
    the 1465 f64 tiles, at most 1024 for the 1954 mixed ones), only that some must."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_cu = LDS_PER_CU // staging
    assert per_cu > 2 and cus * (per_cu - 1) < tiles, (cus, per_cu, tiles)


def test_persistent_grid_f64(persistent_codec):
    """3 * 10^6 ids in random order: 1465 tiles of 2048 records for a grid of fewer workgroups,
    so that workgroups take a second tile into the staging they used for their first."""
    from netidx_amd import synth
    n = 3_000_000
    assert_more_tiles_than_workgroups(-(-n // ebc.F64_TILE), 15 * ebc.F64_TILE + 32)
    ids, vals = synth.f64_columns(n, 900)
    ids = np.random.default_rng(901).permutation(ids)
    check_encode(f64_job(persistent_codec, ids, vals), nxo.encode_f64(ids, vals), 7)
    assert persistent_codec.last_encode_kernel() == "tile"


def test_persistent_grid_mixed(persistent_codec):
    """2 * 10^6 mixed rows: 1954 tiles of 1024 rows, more than the grid has workgroups."""
    import netidx_amd
    from test_gpu_parity import mixed_wire
    assert_more_tiles_than_workgroups(-(-2_000_000 // ebc.GEN_TILE), ebc.GEN_STAGED + 32)
    m, wire = mixed_wire(2_000_000, 902)
    cols = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
    heap = dev(m.heap)
    codec = persistent_codec
    check_encode(lambda buf, off, cap: codec.encode_into(cols, heap, out_ptr(buf, off), cap),
                 wire, 7)
