"""The frames of the encoder bounds tests (tests/test_gpu_encode_bounds.py) and how many bytes
each tile of theirs comes to, so that tests/test_encode_bounds_cpu.py can check on the oracle
alone that every frame reaches the path it is for.

  general encoder (nxg_encode_general.hip): a tile is GEN_TILE rows; it is staged in LDS when the
  frame has no control spans and the tile's bytes are at most GEN_STAGED, else written row by row.
  tiled f64 encoder (nxg_encode_f64.hip): a tile is F64_TILE records; it leaves the staging for
  put_rec_global when (its offset in the frame & 15) + its bytes exceed F64_STAGED.
"""
import random

import numpy as np

import nxo
import to_twin as tw
from frames import golden_twin

GEN_TILE = 1024
GEN_STAGED = 28 * GEN_TILE          # GSTG - 32, NXG_ENC_BPR = 28
F64_TILE = 2048
F64_STAGED = 15 * F64_TILE + 16     # MAXB_ALL - 16, NXG_ENC_STGB = 15
F64_EDGE_WIDE = 1032                # 16 * 1032 + 14 * (2048 - 1032) == F64_STAGED


# ---- Update frames ----------------------------------------------------------------------------
def mixed_rows_wire(n):
    from test_gpu_parity import mixed_wire
    return mixed_wire(n, 500 + n)[1]


def past_the_staging_wire():
    """The frame of test_gpu_parity.test_encode_tiles_past_the_staging: a 40000-byte value in
    some tiles (those write their rows straight to the frame), staged tiles around them."""
    mg = golden_twin()
    rng = random.Random(8)
    msgs = []
    for i in range(5000):
        if i % 1500 == 7:
            msgs.append(("u", i, (13, bytes(rng.getrandbits(8) for _ in range(40000)))))
        elif i % 3 == 0:
            msgs.append(("u", i, (12, b"x" * rng.randrange(0, 33))))
        else:
            msgs.append(("u", i, (9, rng.getrandbits(64))))
    return mg.batch(msgs)[0]


def heartbeats_wire():
    """Heartbeats between the rows of three tiles and a control span after the last row."""
    mg = golden_twin()
    rng = random.Random(9)
    msgs = []
    for i in range(2500):
        if rng.random() < 0.03:
            msgs.append(("hb",))
        v = (12, b"y" * rng.randrange(0, 25)) if i % 4 == 0 else (9, rng.getrandbits(64))
        msgs.append(("u", rng.getrandbits(rng.choice([7, 14, 30])), v))
    msgs.append(("hb",))
    msgs.append(("raw", 2, mg.enc_varint(77)))  # Unsubscribed(77), the last message
    return mg.batch(msgs)[0]


def message_lengths(wire):
    """The bytes of every message of a frame (its length prefix counts itself in)."""
    w = bytes(wire)
    out, p = [], 0
    while p < len(w):
        q, L, sh = p, 0, 0
        while True:
            b = w[q]
            q += 1
            L |= (b & 0x7F) << sh
            sh += 7
            if b < 0x80:
                break
        assert L >= q - p
        out.append(L)
        p += L
    assert p == len(w)
    return np.array(out, np.int64)


def tile_sums(lengths, tile):
    return [int(lengths[i: i + tile].sum()) for i in range(0, len(lengths), tile)]


# ---- archive batches --------------------------------------------------------------------------
def archive_decoded(m):
    d = nxo.Decoded(len(m.id), len(m.ctag) + 1, 1)
    for k in ("id", "tag", "fixed", "aux"):
        getattr(d, k)[:len(m.id)] = getattr(m, k)
    d.ctag[:len(m.ctag)] = m.ctag
    d.cfixed[:len(m.ctag)] = m.cfixed
    d.caux[:len(m.ctag)] = m.caux
    d.s.n_rows, d.s.n_children = len(m.id), len(m.ctag)
    return d


def archive_ref(m):
    return np.frombuffer(nxo.encode_archive(archive_decoded(m), m.heap), np.uint8)


def long_text_archive(n):
    """Archive rows with a 200-byte string in about a third of them: more bytes than the
    staging holds, so the tiles write row by row."""
    from netidx_amd import synth
    return synth.mixed_columns_ctl(n, seed=31, p_hb=0.0, p_long=0.35)[0]


def varint_len(v):
    return max(1, (int(v).bit_length() + 6) // 7)


def archive_tile_bytes(m):
    """The records' bytes per tile: the batch of the first k rows, less its count, at every tile
    boundary k."""
    d = archive_decoded(m)
    n = len(m.id)
    ends = []
    for k in list(range(GEN_TILE, n, GEN_TILE)) + [n]:
        d.s.n_rows = k
        ends.append(len(nxo.encode_archive(d, m.heap)) - varint_len(k))
    return [int(x) for x in np.diff([0] + ends)]


# ---- To::Write frames -------------------------------------------------------------------------
def writes_wire(n, ctl):
    from test_gpu_writes import rand_id, rand_writes
    msgs = rand_writes(n, 700 + n)
    if ctl:
        rng = random.Random(n)
        for i in range(max(2, n // 7)):
            m = ("unsub", rand_id(rng)) if i % 2 else \
                ("sub", dict(path="/c/%d" % i, token=b"k" * (i % 40)))
            msgs.insert(rng.randrange(len(msgs) + 1), m)
        msgs.append(("unsub", 1))  # after the last row
    return tw.batch(msgs)


# ---- f64 batches for the tiled encoder --------------------------------------------------------
def f64_ids(n, wide, seed):
    """wide: every id >= 2^28, records of 16 bytes and more, so that every full tile leaves the
    staging. Mixed, tile by tile:
      even tiles  F64_EDGE_WIDE 16-byte records, then 14-byte ones: a full tile comes to
                  F64_STAGED bytes exactly, the most that is still staged
      odd tiles   one 13-byte record, then 16-byte ones: past the staging (put_rec_global), and
                  the tiles behind start at an odd phase
    so that a staged tile is followed by a row-by-row one and that one by a staged one."""
    rng = np.random.default_rng(seed)
    if wide:
        return rng.integers(2**28, 2**40, n, dtype=np.uint64)
    i = np.arange(n)
    t, j = i // F64_TILE, i % F64_TILE
    ids = rng.integers(2**14, 2**21, n, dtype=np.uint64)             # 14-byte records
    big = rng.integers(2**28, 2**35, n, dtype=np.uint64)             # 16-byte records
    sel = np.where(t % 2 == 0, j < F64_EDGE_WIDE, j > 0)
    ids[sel] = big[sel]
    first = (t % 2 == 1) & (j == 0)
    ids[first] = rng.integers(2**7, 2**14, n, dtype=np.uint64)[first]  # 13-byte records
    return ids


def f64_tile_paths(ids):
    """[(bytes, goes past the staging)] per tile, from the oracle's encode of each tile's
    records and the kernel's condition (nxg_encode_f64.hip: phase + tbytes > MAXB_ALL - 16)."""
    vals = np.zeros(len(ids), np.uint64)
    out, base = [], 0
    for i in range(0, len(ids), F64_TILE):
        b = len(nxo.encode_f64(ids[i: i + F64_TILE], vals[i: i + F64_TILE]))
        out.append((b, (base & 15) + b > F64_STAGED))
        base += b
    return out
