"""The case table of tests/test_gpu_decode_bounds.py (test infrastructure): which frame goes to
which decoder with which capacities, and whether those are short of the frame's needs.

The GPU tests take the expected outcome of every case from the oracle
(nxo.decode(wire, cap_rows=, cap_children=, cap_ctl=), oracle/nx_oracle.c); the table's own
`short` flag is checked against the oracle on the CPU (tests/test_decode_bounds_cpu.py), together
with every frame being well formed. Malformed-and-too-small frames are not in the table: the
device reports the format error first and the sequential oracle whichever it meets first.

A row set {n, n-1, n-2, n//2, n//2+1, 1} keeps its members >= 0: a capacity of 0 rows (arrays that
may not be written at all) is a case, a negative one is not.
"""
import functools
import random
from typing import NamedTuple, Tuple

import numpy as np

import nxo
from frames import golden_twin, rich_wire

LAYOUT_F64, LAYOUT_MIXED = 1, 2
HINT_MIXED = 1
CAPACITY = 7
KINDS = ("rows", "children", "ctl")

# sequential-id f64 decoder: a wave is 256 records (a workgroup 1024) below 256 MiB; first ids 0
# and 16300 cross 2^7 and 2^14 inside the first wave (the mixed-width paired emit), 100 leaves
# whole waves of one width (the uniform paired emit); the last wave is the edge emit
SEQ_N = (1, 2, 3, 255, 256, 257, 1025, 3001)
SEQ_I0 = (0, 100, 16300)
# length-run and single-pass f64 decoders: 12-byte records, 2730 of which fill a 32 KiB tile and
# 2731 do not; 6000 and 20000 span several tiles
F64_N = (1, 2, 2730, 2731, 6000, 20000)
# The length-run probe expects a tile's ids to count up, so one-byte ids (below 2^7) in a tile of
# more than 127 records look to it as if they crossed into two-byte ids: it finds they do not and
# such a tile is decoded by the exact walk (exact_tile), not by the run emit (emit_pairs,
# emit_runs). The run emit's guards are reached by 14-byte records (three-byte ids), 2340 of
# which fill a tile.
RUN14_N = (2340, 2341, 6000, 20000)
ARCHIVE_N = 4000


class Case(NamedTuple):
    decoder: str   # the context that takes it: seq | run | x | fast | general | host
    frame: Tuple   # key of wire()
    layout: int
    flags: int
    caps: Tuple[int, int, int]   # rows, children, ctl
    short: bool    # some capacity is below the frame's need
    label: str


@functools.lru_cache(maxsize=None)
def wire(key):
    """The frame of `key` as a uint8 array."""
    from netidx_amd import synth
    kind = key[0]
    if kind == "seq":
        _, n, i0 = key
        ids, vals = synth.f64_columns(n, 1000 + n + i0, id_offset=i0)
        return nxo.encode_f64(ids, vals)
    if kind == "run":  # ids of one width (one byte) in permuted order: every record 12 bytes
        n, v = key[1], (key[2] if len(key) > 2 else 0)  # (v: another frame of the same shape)
        _, vals = synth.f64_columns(n, 2000 + n + v)
        ids = (np.random.default_rng(n + v).permutation(n) % 128).astype(np.uint64)
        return nxo.encode_f64(ids, vals)
    if kind == "run14":  # three-byte ids in permuted order: every record 14 bytes. No tile's ids
        # can reach the next width (2^21), so the length-run probe takes each tile as one run
        n, v = key[1], (key[2] if len(key) > 2 else 0)
        _, vals = synth.f64_columns(n, 4000 + n + v)
        ids = (2**14 + np.random.default_rng(7 + n + v).permutation(n)).astype(np.uint64)
        return nxo.encode_f64(ids, vals)
    if kind == "x":  # random ids of 1..5 bytes: record lengths vary record to record
        n = key[1]
        _, vals = synth.f64_columns(n, 3000 + n)
        rng = np.random.default_rng(n + 1)
        bits = rng.choice([7, 14, 21, 28, 35], n)
        ids = rng.integers(0, 2**62, n, dtype=np.uint64) >> (62 - bits).astype(np.uint64)
        return nxo.encode_f64(ids, vals)
    if kind == "flat":
        return _flat_wire()
    if kind == "rich":  # Maps, Error(Value), three levels of nesting, Heartbeats, Unsubscribed
        return rich_wire(1500, 5)
    raise KeyError(key)


def _flat_wire():
    """3000 short Updates the fast mixed decoder takes (4 KiB tiles: about 15 of them): every
    third an Array of 2 to 5 scalars, a Heartbeat every 50 messages."""
    mg = golden_twin()
    rng = random.Random(41)

    def scalar():
        k = rng.randrange(4)
        if k == 0:
            return (9, rng.getrandbits(64))
        if k == 1:
            return (6, rng.randint(-2**40, 2**40))
        if k == 2:
            return (12, b"s" * rng.randrange(0, 20))
        return (10, (rng.randrange(4_000_000_000), rng.randrange(10**9)))

    msgs = []
    for i in range(3000):
        if i % 50 == 49:
            msgs.append(("hb",))
        v = (19, [scalar() for _ in range(rng.randrange(2, 6))]) if i % 3 == 0 else scalar()
        msgs.append(("u", rng.getrandbits(rng.choice([7, 14, 21])), v))
    w, _ = mg.batch(msgs)
    return np.frombuffer(w, np.uint8).copy()


@functools.lru_cache(maxsize=None)
def need(key):
    """(rows, children, ctl) of the frame, from the oracle with room to spare."""
    o = nxo.decode(wire(key))
    return (int(o.s.n_rows), int(o.s.n_children), int(o.s.n_ctl))


def row_caps(n):
    """{n, n-1, n-2, n//2, n//2+1, 1}, the members >= 0, the exact one first."""
    return sorted({c for c in (n, n - 1, n - 2, n // 2, n // 2 + 1, 1) if c >= 0}, reverse=True)


def _f64_cases(decoder, key):
    n = need(key)[0]
    return [Case(decoder, key, LAYOUT_F64, 0, (c, 1, 1), c < n, f"rows={c}/{n}")
            for c in row_caps(n)]


def _mixed_cases(decoder, key):
    nd = need(key)
    assert min(nd) >= 2, nd
    out = [Case(decoder, key, LAYOUT_MIXED, HINT_MIXED, nd, False, "all_exact")]
    for k, kind in enumerate(KINDS):
        roomy = [x + 3 for x in nd]
        roomy[k] = nd[k]
        out.append(Case(decoder, key, LAYOUT_MIXED, HINT_MIXED, tuple(roomy), False,
                        f"{kind}_exact"))
        short = list(nd)
        short[k] -= 1
        out.append(Case(decoder, key, LAYOUT_MIXED, HINT_MIXED, tuple(short), True,
                        f"{kind}_one_short"))
    return out


def frames_of(decoder):
    """The frame keys a decoder's context takes, in test order."""
    return {
        "seq": [("seq", n, i0) for n in SEQ_N for i0 in SEQ_I0],
        "run": [("run", n) for n in F64_N] + [("run14", n) for n in RUN14_N],
        "x": [("x", n) for n in F64_N],
        "fast": [("flat",)],
        "general": [("flat",), ("rich",)],
        "host": [("seq", 3001, 100), ("flat",)],
    }[decoder]


def cases(decoder, key):
    """The cases of one frame on one decoder, the exact-capacity one first."""
    if decoder in ("seq", "run", "x"):
        return _f64_cases(decoder, key)
    if decoder in ("fast", "general"):
        return _mixed_cases(decoder, key)
    if decoder == "host":  # pinned-host columns: exact, and rows one short
        nd = need(key)
        f64 = key[0] == "seq"
        layout, flags = (LAYOUT_F64, 0) if f64 else (LAYOUT_MIXED, HINT_MIXED)
        exact = (nd[0], 1, 1) if f64 else nd
        return [Case("host", key, layout, flags, exact, False, "exact"),
                Case("host", key, layout, flags, (exact[0] - 1,) + tuple(exact[1:]), True,
                     "rows_one_short")]
    raise KeyError(decoder)


DECODERS = ("seq", "run", "x", "fast", "general", "host")


def all_cases():
    return [c for d in DECODERS for k in frames_of(d) for c in cases(d, k)]


def backlog_cases():
    """nxg_decode_frames_async: three frames of 3001 records, the middle one's columns one row
    short. {context: [(frame key, caps, short)] * 3}"""
    out = {}
    for decoder, keys in (("seq", [("seq", 3001, 0), ("seq", 3001, 100), ("seq", 3001, 16300)]),
                          ("run", [("run14", 3001, 0), ("run14", 3001, 1), ("run14", 3001, 2)])):
        out[decoder] = [(k, (need(k)[0] - (j == 1), 1, 1), j == 1) for j, k in enumerate(keys)]
    return out


# ---- archive batches -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def archive_wire():
    from netidx_amd import synth
    m = synth.archive_columns(ARCHIVE_N, seed=77)
    d = nxo.Decoded(len(m.id), len(m.ctag) + 1, 1)
    for k in ("id", "tag", "fixed", "aux"):
        getattr(d, k)[:len(m.id)] = getattr(m, k)
    d.ctag[:len(m.ctag)] = m.ctag
    d.cfixed[:len(m.ctag)] = m.cfixed
    d.caux[:len(m.ctag)] = m.caux
    d.s.n_rows, d.s.n_children = len(m.id), len(m.ctag)
    return np.frombuffer(nxo.encode_archive(d, m.heap), np.uint8).copy()


def archive_cases():
    """[(label, (cap_rows, cap_children), short)]: both exact, rows one short, children one short."""
    d, used = nxo.decode_archive(archive_wire())
    assert used == len(archive_wire()) and d.s.err_kind == 0
    nr, nc = int(d.s.n_rows), int(d.s.n_children)
    assert nr == ARCHIVE_N and nc >= 2
    return [("both_exact", (nr, nc), False), ("rows_one_short", (nr - 1, nc), True),
            ("children_one_short", (nr, nc - 1), True)]
