"""A sequential model of an async backlog, and a generator of random backlogs -- TEST HELPER.

nxg_decode_updates_async / nxg_encode_updates_async enqueue work; nxg_ctx_sync completes it. A
call whose fast kernel declines is finished at sync time, after every later call has already
run, and nxg_ctx_sync then has to put the order right again (netidx_amd/csrc/nxg_api.cpp). What
the caller is promised is simple: the backlog behaves as if each call had run to completion
before the next one started. This module is that promise, executed on host copies with the CPU
oracle (tests/nxo.py), so that any backlog can be compared against it. It knows nothing of the
library's kernels, fallbacks or path-selection state, and imports nothing of the product but
its synthetic data (netidx_amd.synth).

Memory pool of a program (the same for every program, so that reuse is frequent):
  - N_BUFS byte buffers of `cap` bytes (the longest frame of the program, rounded up to 16) plus
    a MARGIN-byte margin, filled with SENT past the frame they start with;
  - N_F64 F64-layout column sets, each holding n rows;
  - one MIXED-layout column set (index MIXED), only ever a decode target.
Every frame and batch of one program has the same row count n, one of ROWS.

Frames (kind of the bytes a buffer holds):
  S  ids count up by one;
  P  a permutation of consecutive ids inside one varint width: every record has one length,
     but the ids are out of order;
  H  sequential ids and one Heartbeat (02 05) between two records; decoded into the MIXED
     column set only (F64 columns would report NOT_F64).
Column sets hold sequential (S) or permuted (P) ids.

Operations: ("D", buf, cols) decodes the frame in `buf` into column set `cols`; ("E", buf,
cols) encodes column set `cols` into `buf` (capacity `cap`). `Program.groups` lists the runs
[i0, i1) of consecutive decodes to be issued through one nxg_decode_frames_async call.
"""
from collections import namedtuple

import numpy as np

import nxo
from netidx_amd import synth

SENT = 0xEE
MARGIN = 64
N_BUFS = 3
N_F64 = 3
MIXED = N_F64  # index of the MIXED column set
N_COLS = N_F64 + 1
ROWS = (1, 300, 3000)
HEARTBEAT = b"\x02\x05"

Op = namedtuple("Op", "kind buf cols")


def D(buf, cols):
    return Op("D", buf, cols)


def E(cols, buf):
    return Op("E", buf, cols)


# ---- data ---------------------------------------------------------------------------------
# id ranges inside one varint width that hold 3000 consecutive ids
_WIDTH_RANGES = ((1 << 7, 1 << 14), (1 << 14, 1 << 21), (1 << 21, 1 << 28))


def values(n, seed):
    """n f64 bit patterns (netidx_amd.synth: uniform values and the special ones)."""
    return synth.f64_columns(n, seed)[1]


def seq_ids(n, base):
    return np.arange(base, base + n, dtype=np.uint64)


def perm_ids(n, rng):
    """A permutation of n consecutive ids inside one varint width (n == 1: the one id)."""
    lo, hi = _WIDTH_RANGES[int(rng.integers(0, len(_WIDTH_RANGES)))]
    base = int(rng.integers(lo, hi - n))
    return rng.permutation(seq_ids(n, base))


def frame(ids, vals, heartbeat_at=None):
    """The wire bytes of the rows (the oracle's encoder), with a Heartbeat before record
    `heartbeat_at` if given."""
    if heartbeat_at is None:
        return nxo.encode_f64(ids, vals)
    k = heartbeat_at
    assert 0 < k < len(ids), "a Heartbeat goes between two records"
    return np.concatenate([nxo.encode_f64(ids[:k], vals[:k]), np.frombuffer(HEARTBEAT, np.uint8),
                           nxo.encode_f64(ids[k:], vals[k:])])


def ids_kind(ids):
    ids = np.asarray(ids, np.uint64)
    return "S" if len(ids) < 2 or bool((ids[1:] - ids[:-1] == 1).all()) else "P"


# ---- programs -----------------------------------------------------------------------------
class Program:
    """n rows per batch; frames[b]: the bytes buffer b starts with; cols[c]: (ids, vals) that F64
    column set c starts with; ops; groups: runs of decodes issued as one frames call."""

    def __init__(self, n, frames, cols, ops, groups=(), name=""):
        # (a hand-built scenario may bring a fourth buffer; random programs have N_BUFS)
        assert len(frames) >= N_BUFS and len(cols) == N_F64
        self.n_bufs = len(frames)
        self.n = n
        self.frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        self.cols = [(np.ascontiguousarray(i, np.uint64), np.ascontiguousarray(v, np.uint64))
                     for i, v in cols]
        assert all(len(i) == n and len(v) == n for i, v in self.cols)
        self.ops = [Op(*o) for o in ops]
        self.groups = [tuple(g) for g in groups]
        self.name = name
        for o in self.ops:
            assert o.kind in "DE" and 0 <= o.buf < self.n_bufs
            assert 0 <= o.cols < (N_COLS if o.kind == "D" else N_F64), "MIXED is never encoded"
        for i0, i1 in self.groups:
            assert i1 - i0 >= 2 and all(o.kind == "D" for o in self.ops[i0:i1])
            # nxg_decode_frames_async: its frames are complete when the call is made, so none
            # is the output of an encode still queued
            assert not any(w.kind == "E" and w.buf == o.buf
                           for o in self.ops[i0:i1] for w in self.ops[:i0])
        # the longest frame any buffer can come to hold: every frame of the program is one the
        # buffers start with, or the encoding of rows that the columns or those frames hold
        longest = max([len(f) for f in self.frames] + [len(frame(i, v)) for i, v in self.cols])
        self.cap = (longest + 15) & ~15

    def buffers(self):
        """The buffers' initial bytes: the frame, then SENT up to cap + MARGIN."""
        out = []
        for f in self.frames:
            b = np.full(self.cap + MARGIN, SENT, np.uint8)
            b[:len(f)] = f
            out.append(b)
        return out

    def describe(self):
        return f"{self.name} n={self.n} " + " ".join(
            f"{o.kind}(b{o.buf}{'->' if o.kind == 'D' else '<-'}c{o.cols})" for o in self.ops) + \
            (f" groups={self.groups}" if self.groups else "")


def reads(op):
    """The pool memory a call reads: a decode its frame buffer, an encode its input columns."""
    return ("buf", op.buf) if op.kind == "D" else ("cols", op.cols)


def writes(op):
    return ("cols", op.cols) if op.kind == "D" else ("buf", op.buf)


def hazards(ops):
    """(reader index, later writer index) pairs: a later call of the program writes into memory
    that an earlier one reads. Derived from the program alone."""
    return [(i, j) for i in range(len(ops)) for j in range(i + 1, len(ops))
            if reads(ops[i]) == writes(ops[j])]


class Result:
    """What a backlog must leave behind (Program executed one call after another)."""


def run(prog):
    """Execute the program sequentially on host copies. Returns a Result:
      d_len[i]     the frame length decode i must be given (None for an encode)
      len_out[i]   the length encode i reports (None for a decode)
      frame_kind[i] / batch_kind[i]  S, P or H of what call i reads
      bufs[b]      final bytes of buffer b, margin included
      cols[c]      {"id", "fixed", "n_rows", "n_heartbeat"} of column set c at the end
      status       (n_rows, err_kind, n_heartbeat) nxg_ctx_sync returns: the last decode's, or
                   zeros for a backlog of encodes
      hazards      the (reader, later writer) pairs; stable = there are none
    """
    bufs = prog.buffers()
    lens = [len(f) for f in prog.frames]
    cols = [{"id": i.copy(), "fixed": v.copy(), "n_rows": prog.n, "n_heartbeat": 0}
            for i, v in prog.cols]
    cols.append({"id": np.zeros(0, np.uint64), "fixed": np.zeros(0, np.uint64), "n_rows": 0,
                 "n_heartbeat": 0})
    r = Result()
    k = len(prog.ops)
    r.d_len, r.len_out = [None] * k, [None] * k
    r.frame_kind, r.batch_kind = [None] * k, [None] * k
    r.status = (0, 0, 0)
    for i, op in enumerate(prog.ops):
        if op.kind == "D":
            L = lens[op.buf]
            o = nxo.decode(bufs[op.buf][:L].copy()).trim()
            assert o["err_kind"] == 0, "malformed frames are out of the model's scope"
            assert o["n_heartbeat"] == 0 or op.cols == MIXED, "an H frame goes to MIXED columns"
            assert len(o["id"]) == prog.n
            cols[op.cols] = {"id": o["id"].copy(), "fixed": o["fixed"].copy(),
                             "n_rows": len(o["id"]), "n_heartbeat": int(o["n_heartbeat"])}
            r.d_len[i] = L
            r.frame_kind[i] = "H" if o["n_heartbeat"] else ids_kind(o["id"])
            r.status = (len(o["id"]), 0, int(o["n_heartbeat"]))
        else:
            c = cols[op.cols]
            w = nxo.encode_f64(c["id"], c["fixed"])
            assert len(w) <= prog.cap
            bufs[op.buf][:len(w)] = w
            lens[op.buf] = len(w)
            r.len_out[i] = len(w)
            r.batch_kind[i] = ids_kind(c["id"])
    r.bufs, r.cols = bufs, cols
    r.hazards = hazards(prog.ops)
    r.stable = not r.hazards
    return r


# ---- what a program exercises (for choosing the committed seeds) -----------------------------
def late_decode_then_touch(prog, res):
    """A decode of a P or H frame (the decoders that try first decline those) followed by a call
    that reads or overwrites its columns."""
    ops = prog.ops
    return any(ops[i].kind == "D" and res.frame_kind[i] in "PH" and
               any(("cols", ops[i].cols) in (reads(ops[j]), writes(ops[j]))
                   for j in range(i + 1, len(ops)))
               for i in range(len(ops)))


def late_encode_then_read(prog, res):
    """An encode of permuted ids (the sequential-id encoder declines them) followed by a decode
    of its output."""
    ops = prog.ops
    return any(ops[i].kind == "E" and res.batch_kind[i] == "P" and
               any(reads(ops[j]) == ("buf", ops[i].buf) for j in range(i + 1, len(ops)))
               for i in range(len(ops)))


# ---- random programs -----------------------------------------------------------------------
def generate(seed):
    """Random program `seed`: n from ROWS, S / P / H frames and S / P columns, 3 to 8 calls
    over the pool; half of the programs issue their runs of decodes as frames calls."""
    rng = np.random.default_rng([0xBAC10C, seed])
    n = int(rng.choice(ROWS, p=(0.1, 0.45, 0.45)))

    def ids(kind):
        if kind == "P":
            return perm_ids(n, rng)
        # sequential ids from anywhere below 2^21, so that some cross a varint width change
        return seq_ids(n, int(rng.integers(0, (1 << 21) - n)))

    kinds = "S" if n == 1 else "SPH"
    buf_kind = [str(rng.choice(list(kinds))) for _ in range(N_BUFS)]
    frames = []
    for b, kd in enumerate(buf_kind):
        hb = int(rng.integers(1, n)) if kd == "H" else None
        frames.append(frame(ids(kd), values(n, 1000 * seed + b), hb))
    col_kind = [str(rng.choice(list(kinds[:2]))) for _ in range(N_F64)] + ["S"]
    cols = [(ids(kd), values(n, 1000 * seed + 10 + c)) for c, kd in enumerate(col_kind[:N_F64])]
    # two programs in three avoid hazards: a call that would write what an earlier one reads is
    # drawn again (the program ends early if no call fits)
    avoid = rng.random() < 0.67
    ops = []
    for _ in range(int(rng.integers(3, 9))):
        for _try in range(30):
            if rng.random() < 0.55:
                b = int(rng.integers(0, N_BUFS))
                c = MIXED if buf_kind[b] == "H" or rng.random() < 0.2 else \
                    int(rng.integers(0, N_F64))
                op = D(b, c)
            else:
                op = E(int(rng.integers(0, N_F64)), int(rng.integers(0, N_BUFS)))
            if not (avoid and any(reads(o) == writes(op) for o in ops)):
                break
        else:
            break
        ops.append(op)
        if op.kind == "D":
            col_kind[op.cols] = "P" if buf_kind[op.buf] == "P" else "S"
        else:
            buf_kind[op.buf] = col_kind[op.cols]
    assert len(ops) >= 3
    groups = []
    if rng.random() < 0.5:
        i = 0
        while i < len(ops):
            j = i
            while j < len(ops) and ops[j].kind == "D" and not any(
                    w.kind == "E" and w.buf == ops[j].buf for w in ops[:i]):
                j += 1
            if j - i >= 2:
                groups.append((i, j))
            i = max(j, i + 1)
    return Program(n, frames, cols, ops, groups, name=f"seed{seed}")


# ---- hand-built backlogs --------------------------------------------------------------------
def _pool(n, seed, frame_kinds="SSS", col_kinds="SSS"):
    """Frames and columns of the given kinds, every one with ids and values of its own."""
    rng = np.random.default_rng([0x5CE9A, seed])

    def ids(kind, k):
        return perm_ids(n, rng) if kind == "P" else seq_ids(n, 1000 + 5000 * k)

    frames = [frame(ids(kd, b), values(n, 100 * seed + b), n // 2 if kd == "H" else None)
              for b, kd in enumerate(frame_kinds)]
    cols = [(ids(kd, 10 + c), values(n, 100 * seed + 10 + c)) for c, kd in enumerate(col_kinds)]
    return frames, cols


def scenario_late_decode_shared_columns(n=300, first="P"):
    """tests/test_gpu_f64_seq.py, test_async_backlog_keeps_wire_order_after_a_late_fallback, its
    first and third parts: one frames call of a frame the first decoders decline (P, or H into
    the MIXED columns) and a sequential one into the same columns; the later frame's rows stay."""
    frames, cols = _pool(n, 1, first + "SS")
    c = MIXED if first == "H" else 0
    return Program(n, frames, cols, [D(0, c), D(1, c)], [(0, 2)], name=f"late-decode-{first}")


def scenario_late_decode_then_encode(n=300):
    """The same test's second part: decode of a P frame, an encode of its columns, a decode of
    another frame; the encode must see the P frame's rows."""
    frames, cols = _pool(n, 2, "PSS")
    return Program(n, frames, cols, [D(0, 1), E(1, 2), D(1, 0)], name="late-decode-encode")


def scenario_late_encode_then_decode(n=300):
    """tests/test_gpu_f64_enc_seq.py, test_seq_encode_async_backlog_with_late_fallback: three
    encodes (sequential, permuted, sequential ids) and a decode of the second one's output."""
    frames, cols = _pool(n, 3, "SSS", "SPS")
    return Program(n, frames, cols, [E(0, 0), E(1, 1), E(2, 2), D(1, MIXED)],
                   name="late-encode-decode")


def scenario_frame_overwritten(n=300):
    """tests/test_gpu_api.py, test_async_fallback_frame_overwritten_fails_loudly: a decode of a P
    frame and an encode into that frame's buffer. Hazardous: (0, 1)."""
    frames, cols = _pool(n, 4, "PSS")
    return Program(n, frames, cols, [D(0, 0), E(1, 0)], name="frame-overwritten")


def scenario_write_after_write(n=300):
    """Two encodes into one buffer X, each followed by a decode of X: the first batch has
    permuted ids, the second sequential ones. Hazardous: (1, 2), the first decode's frame is
    written by the second encode."""
    frames, cols = _pool(n, 5, "SSS", "PSS")
    return Program(n, frames, cols, [E(0, 0), D(0, 2), E(1, 0), D(0, MIXED)],
                   name="write-after-write")


def scenario_stale_redo(n=300):
    """decode(F0 -> C) of a P frame, decode(F1 -> C) of an S frame, encode(K -> F1) of
    sequential ids. Hazardous: (1, 2)."""
    frames, cols = _pool(n, 6, "PSS")
    return Program(n, frames, cols, [D(0, 0), D(1, 0), E(1, 1)], name="stale-redo")


def scenario_relay(n=300, kind="S"):
    """decode f1 -> cols, encode cols -> o1, decode f2 -> cols, encode cols -> o2 (a fourth
    buffer). Hazardous: (1, 2), the first encode's columns are written by the second decode."""
    frames, cols = _pool(n, 7, kind + "S" + kind + "S")
    return Program(n, frames, cols, [D(0, 0), E(0, 1), D(2, 0), E(0, 3)], name=f"relay-{kind}")


# The committed programs. Chosen on the CPU (tests/test_backlog_model_cpu.py asserts what they
# cover): mostly input-stable ones, whose results must equal the model in every context state,
# and enough hazardous ones to exercise the loud-error rule.
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25,
         26, 27, 28, 29, 30, 31, 32, 33, 34, 36, 37, 38, 39, 40, 41, 42, 44, 45, 50, 51, 52, 53, 54,
         56, 58, 59, 60, 62, 63, 65, 67, 70, 71, 74, 75, 77, 78, 79, 80, 81, 82, 83, 84, 86, 88, 89,
         91, 92, 93, 97, 98, 99, 102, 103, 104, 113, 114, 116, 123, 129, 135, 165, 181, 202, 203,
         204, 227, 248, 249, 253)
