"""The value table's case table (tests/test_value_table_cpu.py, tests/test_gpu_value_table.py).

`plan()` reads the kernels' constants out of netidx_amd/csrc/nxg_value_table.hip, and every case
states the branch it is there for; `*_branch` compute, from those constants, the branch a case
really takes. A retune then names the case that left its branch (tests/fanout_cases.py does the
same for the fan-out kernels).
"""
import os
import re
import struct

import numpy as np

from value_table_model import (DEPTH, HEAP, KIDS, NOKIDS, ROW, TAG, Model, Source, elems,
                               walk_branch)

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc",
                   "nxg_value_table.hip")


def plan():
    src = open(HIP).read()

    def const(name):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m, f"{name} not found in nxg_value_table.hip"
        return int(m.group(1))

    return dict(block=const("VT_SLOTS_PER_BLOCK"), top=const("VT_TOP_WIDTH"),
                copy=const("VT_COPY_BLOCK"))


# ---- table sizes -----------------------------------------------------------------------------
def slot_cases(p):
    """(name, n_slots, (blocks, top steps)): one wave, one block and one top step, each +- 1."""
    B, T = p["block"], p["top"]

    def c(name, n):
        return (name, n, slots_branch(p, n))

    return [c("one", 1), c("wave-1", 63), c("wave", 64), c("wave+1", 65), c("block-1", B - 1),
            c("block", B), c("block+1", B + 1), c("top-1", T - 1), c("top", T), c("top+1", T + 1)]


def slots_branch(p, n):
    blocks = -(-n // p["block"])
    return blocks, -(-blocks // p["top"])


def top_step_slots(p):
    """The smallest table whose block sums need a second step of the top scan."""
    return p["block"] * p["top"] + 1


# ---- values ----------------------------------------------------------------------------------
def f64(x):
    return ("sc", 9, struct.unpack("<Q", struct.pack("<d", x))[0], 0)


def text(n, tag=12, seed=0):
    return ("txt", tag, bytes((seed + 7 * i) & 0xFF for i in range(n)))


def dec(m, scale=0, neg=False):
    return ("dec", struct.pack("<IIII", (scale << 16) | (0x80000000 if neg else 0),
                               m & 0xFFFFFFFF, (m >> 32) & 0xFFFFFFFF, (m >> 64) & 0xFFFFFFFF))


def nested(depth, leaf=("sc", 6, 1, 0)):
    v = leaf
    for _ in range(depth):
        v = ("arr", [v])
    return v


I64 = 0xFFFFFFFFFFFFFFFF  # -1, sign-extended
# every fixed-size tag (17 included, as stored), with a non-trivial fixed / aux
SCALARS = [("sc", 0, 0xFFFFFFFF, 0), ("sc", 1, 300, 0), ("sc", 2, 0xFFFFFFFE, 0),
           ("sc", 3, I64, 0), ("sc", 4, 1 << 63, 0), ("sc", 5, 1 << 40, 0), ("sc", 6, I64 - 5, 0),
           ("sc", 7, I64, 0), ("sc", 8, 0x7FC00001, 0), f64(float("nan")), f64(-0.0),
           ("sc", 10, 1700000000, 999999999), ("sc", 11, 86400, 1), ("sc", 14, 0, 0),
           ("sc", 15, 0, 0), ("sc", 16, 0, 0), ("sc", 17, 0, 0), ("sc", 23, 255, 0),
           ("sc", 24, 0x80, 0), ("sc", 25, 65535, 0), ("sc", 26, 0x8000, 0),
           ("sc", 0x40, 0, 0)]
TEXT_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100_000]
ABSTRACT = ("txt", 27, bytes(range(16)) + b"payload")

# name -> (value, the walk it is there for)
VALUES = {
    "decimal": (dec(15, 1), "leaf"),
    "abstract": (ABSTRACT, "leaf"),
    "bytes": (text(9, 13, 3), "leaf"),
    "error_string": (text(5, 18, 9), "leaf"),
    "array0": (("arr", []), "scalar"),
    "array1": (("arr", [f64(1.5)]), "flat"),
    "array63": (("arr", [("sc", 6, i, 0) for i in range(63)]), "flat"),
    "array64": (("arr", [("sc", 6, i, 0) for i in range(64)]), "flat"),
    "array65": (("arr", [("sc", 6, i, 0) for i in range(65)]), "flat"),
    "array_strings": (("arr", [text(n, 12, n) for n in (3, 0, 17, 40)]), "flat"),
    "array_mixed_leaves": (("arr", [dec(3), ABSTRACT, text(2), f64(2.0)]), "flat"),
    "map": (("map", [(("sc", 6, 1, 0), text(4)), (("sc", 6, 2, 0), dec(7, 2))]), "flat"),
    "error_value": (("err", ("sc", 6, 9, 0)), "flat"),
    "error_text_child": (("err", text(6)), "flat"),
    "nest3": (("arr", [("map", [(text(1), ("arr", [text(20), ("err", dec(1))]))]), text(3),
                       ("arr", [])]), "stack"),
    "nest_map_of_arrays": (("map", [(("sc", 6, 0, 0), ("arr", [text(5), text(6)])),
                                    (("sc", 6, 1, 0), ("arr", [("arr", [f64(0.5)])]))]), "stack"),
    "depth_max": (nested(32), "stack"),
}


def value_branch(v):
    """'scalar' also for an empty container: no payload, nothing to walk."""
    b = walk_branch(v)
    return "scalar" if b == "flat" and not v[1] else b


# ---- the copy kernel's blocks --------------------------------------------------------------------
def copy_branch(p, phase, lo, seg_lens):
    """(blocks moved with one 16-byte load and store, blocks moved byte by byte) for segments of
    these lengths appended at heap offset `lo` of a heap whose address is `phase` mod 16."""
    C = p["copy"]
    hi = lo + sum(seg_lens)
    starts = np.concatenate([[lo], lo + np.cumsum(seg_lens)]).astype(np.int64)
    wide = narrow = 0
    b = (lo + phase) // C
    while b * C < hi + phase:
        a_lo, a_hi = b * C - phase, b * C - phase + C
        b_lo, b_hi = max(a_lo, lo), min(a_hi, hi)
        if b_lo < b_hi:
            seg = int(np.searchsorted(starts, b_lo, side="right")) - 1
            if b_hi - b_lo == C and starts[seg + 1] >= b_hi:
                wide += 1
            else:
                narrow += 1
        b += 1
    return wide, narrow


# ---- sources -----------------------------------------------------------------------------------
def scrambled_source(trees):
    """The trees in a layout no encoder or decoder here writes: a container's block comes after
    the blocks of everything below it (postorder), and junk bytes lie between the payloads."""
    ctag, cfixed, caux, heap = [], [], [], bytearray(b"\xEE\xEE\xEE")

    def emit(v):
        k = v[0]
        if k == "sc":
            return v[1], v[2], v[3]
        if k in ("txt", "dec"):
            t, b = (v[1], v[2]) if k == "txt" else (20, v[1])
            off = len(heap)
            heap.extend(b + b"\xEE" * (1 + len(b) % 3))
            return t, off, len(b)
        slots = [emit(x) for x in reversed(elems(v))][::-1]  # children first, last child first
        base = len(ctag)
        for t, f, a in slots:
            ctag.append(t), cfixed.append(f), caux.append(a)
        return {"arr": 19, "map": 21, "err": 22}[k], base, len(v[1]) if k != "err" else 1

    rows = [emit(v) for v in reversed(trees)][::-1]
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    return Source(col(0, np.uint8), col(1, np.uint64), col(2, np.uint32), np.array(ctag, np.uint8),
                  np.array(cfixed, np.uint64), np.array(caux, np.uint32), bytes(heap))


def source_of(trees, f64_layout=False):
    """The trees as batch columns (tests/test_publish_values_cpu.py Layout order)."""
    m = Model(len(trees), 1 << 40, 1 << 40)
    for s, v in enumerate(trees):
        m._store(s, v)
    a = m.arrays()
    if f64_layout:
        return Source(None, a["fixed"].copy(), None)
    return Source(a["tag"].copy(), a["fixed"].copy(), a["aux"].copy(), a["ctag"], a["cfixed"],
                  a["caux"], bytes(m.heap))


# name -> (rows, edit(Source, row) making `row` bad, cause). `row` holds rows[0]; the edit keeps
# every other row valid.
def _bad_tag(S, r):
    S.tag[r] = 28


def _bad_child_tag(S, r):
    S.ctag[int(S.fixed[r])] = 0x41


def _bad_heap(S, r):
    S.fixed[r] = S.heap_len - int(S.aux[r]) + 1


def _bad_heap_child(S, r):
    S.cfixed[int(S.fixed[r]) + 1] = S.heap_len + 1


def _bad_kids(S, r):
    S.aux[r] = S.n_children - int(S.fixed[r]) + 1


def _bad_kids_start(S, r):
    S.fixed[r] = S.n_children + 1


def _no_kids(S, r):
    S.ctag = S.cfixed = S.caux = None
    S.n_children = 0


REFUSALS = {
    "tag": (text(3), _bad_tag, TAG),
    "child_tag": (("arr", [f64(1.0), f64(2.0)]), _bad_child_tag, TAG),
    "heap": (text(5), _bad_heap, HEAP),
    "heap_child": (("arr", [text(2), text(3)]), _bad_heap_child, HEAP),
    "kids": (("arr", [f64(1.0)]), _bad_kids, KIDS),
    "kids_start": (("arr", [f64(1.0)]), _bad_kids_start, KIDS),
    "no_child_columns": (("err", f64(3.0)), _no_kids, NOKIDS),
    "depth": (nested(33), None, DEPTH),
    "row": (f64(1.0), None, ROW),
}


# Values the table holds, edited in place: name -> (value, edit(model, slot) -> (array, index,
# new element), cause). The edit is applied to the model's arrays and to the device's alike.
OLD_REFUSALS = {
    "old_tag": (text(4), lambda m, s: ("tag", s, 28), TAG),
    "old_child_tag": (("arr", [f64(1.0), f64(2.0)]),
                      lambda m, s: ("ctag", int(m.fixed[s]) + 1, 28), TAG),
    "old_kids": (("arr", [f64(1.0), f64(2.0)]),
                 lambda m, s: ("aux", s, m.child_used - int(m.fixed[s]) + 1), KIDS),  # one past
    "old_heap": (text(6), lambda m, s: ("fixed", s, m.heap_used - int(m.aux[s]) + 1), HEAP),
}
