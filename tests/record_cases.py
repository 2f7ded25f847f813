"""nxg_record_entries' case table (tests/test_record_cpu.py, tests/test_gpu_record.py).

`constants()` reads the kernels' constants out of netidx_amd/csrc/nxg_record.hip; `plan()`
computes from them which branches a case reaches, and every case states what it is there for
(`want`). A retune then names the case that no longer sits on its edge.
"""
import os
import re

import numpy as np

from record_model import ENT_SPAN, NO_SLOT, Case, item_lens
from record_model import BIG, DEPTH, KIDS, NOKIDS, ROW, TAG  # noqa: F401  (re-exported)
from value_table_cases import ABSTRACT, dec, f64, nested, source_of
from value_table_model import Source

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc",
                   "nxg_record.hip")


def constants():
    src = open(HIP).read()

    def const(name):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m, f"{name} not found in nxg_record.hip"
        return int(m.group(1))

    return dict(block=const("REC_ENTRIES_PER_BLOCK"), tile=const("REC_ENTRIES_PER_TILE"),
                staging=const("REC_STAGING_BYTES"), top=const("REC_TOP_WIDTH"))


# ---- the branches a case reaches ------------------------------------------------------------------
def _vl(v):
    return 1 + sum(v >= (1 << s) for s in (7, 14, 21, 28, 35, 42, 49, 56, 63))


def row_walk(S, row):
    """How the kernels walk a row: 'unsub', 'scalar' (sized from the row), 'flat' (an array of
    non-containers, in registers) or 'stack' (the wave's LDS stack)."""
    if S.tag is None:
        return "scalar"
    t = int(S.tag[row])
    if t == 0x40:
        return "unsub"
    if t not in (19, 21, 22):
        return "scalar"
    if t != 19:
        return "stack"
    f, a = int(S.fixed[row]), int(S.aux[row])
    return "stack" if any(int(S.ctag[f + k]) in (19, 21, 22) for k in range(a)) else "flat"


def plan(case, K=None):
    """The branches of a call that succeeds: blocks, groups (of the top scan), tiles; tiles staged
    in LDS / written directly / with nothing kept; the walks of the kept rows; the widths of the
    count varints; entries dropped; channels without a record."""
    K = K or constants()
    n = case.n_entries
    kept, _ = case.keep()
    lens = item_lens(case)
    off = case.chan_off.astype(np.int64)
    lead = np.zeros(n, np.int64)
    widths, empty = set(), 0
    for c in range(case.n_chans):
        idx = np.flatnonzero(kept[off[c]:off[c + 1]])
        if len(idx):
            lead[off[c] + idx[0]] = _vl(len(idx))
            widths.add(_vl(len(idx)))
        else:
            empty += 1
    staged = direct = idle = 0
    T = K["tile"]
    for t0 in range(0, n, T):
        if not kept[t0:t0 + T].any():
            idle += 1
        elif int((lens[t0:t0 + T] + lead[t0:t0 + T]).sum()) > K["staging"]:
            direct += 1
        else:
            staged += 1
    span = case.is_span()
    walks = {"unsub"} if (kept & span).any() else set()
    for r in np.unique(case.ent_row[kept & ~span]):
        walks.add(row_walk(case.src, int(r)))
    blocks = -(-n // K["block"])
    return dict(blocks=blocks, groups=-(-blocks // K["top"]), tiles=-(-n // T), staged=staged,
                direct=direct, idle=idle, walks=walks, widths=widths,
                dropped=int((~kept).sum()), empty=empty, chans=case.n_chans)


def reaches(p, want):
    """Does the plan p have what the case is there for? Sets: at least these; numbers: exactly."""
    for k, v in want.items():
        if isinstance(v, set):
            if not v <= p[k]:
                return False
        elif p[k] != v:
            return False
    return True


# ---- batches --------------------------------------------------------------------------------------
def text(n, tag=12, seed=0):
    """n bytes of text: printable ASCII, so that a String decodes (str::from_utf8)."""
    return ("txt", tag, bytes(32 + (seed + 7 * i) % 95 for i in range(n)))


def f64_source(n_rows=300):
    return source_of([f64(1.5 * i - 7) for i in range(n_rows)])


I64 = 0xFFFFFFFFFFFFFFFF
# every fixed-size tag, with a non-trivial fixed / aux
SCALARS = [("sc", 0, 0xFFFFFFFF, 0), ("sc", 1, 300, 0), ("sc", 2, 0xFFFFFFFE, 0),
           ("sc", 3, 0xFFFFFFFF, 0), ("sc", 4, 1 << 63, 0), ("sc", 5, 1 << 40, 0),
           ("sc", 6, I64 - 5, 0), ("sc", 7, I64, 0), ("sc", 8, 0x7FC00001, 0), f64(float("nan")),
           f64(-0.0), ("sc", 10, 1700000000, 999999999), ("sc", 11, 86400, 1), ("sc", 14, 0, 0),
           ("sc", 15, 0, 0), ("sc", 16, 0, 0), ("sc", 23, 255, 0), ("sc", 24, 0x80, 0),
           ("sc", 25, 65535, 0), ("sc", 26, 0x8000, 0)]
TEXTS = [text(n, t, n + t) for n in range(34) for t in (12, 13, 18)]
CONTAINERS = [("arr", [("sc", 6, i, 0) for i in range(k)]) for k in (0, 1, 63, 64, 65)] + [
    ("arr", [text(n, 12, n) for n in (3, 0, 17, 40)]),
    ("map", [(("sc", 6, 1, 0), text(4)), (("sc", 6, 2, 0), dec(7, 2))]),
    ("err", ("sc", 6, 9, 0)),
    ("arr", [("map", [(text(1), ("arr", [text(20), ("err", dec(1))]))]), text(3), ("arr", [])]),
    nested(32)]
UNSUB_ROW = ("sc", 0x40, 0, 0)


def pool_source():
    """Every kind of value, a row tagged NXG_TAG_UNSUBSCRIBED, and two rows that share children
    with earlier ones."""
    trees = SCALARS + TEXTS + [dec(15, 1), dec(7, 3, True), ABSTRACT] + CONTAINERS + [UNSUB_ROW]
    S = source_of(trees)
    arr = len(SCALARS) + len(TEXTS) + 3 + 3  # the 64-element array
    err = arr + 4                            # Error(Value)
    tag = np.append(S.tag, [S.tag[arr], S.tag[err]]).astype(np.uint8)
    fixed = np.append(S.fixed, [S.fixed[arr], S.fixed[err]]).astype(np.uint64)
    aux = np.append(S.aux, [S.aux[arr], S.aux[err]]).astype(np.uint32)
    return Source(tag, fixed, aux, S.ctag, S.cfixed, S.caux, S.heap)


ARCH_IDS = [0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 14) + 1, (1 << 21) - 1, 1 << 21,
            (1 << 21) + 1, (1 << 28) - 1, 1 << 28, (1 << 28) + 1, 0xFFFFFFFE]


def plain(src, n, chan_off=None, arch=None, sub=None, row=None):
    """n entries: entry e is SubId e mod the table, row e mod the batch, in one channel."""
    arch = np.asarray(ARCH_IDS if arch is None else arch, np.uint32)
    e = np.arange(n, dtype=np.uint64)
    sub = e % np.uint64(len(arch)) if sub is None else sub
    row = e % np.uint64(max(src.n_rows, 1)) if row is None else row
    return Case(src, sub, row, [0, n] if chan_off is None else chan_off, arch)


# ---- the table --------------------------------------------------------------------------------------
def cases(K=None):
    """name -> (Case, want, f64 too): `want` is what plan() must report; `f64 too`: every row is
    an F64, so the case also runs in F64 layout."""
    K = K or constants()
    B, T, W = K["block"], K["tile"], K["top"]
    F, P = f64_source(), pool_source()
    out = {}

    def add(name, case, want, f64_too=False):
        assert name not in out
        out[name] = (case, want, f64_too)

    # entry counts: one wave, one block, one tile, two tiles and the top scan's width, each +- 1
    for name, n, want in [
            ("n0", 0, dict(blocks=0, tiles=0)), ("n1", 1, dict(blocks=1, staged=1)),
            ("wave-1", 63, dict(blocks=1)), ("wave", 64, dict(blocks=1)),
            ("wave+1", 65, dict(blocks=1)),
            ("block-1", B - 1, dict(blocks=1)), ("block", B, dict(blocks=1)),
            ("block+1", B + 1, dict(blocks=2)),
            ("tile-1", T - 1, dict(tiles=1)), ("tile", T, dict(tiles=1)),
            ("tile+1", T + 1, dict(tiles=2)), ("tiles2+1", 2 * T + 1, dict(tiles=3)),
            ("top-1", (W - 1) * B, dict(blocks=W - 1, groups=1)),
            ("top", W * B, dict(blocks=W, groups=1)),
            ("top+1", (W + 1) * B, dict(blocks=W + 1, groups=2))]:
        add(name, plain(F, n), want, True)

    # channels
    n = 3 * T + 5
    edges = [0, 1, B - 1, B, B + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T, 2 * T + 1,
             2 * T + B, 3 * T, 3 * T + 1, 3 * T + 4, n]
    add("chan16_edges", plain(F, n, edges), dict(chans=16, tiles=4, empty=1), True)
    add("empty_first", plain(F, 700, [0, 0, 0, 0, 300, 700]), dict(empty=3), True)
    add("empty_middle", plain(F, 700, [0, 300, 300, 300, 300, 700]), dict(empty=3), True)
    add("empty_last", plain(F, 700, [0, 300, 700, 700, 700, 700]), dict(empty=3), True)
    add("empty_everywhere", plain(F, 0, [0] * 9), dict(empty=8, blocks=0), True)
    rng = np.random.default_rng(0x7EC)
    sizes = rng.integers(0, 4, 1000)
    off = np.concatenate([[0], np.cumsum(sizes)])
    add("chan1000", plain(P, int(off[-1]), off), dict(chans=1000, walks={"stack", "flat"}))
    add("chan1000_f64", plain(F, int(off[-1]), off), dict(chans=1000), True)

    # the filter
    none = np.full(8, NO_SLOT, np.uint32)
    add("drop_nothing", plain(F, 2 * T + 7, arch=[5] * 8), dict(dropped=0), True)
    add("drop_all", plain(F, 2 * T + 7, [0, T, 2 * T + 7], arch=none),
        dict(dropped=2 * T + 7, empty=2, idle=3), True)
    add("drop_alternating", plain(F, 2 * T + 7, [0, 9, T + 1, 2 * T + 7], arch=[3, NO_SLOT]),
        dict(dropped=T + 3), True)
    e = np.arange(3 * T, dtype=np.uint64)
    mid = (e >= T) & (e < 2 * T)
    add("drop_one_tile", plain(F, 3 * T, [0, T // 2, 3 * T], arch=[7, 200, NO_SLOT],
                               sub=np.where(mid, np.uint64(2), e % np.uint64(2)).astype(np.uint64)),
        dict(idle=1, staged=2, dropped=T), True)
    add("sub_past_table", plain(F, T + 3, arch=[9, 300],
                                sub=np.where(e[:T + 3] % 3 == 1, 2 + e[:T + 3], e[:T + 3] % 2)),
        dict(dropped=(T + 3 + 1) // 3), True)
    add("dropped_row_anything", plain(F, 200, arch=[4, NO_SLOT],
                                      row=np.where(e[:200] % 2 == 1, np.uint64(I64), e[:200])),
        dict(dropped=100), True)

    # the count varint: channels keeping 1, 127, 128, 16383 and 16384 of twice as many entries
    keepn = [1, 127, 128, 16383, 16384]
    off = np.concatenate([[0], np.cumsum([2 * k for k in keepn])])
    add("count_varint", plain(F, int(off[-1]), off, arch=[NO_SLOT, 77]),
        dict(widths={1, 2, 3}, dropped=int(off[-1]) // 2), True)

    # archive Ids of every varint width inside one tile
    add("arch_ids", plain(F, T, [0, 40, T]), dict(tiles=1, dropped=0), True)

    # values
    add("values_all", plain(P, P.n_rows, [0, 11, P.n_rows]),
        dict(walks={"scalar", "flat", "stack", "unsub"}))
    rep = np.concatenate([np.arange(P.n_rows)[::-1], np.arange(P.n_rows)[::-1],
                          np.full(70, P.n_rows - 1), np.full(70, P.n_rows - 2)]).astype(np.uint64)
    add("values_repeat_descending", plain(P, len(rep), [0, 3, len(rep) - 1, len(rep)], row=rep),
        dict(walks={"scalar", "flat", "stack", "unsub"}))
    big = source_of([f64(2.0), text(100_000, 13, 5), f64(3.0)])
    add("big_text_mid_tile", plain(big, T + 9, [0, 5, T + 9],
                                   row=np.where(e[:T + 9] == T // 2, np.uint64(1), e[:T + 9] % np.uint64(3) // np.uint64(2) * np.uint64(2))),
        dict(direct=1, staged=1))

    # Unsubscribed: span entries (the index, out of range on purpose, is not read) and rows tagged
    # NXG_TAG_UNSUBSCRIBED, first, last and as a whole channel
    unsub_row = P.n_rows - 3
    k = np.arange(600, dtype=np.uint64)
    row = k % np.uint64(20)
    row = np.where((k < 3) | (k >= 597) | ((k >= 100) & (k < 140)),
                   np.uint64(ENT_SPAN) | (k * np.uint64(0x1000000001)) | np.uint64(1 << 40), row)
    row = np.where((k == 3) | (k == 596) | ((k >= 300) & (k < 330)), np.uint64(unsub_row), row)
    add("unsubscribed", plain(P, 600, [0, 100, 140, 300, 330, 600], row=row.astype(np.uint64)),
        dict(walks={"unsub", "scalar"}, chans=5))
    return out


# ---- refusals ---------------------------------------------------------------------------------------
def _edit_tag(S, r):
    S.tag[r] = 28


def _edit_kids(S, r):  # the child range ends one past n_children
    S.aux[r] = S.n_children - int(S.fixed[r]) + 1


REFUSED_VALUES = {"tag": (text(3), _edit_tag, TAG),
                  "kids": (("arr", [f64(1.0), f64(2.0)]), _edit_kids, KIDS),
                  "depth": (nested(33), None, DEPTH),
                  "row": (f64(1.0), None, ROW)}


def refusal_cases(K=None):
    """name -> (Case, ("entry", e, cause)): the lowest of two bad kept entries carries the cause
    under test, in first, middle and last position; the other one is bad for another reason. A
    dropped entry with a bad row in front of them must not matter."""
    K = K or constants()
    T = K["tile"]
    n = 2 * T + 1
    out = {}
    for name, (v, edit, cause) in REFUSED_VALUES.items():
        other = text(3) if cause == ROW else f64(1.0)
        S = source_of([f64(0.5), v, other, ("arr", [f64(4.0)])])
        if edit:
            edit(S, 1)
        if cause == ROW:
            _edit_tag(S, 2)
        for pos, (lo, hi) in (("first", (1, n - 1)), ("middle", (n // 2, n - 1)),
                              ("last", (n - 2, n - 1))):
            row = np.zeros(n, np.uint64)
            sub = np.ones(n, np.uint64)
            row[0], sub[0] = I64 >> 1, 0  # dropped: its row is not read
            row[lo] = S.n_rows + 5 if cause == ROW else 1
            row[hi] = 2 if cause == ROW else S.n_rows
            out[f"{name}_{pos}"] = (Case(S, sub, row, [0, 7, n], [NO_SLOT, 12]),
                                    ("entry", lo, cause))
    F = f64_source(10)
    out["chan_decreases"] = (plain(F, 50, [0, 20, 10, 30, 25, 50]), ("chan", 1))
    out["chan_ends_short"] = (plain(F, 50, [0, 20, 49]), ("chan", 1))
    out["chan_past_end"] = (plain(F, 50, [0, 60, 50]), ("chan", 1))
    return out
