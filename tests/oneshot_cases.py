"""The case tables of nxg_oneshot_pack_pathmap and nxg_oneshot_pack_deltas
(tests/test_oneshot_cpu.py, tests/test_gpu_oneshot.py).

`constants()` reads the kernels' constants out of netidx_amd/csrc/nxg_oneshot.hip; `pathmap_plan()`
and `deltas_plan()` compute from them which branches a case reaches, and every case states what it
is there for (`want`). A retune then names the case that no longer sits on its edge.
"""
import os
import re

import numpy as np

import oneshot_model as om
import record_cases as rc
import record_model as rm
from record_cases import reaches, text  # noqa: F401  (re-exported)
from value_table_cases import f64, nested, source_of

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc",
                   "nxg_oneshot.hip")


def constants():
    src = open(HIP).read()

    def const(name):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m, f"{name} not found in nxg_oneshot.hip"
        return int(m.group(1))

    return dict(pm_block=const("OS_PM_IDS_PER_BLOCK"), pm_tile=const("OS_PM_IDS_PER_TILE"),
                pm_staging=const("OS_PM_STAGING_BYTES"), pm_top=const("OS_PM_TOP_WIDTH"),
                long_path=const("OS_PM_LONG_PATH"),
                block=const("OS_DL_ROWS_PER_BLOCK"), tile=const("OS_DL_ROWS_PER_TILE"),
                staging=const("OS_DL_STAGING_BYTES"), top=const("OS_DL_TOP_WIDTH"))


def _vl(v):
    return 1 + sum(v >= (1 << s) for s in (7, 14, 21, 28, 35, 42, 49, 56, 63))


# ---- the pathmap: the branches a case reaches ---------------------------------------------------------
def pathmap_plan(paths, K=None):
    """blocks, groups (of the top scan), tiles; tiles staged in LDS / written straight to the
    output (a long path, or more bytes than the staging) / with nothing selected; paths copied by
    a wave; the widths of the Id, length and count varints; kept Ids without a path."""
    K = K or constants()
    n = paths.n_ids
    plen = np.array([len(p) for p in paths.paths], np.int64)
    sel = (paths.keep != 0) & (plen > 0)
    lens = np.array([_vl(a) + _vl(int(plen[a])) + int(plen[a]) if sel[a] else 0
                     for a in range(n)], np.int64) if n <= 1 << 18 else None
    T, L = K["pm_tile"], K["long_path"]
    staged = direct = idle = 0
    ids = np.flatnonzero(sel)
    if lens is not None:
        for t0 in range(0, n, T):
            s = sel[t0:t0 + T]
            if not s.any():
                idle += 1
            elif (plen[t0:t0 + T][s] >= L).any() or int(lens[t0:t0 + T].sum()) > K["pm_staging"]:
                direct += 1
            else:
                staged += 1
    blocks = -(-n // K["pm_block"])
    return dict(blocks=blocks, groups=-(-blocks // K["pm_top"]), tiles=-(-n // T), staged=staged,
                direct=direct, idle=idle, long=int((plen[ids] >= L).sum()),
                id_widths={_vl(int(a)) for a in ids}, len_widths={_vl(int(x)) for x in plen[ids]},
                count_width=_vl(len(ids)), n_sel=len(ids),
                pathless=int(((paths.keep != 0) & (plen == 0)).sum()),
                lens={int(x) for x in plen[ids]})


def path(n, seed=0):
    """An n-byte path: '/' and printable ASCII."""
    return b"/" + bytes(97 + (seed + 3 * i) % 26 for i in range(n - 1)) if n else b""


def short_paths(n, keep=None):
    """Paths of 6 to 15 bytes for Ids [0, n)."""
    ps = [path(6 + a % 10, a) for a in range(n)]
    return om.Paths(ps, np.ones(n, np.uint8) if keep is None else keep)


def pathmap_cases(K=None):
    """name -> (Paths, want)."""
    K = K or constants()
    B, T, W, L = K["pm_block"], K["pm_tile"], K["pm_top"], K["long_path"]
    out = {}

    def add(name, paths, want):
        assert name not in out
        out[name] = (paths, want)

    for name, n, want in [
            ("n0", 0, dict(blocks=0, n_sel=0)), ("n1", 1, dict(blocks=1, staged=1)),
            ("n64", 64, dict(blocks=1)), ("n65", 65, dict(blocks=1)),
            ("block-1", B - 1, dict(blocks=1)), ("block", B, dict(blocks=1)),
            ("block+1", B + 1, dict(blocks=2)),
            ("tile+1", T + 1, dict(tiles=2)), ("tiles2+1", 2 * T + 1, dict(tiles=3)),
            ("top-1", (W - 1) * B, dict(blocks=W - 1, groups=1)),
            ("top", W * B, dict(blocks=W, groups=1)),
            ("top+1", (W + 1) * B, dict(blocks=W + 1, groups=2, id_widths={1, 2, 3}))]:
        add(name, short_paths(n), want)
    n = 2 * T + 9
    a = np.arange(n)
    add("keep_none", short_paths(n, np.zeros(n, np.uint8)), dict(n_sel=0, idle=3))
    add("keep_all", short_paths(n), dict(n_sel=n, idle=0))
    add("keep_alternate", short_paths(n, (a % 2).astype(np.uint8)), dict(n_sel=n // 2))
    add("keep_one_tile_none", short_paths(3 * T, ((np.arange(3 * T) // T) != 1).astype(np.uint8)),
        dict(idle=1, staged=2))
    ps = [path(6 + i % 10, i) if i % 3 else b"" for i in range(n)]
    add("kept_without_path", om.Paths(ps, np.where(a % 5 == 0, 0, 7).astype(np.uint8)),
        dict(pathless=int(((a % 3 == 0) & (a % 5 != 0)).sum())))
    # path lengths: the length varint's width, and the long-path threshold, one tile each
    for ln in (1, 127, 128, L - 1, L, L + 1):
        ps = [path(7, i) for i in range(T)]
        ps[T // 2] = path(ln, 5)
        want = dict(lens={ln}, long=int(ln >= L), direct=int(ln >= L), staged=int(ln < L))
        add(f"len{ln}", om.Paths(ps, np.ones(T, np.uint8)), want)
    # a path across tiles of the output, first / middle / last of its wave, and two in one wave
    for name, at in (("long_first", [64]), ("long_mid", [100]), ("long_last", [127]),
                     ("long_two", [70, 71]), ("long_tile_ends", [0, T - 1])):
        ps = [path(9, i) for i in range(T + 3)]
        for k, i in enumerate(at):
            ps[i] = path(5000 + 17 * k, i)
        add(name, om.Paths(ps, np.ones(T + 3, np.uint8)), dict(long=len(at), direct=1, staged=1))
    ps = [path(8, i) for i in range(2 * T)]
    for i in range(40, 104):
        ps[i] = path(200, i)
    add("paths200x64", om.Paths(ps, np.ones(2 * T, np.uint8)), dict(long=0, staged=2))
    ps = [path(200, i) for i in range(T)]
    add("paths200_over_staging", om.Paths(ps, np.ones(T, np.uint8)), dict(long=0, direct=1))
    # the count varint
    for k in (127, 128):
        keep = np.zeros(3 * k, np.uint8)
        keep[::3] = 1
        add(f"n_sel{k}", short_paths(3 * k, keep), dict(n_sel=k, count_width=_vl(k)))
    # Ids across 2^7 and 2^14 in one tile each, and 2^21 (sparse: most Ids have no path)
    n = (1 << 14) + 40
    keep = np.zeros(n, np.uint8)
    keep[[100, 127, 128, 129, (1 << 14) - 1, 1 << 14, (1 << 14) + 1]] = 1
    add("ids_2^7_2^14", short_paths(n, keep), dict(id_widths={1, 2, 3}, n_sel=7))
    n = (1 << 21) + 300
    ps = [b""] * n
    keep = np.zeros(n, np.uint8)
    for i in (5, (1 << 21) - 2, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, n - 1):
        ps[i] = path(11, i)
        keep[i] = 1
    keep[77] = 1  # (no path)
    add("ids_2^21", om.Paths(ps, keep), dict(id_widths={1, 3, 4}, n_sel=6, pathless=1,
                                            groups=-(-(-(-n // B)) // W)))
    return out


def pathmap_refusal_cases():
    """name -> (Paths-like with a raw path_off, the Id the message names)."""
    out = {}
    for name, (lo, hi) in (("first", (0, 699)), ("middle", (300, 301)), ("last", (698, 699))):
        p = short_paths(700)
        off = p.path_off().astype(np.int64) + 10  # (path_off[0] need not be 0)
        for a in (lo, hi):  # path_off[a + 1] = path_off[a] - 1
            off[a + 1:] -= 1 + (off[a + 1] - off[a])
        assert off.min() >= 0
        out[f"decreases_{name}"] = (p, off.astype(np.uint64), lo)
    return out


# ---- the deltas: the branches a case reaches ----------------------------------------------------------
def deltas_plan(win, K=None):
    """Over the rows [first, first + n) the records span: blocks, groups, tiles; tiles staged /
    written straight to the output / with nothing kept; the walks of the kept rows; the widths of
    the count and Id varints; rows dropped; records without an element; rows between records."""
    K = K or constants()
    case = win.as_record_case()
    rows, off = win.rows()
    kept, _ = case.keep()
    lens_e = rm.item_lens(case)
    first = win.recs[0][0] if win.recs else 0
    n = (win.recs[-1][0] + win.recs[-1][1] - first) if win.recs else 0
    lens = np.zeros(n, np.int64)
    lens[rows - first] = lens_e
    keptr = np.zeros(n, bool)
    keptr[rows - first] = kept
    widths, empty = set(), 0
    for i in range(win.n_recs):
        idx = np.flatnonzero(kept[off[i]:off[i + 1]])
        if len(idx):
            lens[rows[off[i] + idx[0]] - first] += 12 + _vl(len(idx))
            widths.add(_vl(len(idx)))
        else:
            empty += 1
    staged = direct = idle = 0
    T = K["tile"]
    bounds = [0] * (-(-n // T))
    for a, m in win.recs:
        if m and (a - first) % T:
            bounds[(a - first) // T] += 1
    for t0 in range(0, n, T):
        if not keptr[t0:t0 + T].any():
            idle += 1
        elif int(lens[t0:t0 + T].sum()) > K["staging"]:
            direct += 1
        else:
            staged += 1
    walks = {rc.row_walk(win.src, int(r)) for r in np.unique(rows[kept])}
    blocks = -(-n // K["block"])
    spans = max([(a + m - 1 - first) // T - (a - first) // T + 1 for a, m in win.recs if m] + [0])
    return dict(blocks=blocks, groups=-(-blocks // K["top"]), tiles=-(-n // T), staged=staged,
                direct=direct, idle=idle, walks=walks, widths=widths,
                id_widths={_vl(int(a)) for a in win.ids[rows[kept]]},
                dropped=int((~kept).sum()), empty=empty, recs=win.n_recs,
                gap_rows=n - len(rows), max_bounds_in_tile=max(bounds + [0]),
                max_tiles_of_a_record=spans, items={int(kept[off[i]:off[i + 1]].sum())
                                                    for i in range(win.n_recs)})


SECS = [0, 1, -1, 1_700_000_000, -(1 << 63), (1 << 63) - 1, -62135596800]
NANOS = [0, 999_999_999, 1_999_999_999, 1_000_000_000, 0xFFFFFFFF, 5]


def window(src, recs, ids=None, n_ids=None, selected=None):
    """A Window over src: ids default to row mod 200, every Id selected."""
    n = src.n_rows
    ids = np.arange(n, dtype=np.uint64) % np.uint64(200) if ids is None else np.asarray(ids, np.uint64)
    n_ids = int(ids.max()) + 1 if n_ids is None and n else (n_ids or 0)
    sel = set(int(a) for a in np.unique(ids) if a < n_ids) if selected is None else selected
    k = len(recs)
    wrap = lambda v: (v + (1 << 63)) % (1 << 64) - (1 << 63)  # noqa: E731  (an i64)
    return om.Window(src, ids, recs, [wrap(SECS[i % len(SECS)] + i) for i in range(k)],
                     [NANOS[i % len(NANOS)] for i in range(k)], n_ids, sel)


def split(n, edges):
    """Records covering [0, n) with boundaries at `edges`."""
    e = [0] + list(edges) + [n]
    return [(e[i], e[i + 1] - e[i]) for i in range(len(e) - 1)]


def deltas_cases(K=None):
    """name -> (Window, want)."""
    K = K or constants()
    B, T, W = K["block"], K["tile"], K["top"]
    P = rc.pool_source()
    out = {}

    def add(name, win, want):
        assert name not in out
        out[name] = (win, want)

    def F(n):
        return source_of([f64(0.25 * i - 3) for i in range(n)])

    for name, n, want in [
            ("n1", 1, dict(blocks=1, staged=1)), ("wave-1", 63, dict(blocks=1)),
            ("wave", 64, dict(blocks=1)), ("wave+1", 65, dict(blocks=1)),
            ("block-1", B - 1, dict(blocks=1)), ("block", B, dict(blocks=1)),
            ("block+1", B + 1, dict(blocks=2)),
            ("tile-1", T - 1, dict(tiles=1)), ("tile", T, dict(tiles=1)),
            ("tile+1", T + 1, dict(tiles=2)),
            ("top-1", (W - 1) * B, dict(blocks=W - 1, groups=1)),
            ("top", W * B, dict(blocks=W, groups=1)),
            ("top+1", (W + 1) * B, dict(blocks=W + 1, groups=2))]:
        add(name, window(F(n), split(n, [n // 3])), want)
    add("no_records", window(F(10), []), dict(recs=0, blocks=0))
    add("records_of_0_rows", window(F(700), [(0, 0), (0, 300), (300, 0), (300, 0), (300, 400),
                                             (700, 0)]), dict(recs=6, empty=4))
    # runs of records that keep nothing: Ids 0..99 selected, the runs carry Ids 100..199
    n = 3 * T
    r = np.arange(n, dtype=np.uint64)

    def runs(quiet):
        ids = np.where(quiet, np.uint64(100), np.uint64(0)) + r % np.uint64(100)
        return window(F(n), split(n, range(50, n, 50)), ids, 200, set(range(100)))

    add("nothing_kept_at_start", runs(r < 200), dict(empty=4, dropped=200))
    add("nothing_kept_in_middle", runs((r >= T - 50) & (r < 2 * T + 50)),
        dict(empty=(T + 100) // 50 - 1, idle=1))
    add("nothing_kept_at_end", runs(r >= n - 150), dict(empty=3, dropped=150))
    add("a_tile_keeps_nothing", runs((r >= T) & (r < 2 * T)), dict(idle=1, staged=2))
    add("keeps_nothing_at_all", window(F(n), split(n, [T]), None, 200, set()),
        dict(idle=3, empty=2, dropped=n))
    recs = split(600, [100, 200, 300, 400, 500])
    first_of = np.array([a for a, _ in recs])
    ids = np.full(600, 150, np.uint64)
    ids[first_of] = 3
    add("only_first_row_kept", window(F(600), recs, ids, 200, {3}), dict(items={1}, dropped=594))
    ids = np.full(600, 150, np.uint64)
    ids[first_of + 99] = 3
    add("only_last_row_kept", window(F(600), recs, ids, 200, {3}), dict(items={1}, dropped=594))
    add("three_bounds_in_a_tile", window(F(2 * T), split(2 * T, [T + 10, T + 20, T + 30])),
        dict(max_bounds_in_tile=3))
    add("record_spans_three_tiles", window(F(4 * T), split(4 * T, [T - 5, 3 * T + 5])),
        dict(max_tiles_of_a_record=4))
    add("rows_between_records", window(F(900), [(10, 90), (100, 0), (130, 300), (T + 7, 200)]),
        dict(gap_rows=T + 197 - 590, recs=4))
    add("recs1000x3", window(F(3000), split(3000, range(3, 3000, 3))),
        dict(recs=1000, items={3}))
    rng = np.random.default_rng(0x51)
    sizes = rng.integers(0, 4, 1000)
    edges = np.cumsum(sizes)[:-1]
    tot = int(sizes.sum())
    add("recs1000_values", window(_repeat(P, tot), split(tot, edges)),
        dict(recs=1000, walks={"stack", "flat", "scalar", "unsub"}))
    # the count varint's width: 127 and 128 kept of twice as many rows
    ids = np.tile(np.array([5, 150], np.uint64), 255)
    add("count_127_128", window(F(510), [(0, 254), (254, 256)], ids, 200, {5}),
        dict(items={127, 128}, widths={1, 2}))
    # Ids of each varint width, and at the edge of n_ids
    wide = [0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28,
            (1 << 28) + 5]
    ids = np.array(wide * 6, np.uint64)
    add("id_widths", window(F(60), split(60, [7, 30]), ids, (1 << 28) + 6, set(wide)),
        dict(id_widths={1, 2, 3, 4, 5}, dropped=0))
    ids = np.array([198, 199, 200, 201, 1 << 40, (1 << 64) - 1] * 10, np.uint64)
    add("id_at_n_ids", window(F(60), split(60, [31]), ids, 200, {198, 199}),
        dict(dropped=40, id_widths={2}))
    # values
    add("values_all", window(P, split(P.n_rows, [11])),
        dict(walks={"scalar", "flat", "stack", "unsub"}))
    big = source_of([f64(2.0), text(100_000, 13, 5), f64(3.0)])
    rows = np.where(np.arange(T + 9) == T // 2, 1, (np.arange(T + 9) % 3) // 2 * 2)
    add("big_text_mid_tile", window(_gather(big, rows), split(T + 9, [5])),
        dict(direct=1, staged=1))
    return out


def _gather(S, rows):
    """A Source whose row i is S's row rows[i] (children and heap shared)."""
    from value_table_model import Source
    rows = np.asarray(rows, np.int64)
    return Source(S.tag[rows].copy(), S.fixed[rows].copy(), S.aux[rows].copy(), S.ctag, S.cfixed,
                  S.caux, S.heap)


def _repeat(S, n):
    return _gather(S, np.arange(n) % S.n_rows)


# ---- refusals -----------------------------------------------------------------------------------------
def deltas_refusal_cases(K=None):
    """name -> (Window, ("row", r, cause)): the lowest of two bad kept rows carries the cause
    under test, in first, middle and last position; the other is bad for another reason. A dropped
    row with a bad tag in front of them must not matter."""
    K = K or constants()
    T = K["tile"]
    n = 2 * T + 1
    out = {}
    for name, (v, edit, cause) in rc.REFUSED_VALUES.items():
        if cause == rm.ROW:
            continue
        S0 = source_of([f64(0.5), v, text(3), ("arr", [f64(4.0)])])
        if edit:
            edit(S0, 1)
        rc._edit_tag(S0, 2)
        for pos, (lo, hi) in (("first", (1, n - 1)), ("middle", (n // 2, n - 1)),
                              ("last", (n - 2, n - 1))):
            rows = np.zeros(n, np.int64)
            rows[0] = 2        # a bad tag, dropped: nothing of it is read
            rows[lo] = 1
            rows[hi] = 2 if cause != rm.TAG else 3
            S = _gather(S0, rows)
            if cause == rm.TAG:  # the other offender: a child range outside n_children
                S.aux[hi] = S.n_children + 1
            ids = np.full(n, 12, np.uint64)
            ids[0] = 150
            out[f"{name}_{pos}"] = (window(S, split(n, [7]), ids, 100, {12}), ("row", lo, cause))
    # size guards (PackError::TooBig), each checked before anything the count or length would
    # reach is read: an Array of MAX_VEC / 16 + 1 elements (sized in registers), a Map of MAX_VEC /
    # 32 + 1 pairs (the stack walk), and an item of 2^32 bytes or more (a Bytes value whose length
    # says so). The other offender has an unknown tag.
    B0 = source_of([f64(0.5), ("arr", [f64(1.0)]), text(3), ("map", [(f64(1.0), f64(2.0))]),
                    text(5, 13)])
    rc._edit_tag(B0, 2)
    B0.aux[1] = rm.MAX_VEC // 16 + 1
    B0.aux[3] = rm.MAX_VEC // 32 + 1
    B0.aux[4] = 0xFFFFFFFF
    for name, bad, places in (("big_array", 1, ("first", "middle", "last")),
                              ("big_map", 3, ("first", "middle", "last")),
                              ("big_item", 4, ("middle",))):
        for pos, (lo, hi) in (("first", (1, n - 1)), ("middle", (n // 2, n - 1)),
                              ("last", (n - 2, n - 1))):
            if pos not in places:
                continue
            rows = np.zeros(n, np.int64)
            rows[0] = bad      # dropped: nothing of it is read
            rows[lo] = bad
            rows[hi] = 2
            ids = np.full(n, 12, np.uint64)
            ids[0] = 150
            out[f"{name}_{pos}"] = (window(_gather(B0, rows), split(n, [7]), ids, 100, {12}),
                                    ("row", lo, rm.BIG))
    S = _gather(source_of([f64(1.0), ("arr", [f64(4.0)])]), [0, 1, 0, 1])
    S = type(S)(S.tag, S.fixed, S.aux, None, None, None, S.heap)
    out["nokids"] = (window(S, split(4, [2]), np.full(4, 3, np.uint64), 10, {3}),
                     ("row", 1, rm.NOKIDS))
    return out


assert nested  # (value_table_cases.nested builds REFUSED_VALUES' depth case)
