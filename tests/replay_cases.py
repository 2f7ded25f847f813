"""nxg_replay_window's and nxg_replay_image's case tables (tests/test_replay_cpu.py,
tests/test_gpu_replay.py).

`constants()` reads the tile size out of netidx_amd/csrc/nxg_replay.hip; `features()` computes from
it which branches a case reaches, and every case states what it is there for (`want`). A retune
then names the case that no longer sits on its edge.

A window case's rows are built from a per-row class string: 'k' kept, 'd' dropped, 'm' a miss the
table names (NXG_REPLAY_MISS), 'M' a miss by an Id at or past n_ids. The values are opaque to the
call (it copies tag / fixed / aux and rewrites Unsubscribed), so they cycle through every kind of
row: F64, Unsubscribed, text (fixed = an offset), Array (fixed = a child slot), Null, U64."""
import os
import re

import numpy as np

import replay_model as rm
from replay_model import DROP, MISS

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc",
                   "nxg_replay.hip")
VALUE_CYCLE = ((9, 0x400921FB54442D18, 0), (0x40, 0, 0), (12, 1000, 5), (19, 40, 3), (16, 0, 0),
               (3, 77, 0), (0x40, 0, 0), (12, 1 << 33, 300))


def constants():
    src = open(HIP).read()
    m = re.search(r"constexpr int RP_TILE = (\d+);", src)
    assert m, "RP_TILE not found in nxg_replay.hip"
    return dict(tile=int(m.group(1)))


class Case:
    def __init__(self, name, cols, infos, table, want, cap_rows=None, cap_miss=8):
        self.name, self.cols, self.infos, self.table = name, cols, infos, table
        self.want, self.cap_rows, self.cap_miss = want, cap_rows, cap_miss

    def expected(self):
        return rm.window_loop(self.cols, self.infos, self.table)


def pub_small(a):
    return 1000 + 7 * a


def pub_big(a):
    return (MISS - 1 - a // 2) if a % 2 else (1 << 32) + a


def window(name, recs, want, pub=pub_small, gaps=None, lead=0, tail=0, n_kept_ids=23, **kw):
    """recs: one class string per record. gaps[i]: window rows in front of record i that belong to
    no record; lead / tail rows likewise at both ends (they are misses, were they read)."""
    n_drop_ids, n_miss_ids = 5, 4
    n_ids = n_kept_ids + n_drop_ids + n_miss_ids
    table = np.array([pub(a) for a in range(n_kept_ids)] + [DROP] * n_drop_ids + [MISS] * n_miss_ids,
                     np.uint64)
    gaps = gaps or {}
    ids, infos, row = [], [], 0
    ids += [n_ids + 9] * lead
    row += lead
    seq = {"k": 0, "d": 0, "m": 0, "M": 0}
    for i, r in enumerate(recs):
        g = gaps.get(i, 0)
        ids += [n_ids + 9] * g
        row += g
        infos.append((row, len(r)))
        for c in r:
            s = seq[c]
            seq[c] += 1
            ids.append({"k": s * 5 % n_kept_ids, "d": n_kept_ids + s % n_drop_ids,
                        "m": n_kept_ids + n_drop_ids + s * 3 % n_miss_ids,
                        "M": n_ids + s % 3 * 1000}[c])
        row += len(r)
    ids += [n_ids + 9] * tail
    n = len(ids)
    vals = [VALUE_CYCLE[(j * 3 + j // 7) % len(VALUE_CYCLE)] for j in range(n)]
    cols = {"id": np.array(ids, np.uint64), "tag": np.array([v[0] for v in vals], np.uint8),
            "fixed": np.array([v[1] for v in vals], np.uint64),
            "aux": np.array([v[2] for v in vals], np.uint32)}
    return Case(name, cols, infos, table, want, **kw)


def mix(n, seed, classes="kkkd"):
    rng = np.random.RandomState(seed)
    return "".join(classes[i] for i in rng.randint(0, len(classes), n))


def cases(K=None):
    T = (K or constants())["tile"]
    out = {}

    def add(c):
        assert c.name not in out
        out[c.name] = c

    add(window("no_records", [], ["n_recs_0"]))
    add(window("no_rows", ["", "", ""], ["no_rows"]))
    add(window("empty_records_around", ["", mix(30, 1), "", "", mix(40, 2), ""],
               ["empty_front", "empty_between", "empty_behind"]))
    add(window("three_empty_at_a_tile_edge", [mix(T, 3), "", "", "", mix(T // 2, 4)],
               ["empty3_at_tile_edge", "boundary_on_tile_edge"]))
    add(window("all_kept", ["k" * 100, "k" * (T + 50)], ["all_kept"]))
    add(window("all_dropped", ["d" * 70, "d" * T], ["all_dropped"]))
    for d in (-1, 0, 1):
        add(window(f"rows_tile{d:+d}", [mix(T // 2, 5 + d), mix(T - T // 2 + d, 8 + d)],
                   [f"rows_tile{d:+d}"]))
    add(window("boundary_on_tile_edge", [mix(T, 11), mix(T, 12), mix(7, 13)],
               ["boundary_on_tile_edge"]))
    add(window("one_record_three_tiles", [mix(5, 14), mix(3 * T + 10, 15), mix(9, 16)],
               ["record_over_3_tiles"]))
    add(window("more_records_than_a_tile", [mix(i % 3, 100 + i) for i in range(T + 70)],
               ["recs_gt_tile"]))
    add(window("big_publisher_ids", [mix(300, 17), mix(300, 18)], ["pub_above_2_32",
               "pub_near_miss"], pub=pub_big))
    add(window("every_kind_kept", ["k" * 64, "k" * 64], ["unsub_kept", "array_kept", "text_kept"]))
    add(window("miss_in_record_0", [mix(50, 19) + "m" + mix(20, 20), mix(60, 21)],
               ["miss_rec0", "n_miss_below_cap"]))
    add(window("miss_in_the_last_record", [mix(50, 22), mix(60, 23), mix(10, 24) + "m"],
               ["miss_last"]))
    add(window("miss_first_row_of_a_tile", [mix(T - 3, 25), "kkk" + "m" + mix(10, 26), mix(5, 27)],
               ["miss_first_row_of_tile"]))
    # the lower record's miss in a high tile of a long record 1; record 3's in the last tile
    add(window("two_records_miss", [mix(T, 28), mix(2 * T + 100, 29) + "m" + mix(5, 30), mix(T, 31),
                                    "m" + mix(T, 32)], ["two_miss_records"]))
    add(window("miss_past_the_table", [mix(40, 33), mix(10, 34) + "M" + mix(10, 35)],
               ["miss_ge_n_ids"]))
    add(window("miss_behind_a_drop", [mix(40, 36), "kkd" + "m" + "kd", mix(10, 37)],
               ["miss_behind_drop"]))
    add(window("misses_at_cap", [mix(20, 38), "mkdM" * 2, mix(10, 39)], ["n_miss_at_cap"],
               cap_miss=4))
    add(window("misses_past_cap", [mix(20, 40), "mkMd" * 3, mix(10, 41)], ["n_miss_above_cap"],
               cap_miss=4))
    add(window("no_miss_list", [mix(20, 42), "mm", mix(10, 43)], ["n_miss_above_cap"], cap_miss=0))
    add(window("rows_of_no_record", [mix(T - 10, 44), mix(30, 45), mix(20, 46)], ["gaps", "lead"],
               gaps={1: 25, 2: T + 3}, lead=13, tail=17))
    add(window("cap_exact", [mix(T + 9, 47), mix(100, 48)], ["cap_exact"], cap_rows="exact"))
    add(window("cap_generous", [mix(T + 9, 47), mix(100, 48)], ["cap_window_rows"],
               cap_rows="window"))
    return out


def short_cases(K=None):
    """Calls whose cap_rows is one short of the kept rows: refused with n_rows = the need."""
    T = (K or constants())["tile"]
    return {
        "cap_one_short": window("cap_one_short", [mix(T + 9, 47), mix(100, 48)], ["cap_short"],
                                cap_rows="short"),
        "cap_zero": window("cap_zero", [mix(20, 49)], ["cap_short"], cap_rows=0),
        "cap_short_and_stopped": window("cap_short_and_stopped", [mix(T, 50), mix(9, 51) + "m"],
                                        ["cap_short", "miss_last"], cap_rows="short"),
    }


def cap_rows_of(case, want):
    c = case.cap_rows
    return {None: len(case.cols["id"]), "window": len(case.cols["id"]), "exact": want.n_rows,
            "short": want.n_rows - 1}.get(c, c)


def features(case, K=None):
    """The names of the branches a window case reaches."""
    T = (K or constants())["tile"]
    infos, cols, table = case.infos, case.cols, case.table
    n_recs = len(infos)
    f = set()
    if n_recs == 0:
        return {"n_recs_0"}
    first, end = infos[0][0], infos[-1][0] + infos[-1][1]
    n = end - first
    if n == 0:
        f.add("no_rows")
        return f
    cnt = [c for _, c in infos]
    nz = [i for i, c in enumerate(cnt) if c]
    if cnt[0] == 0:
        f.add("empty_front")
    if cnt[-1] == 0:
        f.add("empty_behind")
    if any(c == 0 for c in cnt[nz[0]:nz[-1]]):
        f.add("empty_between")
    for i in range(1, n_recs - 3):
        if cnt[i:i + 3] == [0, 0, 0] and (infos[i][0] - first) % T == 0 and infos[i][0] > first:
            f.add("empty3_at_tile_edge")
    for i in nz[1:]:
        if (infos[i][0] - first) % T == 0:
            f.add("boundary_on_tile_edge")
    for o, c in infos:
        if c and (o + c - 1 - first) // T - (o - first) // T >= 2:
            f.add("record_over_3_tiles")
    if n_recs > T:
        f.add("recs_gt_tile")
    for d in (-1, 0, 1):
        if n == T + d:
            f.add(f"rows_tile{d:+d}")
    in_rec = np.zeros(len(cols["id"]), bool)
    rec_of = np.full(len(cols["id"]), -1)
    for i, (o, c) in enumerate(infos):
        in_rec[o:o + c] = True
        rec_of[o:o + c] = i
    if first > 0:
        f.add("lead")
    if not in_rec[first:end].all():
        f.add("gaps")
    p = rm._lookup(cols["id"], table)
    miss, drop = (p == np.uint64(MISS)) & in_rec, (p == np.uint64(DROP)) & in_rec
    kept = in_rec & ~miss & ~drop
    if kept[in_rec].all():
        f.add("all_kept")
    if drop[in_rec].all():
        f.add("all_dropped")
    want = case.expected()
    pubs = want.rows["id"]
    if (pubs >= np.uint64(1 << 32)).any():
        f.add("pub_above_2_32")
    if (pubs == np.uint64(MISS - 1)).any():
        f.add("pub_near_miss")
    src = want.rows["src_row"].astype(np.int64)
    for name, tag in (("unsub_kept", 0x40), ("array_kept", 19), ("text_kept", 12)):
        if (cols["tag"][src] == tag).any():
            f.add(name)
    mrec = sorted(set(rec_of[miss].tolist()))
    if mrec:
        if mrec[0] == 0:
            f.add("miss_rec0")
        if mrec[0] == n_recs - 1:
            f.add("miss_last")
        mrows = np.flatnonzero(miss & (rec_of == mrec[0]))
        if any((r - first) % T == 0 and r > first for r in mrows.tolist()):
            f.add("miss_first_row_of_tile")
        tiles = {(int(np.flatnonzero(miss & (rec_of == m))[0]) - first) // T for m in mrec}
        if len(mrec) >= 2 and len(tiles) >= 2:
            f.add("two_miss_records")
        if (cols["id"][mrows] >= np.uint64(len(table))).any():
            f.add("miss_ge_n_ids")
        o = infos[mrec[0]][0]
        if any(drop[o:r].any() for r in mrows.tolist()):
            f.add("miss_behind_drop")
        k = want.n_miss
        f.add("n_miss_below_cap" if k < case.cap_miss else
              "n_miss_at_cap" if k == case.cap_miss else "n_miss_above_cap")
    cap = cap_rows_of(case, want)
    if case.cap_rows is not None:
        f.add("cap_exact" if cap == want.n_rows and case.cap_rows == "exact" else
              "cap_short" if cap < want.n_rows else "cap_window_rows")
    return f


# ---- the image ------------------------------------------------------------------------------------
class ImageCase:
    def __init__(self, name, image, order, table, want, cap_rows=None, cap_miss=8):
        self.name, self.image, self.order, self.table = name, image, order, table
        self.want, self.cap_rows, self.cap_miss = want, cap_rows, cap_miss

    def expected(self):
        return rm.image_loop(self.image, self.order, self.table)


def image_of(ids):
    """An image (ids ascending) whose values cycle through the kinds."""
    ids = np.array(sorted(ids), np.uint64)
    vals = [VALUE_CYCLE[(j * 5 + 1) % len(VALUE_CYCLE)] for j in range(len(ids))]
    return {"id": ids, "tag": np.array([v[0] for v in vals], np.uint8),
            "fixed": np.array([v[1] for v in vals], np.uint64),
            "aux": np.array([v[2] for v in vals], np.uint32)}


def image_cases(K=None):
    T = (K or constants())["tile"]
    n_ids = 400
    table = np.array([pub_small(a) if a % 11 else (DROP if a % 22 else MISS) for a in range(n_ids)],
                     np.uint64)
    every = image_of(range(0, n_ids, 1))
    sparse = image_of(range(3, n_ids, 4))
    rng = np.random.RandomState(7)
    out = {}

    def add(name, image, order, want, **kw):
        out[name] = ImageCase(name, image, np.asarray(order, np.uint32), table, want, **kw)

    add("empty_image", image_of([]), np.arange(1, 60), ["empty_image", "absent"])
    add("empty_order", every, [], ["n_order_0"])
    add("absent_ids", sparse, np.arange(1, 300), ["absent", "present"])
    add("unsubscribed_in_the_image", every, np.arange(1, 200), ["unsub_in_image", "present"])
    add("unsorted_order", sparse, rng.permutation(n_ids), ["unsorted", "misses", "drops"])
    add("duplicates", sparse, rng.randint(0, 40, 300), ["duplicates"])
    add("ids_past_the_table", sparse, [5, n_ids, 7, n_ids + 1000, 3, 0xFFFFFFFF],
        ["order_ge_n_ids", "misses"])
    add("misses_past_cap", every, np.arange(0, n_ids), ["misses_above_cap"], cap_miss=3)
    for d in (-1, 0, 1):
        add(f"order_tile{d:+d}", sparse, rng.randint(0, n_ids, T + d), [f"order_tile{d:+d}"])
    add("order_three_tiles", sparse, rng.randint(0, n_ids + 20, 2 * T + 77), ["order_3_tiles"])
    add("cap_exact", sparse, rng.randint(0, n_ids, 200), ["cap_exact"], cap_rows="exact")
    return out


def image_features(case, K=None):
    T = (K or constants())["tile"]
    f = set()
    order, image, table = case.order.astype(np.uint64), case.image, case.table
    n = len(order)
    if n == 0:
        return {"n_order_0"}
    if len(image["id"]) == 0:
        f.add("empty_image")
    want = case.expected()
    src = want.rows["src_row"]
    kept_ids = order[(rm._lookup(order, table) < np.uint64(MISS))]
    in_img = np.isin(kept_ids, image["id"])
    if (~in_img).any():
        f.add("absent")
    if (src != np.uint64(rm.U64_MAX)).any():
        f.add("present")
    if (in_img & (src == np.uint64(rm.U64_MAX))).any():
        f.add("unsub_in_image")
    if (np.diff(order.astype(np.int64)) < 0).any():
        f.add("unsorted")
    if len(np.unique(order)) < n:
        f.add("duplicates")
    if (order >= np.uint64(len(table))).any():
        f.add("order_ge_n_ids")
    if want.n_miss:
        f.add("misses")
    if want.n_miss > case.cap_miss:
        f.add("misses_above_cap")
    if want.n_dropped:
        f.add("drops")
    for d in (-1, 0, 1):
        if n == T + d:
            f.add(f"order_tile{d:+d}")
    if (n + T - 1) // T >= 3:
        f.add("order_3_tiles")
    if case.cap_rows == "exact":
        f.add("cap_exact")
    return f
