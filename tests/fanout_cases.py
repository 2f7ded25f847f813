"""Inputs that sit on the thresholds the fan-out kernels branch on (test infrastructure).

The dispatch (netidx_amd/csrc/nxg_dispatch.hip, under nxg_dispatch_updates, nxg_publish_commit,
nxg_publish_unsubscribes and nxg_route_writes) and the commit's repeated-Id check and radix sort
(nxg_publish.hip) choose their paths from a handful of constants: the segment length and its
doubling, the scan's block and top-level sizes, the LDS-counter bound, the row cache's two
encodings, the streams a row holds in registers, the bounded grid of the repeated-Id check, the
radix digit count. `plan()` and `pub_plan()` restate those choices from the constants READ FROM
THE KERNEL SOURCES, so a retune makes tests/test_fanout_cases_cpu.py say which case no longer
reaches its branch. Every case is deterministic and built with numpy (no Python loop over rows).

  constants()               the constants, by regex; one that is not found raises RuntimeError
  plan(n_rows, n_chans)     seg_rows, n_seg, M, nb, lds, fused, cache, ...
  pub_plan(n, n_slots, cus) grid, stride, radix passes of the commit
  dispatch_case(name)       a DispatchCase (DISPATCH_CASES lists the names)
  commit_case(name, cus)    a CommitCase (COMMIT_CASES lists the names)
  unsubscribe_case(n_clients)
  prefix(case, n)           the first n rows of a case on the same table
"""
import functools
import os
import random
import re
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "netidx_amd", "csrc")
NO_SLOT = 0xFFFFFFFF
U64_MAX = 2 ** 64 - 1
PUB_UPDATE, PUB_UPDATE_CHANGED, PUB_UPDATE_CLIENT = 0, 1, 2
STEP = 64  # rows per step: one wave

_INT = r"(0x[0-9a-fA-F]+|\d+)"
_PATTERNS = {
    "nxg_dispatch.hip": {
        "NXG_DISP_SEG": r"#define\s+NXG_DISP_SEG\s+" + _INT,
        "NXG_DISP_U": r"#define\s+NXG_DISP_U\s+" + _INT,
        "NXG_DISP_CACHE": r"#define\s+NXG_DISP_CACHE\s+" + _INT,
        "NXG_DISP_FUSE": r"#define\s+NXG_DISP_FUSE\s+" + _INT,
        "NXG_DISP_NARROW": r"#define\s+NXG_DISP_NARROW\s+" + _INT,
        "TPB": r"constexpr\s+int\s+TPB\s*=\s*" + _INT + r"\s*;",
        "LCH": r"constexpr\s+uint32_t\s+LCH\s*=\s*" + _INT + r"\s*;",
        "SCAN_K": r"constexpr\s+int\s+SCAN_K\s*=\s*" + _INT + r"\s*;",
        "RF": r"constexpr\s+uint32_t\s+RF\s*=\s*" + _INT + r"\s*;",
        "MAX_M_LOG2": r"constexpr\s+uint64_t\s+MAX_M\s*=\s*1ull\s*<<\s*" + _INT + r"\s*;",
        "kLookup": r"\bkLookup\s*=\s*" + _INT,
        "kNoChan": r"\bkNoChan\s*=\s*" + _INT,
        # RowCache rc{..., NXG_DISP_NARROW && tb.n_chans < 0xfeu}
        "NARROW_BOUND": r"NXG_DISP_NARROW\s*&&\s*tb\.n_chans\s*<\s*" + _INT + r"u?\s*\}",
        # the top scan's workgroup: the block totals one round takes
        "TOP": r"__launch_bounds__\(" + _INT + r"\)\s*void\s+nxg_disp_scan_top_kernel",
        "TOP_CHAN": r"__launch_bounds__\(" + _INT + r"\)\s*void\s+nxg_disp_scan_top_chan_kernel",
    },
    "nxg_publish.hip": {
        "PUB_TPB": r"constexpr\s+int\s+TPB\s*=\s*" + _INT + r"\s*;",
        "PUB_SEG": r"constexpr\s+uint32_t\s+SEG\s*=\s*" + _INT + r"\s*;",
        "PUB_BINS": r"constexpr\s+uint32_t\s+BINS\s*=\s*" + _INT + r"\s*;",
        "NXG_PUB_GCAP": r"#define\s+NXG_PUB_GCAP\s+" + _INT,
        "PUB_HEADS": r"__popcll\(heads\)\s*<=\s*" + _INT,
    },
}
# statements plan() restates: if one of them changes shape, plan() has to be read against it again
_SHAPES = {
    "nxg_dispatch.hip": {
        "segment doubling": r"while\s*\(\(\(n \+ seg - 1\) / seg\) \* ch > MAX_M\)\s*seg \*= 2;",
        "wide cache bound": r"NXG_DISP_CACHE\s*&&\s*tb\.n_chans\s*<\s*kLookup\)",
        "fused top scan": r"fuse = NXG_DISP_FUSE && M != 0 && tb\.n_chans <= LCH;",
        "LDS counters": r"lds = tb\.n_chans <= LCH;",
        "step group": r"b0 \+= 64 \* DU\)",
    },
    "nxg_publish.hip": {
        "radix passes": r"for \(uint32_t shift = 0; shift < bits; shift \+= 8\)",
        "key bits": r"while \(bits < 32 && \(1ull << bits\) <= tb\.n_slots\) bits\+\+;",
        "bounded grid": r"\(uint64_t\)ncu \* NXG_PUB_GCAP\)",
    },
}


@functools.lru_cache(maxsize=None)
def constants():
    """The kernels' constants, read from their sources. A constant or a restated statement that
    is not found is an error: the cases below would otherwise stop straddling a threshold
    without any test saying so."""
    out, missing = {}, []
    for fname, pats in _PATTERNS.items():
        with open(os.path.join(CSRC, fname)) as f:
            src = f.read()
        for name, pat in pats.items():
            m = re.search(pat, src)
            if m is None:
                missing.append(f"{fname}: {name} (/{pat}/)")
            else:
                out[name] = int(m.group(1), 0)
        for name, pat in _SHAPES[fname].items():
            if re.search(pat, src) is None:
                missing.append(f"{fname}: the {name} statement (/{pat}/)")
    if missing:
        raise RuntimeError("tests/fanout_cases.py restates these from the kernel sources and no "
                           "longer finds them; re-read plan() against the kernels:\n  " +
                           "\n  ".join(missing))
    out["MAX_M"] = 1 << out.pop("MAX_M_LOG2")
    out["SCAN_B"] = out["TPB"] * out["SCAN_K"]
    return types.MappingProxyType(out)


def _cdiv(a, b):
    return (a + b - 1) // b


def plan(n_rows, n_chans):
    """What nxg_launch_dispatch does with n_rows rows on n_chans channels (nxg_disp_seg_rows and
    the launch code, restated)."""
    k = constants()
    seg = k["NXG_DISP_SEG"]
    ch = n_chans if n_chans else 1
    while _cdiv(n_rows, seg) * ch > k["MAX_M"]:
        seg *= 2
    n_seg = _cdiv(n_rows, seg)
    M = n_seg * n_chans
    nb = _cdiv(M, k["SCAN_B"])
    lds = n_chans <= k["LCH"]
    fused = bool(k["NXG_DISP_FUSE"]) and M != 0 and lds
    if not k["NXG_DISP_CACHE"] or n_chans >= k["kLookup"]:
        cache = "none"
    elif k["NXG_DISP_NARROW"] and n_chans < k["NARROW_BOUND"]:
        cache = "narrow"
    else:
        cache = "wide"
    top = k["TOP_CHAN"] if fused else k["TOP"]
    return {"seg_rows": seg, "n_seg": n_seg, "M": M, "nb": nb, "lds": lds, "fused": fused,
            "cache": cache, "group": STEP * k["NXG_DISP_U"],
            "iterations": _cdiv(min(seg, max(n_rows, 1)), STEP * k["NXG_DISP_U"]),
            "top_rounds": _cdiv(nb, top)}


def pub_plan(n_rows, n_slots, cus):
    """What nxg_launch_pub_stage1 / stage2 do: the repeated-Id check's grid and the rows between
    two visits of one thread; the radix sort's passes."""
    k = constants()
    grid = min(_cdiv(n_rows, k["PUB_TPB"]), cus * k["NXG_PUB_GCAP"])
    bits = 1
    while bits < 32 and (1 << bits) <= n_slots:
        bits += 1
    return {"grid": grid, "stride": grid * k["PUB_TPB"], "strided": n_rows > grid * k["PUB_TPB"],
            "bits": bits, "passes": _cdiv(bits, 8), "n_seg": _cdiv(n_rows, k["PUB_SEG"])}


# ---- dispatch cases ----------------------------------------------------------------------------
class DispatchCase(types.SimpleNamespace):
    """name, reaches, n_chans, ids and the NxgSubTable arrays (slot_of_id, sub_id, stream_off,
    stream_chan, keep); id_of_slot; repeat_id / repeat_rows (a kept-`last` Id named again within a
    step, in the next step, in another segment); per-case extras."""

    def table(self):
        return (self.slot_of_id, self.sub_id, self.stream_off, self.stream_chan, self.keep)

    @property
    def n_rows(self):
        return len(self.ids)

    @property
    def n_slots(self):
        return len(self.sub_id)

    def fan_of_rows(self):
        """Streams of every row's subscription (0: unmatched or none)."""
        s = np.full(len(self.ids), NO_SLOT, np.uint32)
        ok = self.ids < np.uint64(len(self.slot_of_id))
        s[ok] = self.slot_of_id[self.ids[ok].astype(np.int64)]
        fan = np.diff(self.stream_off.astype(np.int64))
        out = np.zeros(len(self.ids), np.int64)
        hit = s != NO_SLOT
        out[hit] = fan[s[hit]]
        return out, s


def _table(slot_streams, seed):
    """Slots in a shuffled order behind Ids with every seventh Id a hole."""
    n_slots = len(slot_streams)
    rng = np.random.default_rng(seed)
    cand = np.arange(n_slots + n_slots // 6 + 8)
    used = cand[cand % 7 != 3][:n_slots]
    n_ids = (int(used[-1]) + 3) if n_slots else 5
    slot_of_id = np.full(n_ids, NO_SLOT, np.uint32)
    perm = rng.permutation(n_slots).astype(np.uint32)
    slot_of_id[used] = perm
    id_of_slot = np.zeros(n_slots, np.uint64)
    id_of_slot[perm] = used.astype(np.uint64)
    fan = np.array([len(s) for s in slot_streams], np.int64)
    off = np.zeros(n_slots + 1, np.uint32)
    off[1:] = np.cumsum(fan)
    chan = (np.concatenate([np.asarray(s, np.uint32) for s in slot_streams])
            if fan.sum() else np.zeros(0, np.uint32))
    sub_id = rng.integers(0, U64_MAX, n_slots, dtype=np.uint64, endpoint=True)
    keep = (np.arange(n_slots) % 3 != 1).astype(np.uint8)
    return types.SimpleNamespace(slot_of_id=slot_of_id, sub_id=sub_id, stream_off=off,
                                 stream_chan=chan, keep=keep, id_of_slot=id_of_slot,
                                 n_ids=n_ids)


def _sprinkle(ids, n_ids):
    """Ids past the table, 2^64 - 1 and a hole (Id 3: every seventh Id has no slot) among the
    rows."""
    i = np.arange(len(ids))
    ids[i % 89 == 11] = np.uint64(3)
    ids[i % 97 == 5] = (n_ids + i[i % 97 == 5] % 5).astype(np.uint64)
    ids[i % 101 == 7] = np.uint64(U64_MAX)
    return (i % 97 == 5) | (i % 101 == 7) | (i % 89 == 11)


def _repeat_rows(n_rows, seg_rows):
    want = [1, 3, STEP + 6, seg_rows + 2, 3 * seg_rows + 9, n_rows - 2]
    return sorted({p for p in want if 0 <= p < n_rows})


def _dispatch_case(name, reaches, n_chans, n_rows, slot_streams, seed, must_slots=(),
                   fill=None, free=None, repeat_slot=None, **extra):
    """Rows drawn over the whole Id range (holes included) with every Id of the table named once
    where the batch is long enough (or as `fill` lays them out); `must_slots` named for certain
    (in rows where `free` allows); one kept-`last` Id repeated."""
    tb = _table(slot_streams, seed)
    rng = np.random.default_rng(seed + 1)
    ids = rng.integers(0, tb.n_ids, n_rows, dtype=np.uint64)
    if n_rows >= tb.n_ids:
        ids[: tb.n_ids] = rng.permutation(tb.n_ids).astype(np.uint64)
    if fill is not None:
        fill(ids, tb, rng)
    taken = _sprinkle(ids, tb.n_ids)
    seg_rows = plan(n_rows, n_chans)["seg_rows"]
    rep = _repeat_rows(n_rows, seg_rows)
    taken[rep] = True
    if free is not None:
        taken |= ~free(np.arange(n_rows))
    open_rows = np.flatnonzero(~taken)
    must_slots = list(must_slots)
    assert len(open_rows) >= len(must_slots), name
    # spread over the batch, so that every part of it sees some of them
    at = open_rows[np.arange(len(must_slots)) * (len(open_rows) // max(len(must_slots), 1))]
    ids[at] = tb.id_of_slot[np.asarray(must_slots, np.int64)] if must_slots else ids[at]
    kept = np.flatnonzero(tb.keep == 1)
    repeat_id = None
    if len(kept):
        fan = np.diff(tb.stream_off.astype(np.int64))
        pick = kept[np.argmax(fan[kept] > 0)] if n_chans else kept[0]
        if repeat_slot is not None:
            assert tb.keep[repeat_slot] == 1
            pick = repeat_slot
        repeat_id = int(tb.id_of_slot[pick])
        ids[rep] = np.uint64(repeat_id)
    return DispatchCase(name=name, reaches=reaches, n_chans=n_chans, ids=ids,
                        slot_of_id=tb.slot_of_id, sub_id=tb.sub_id, stream_off=tb.stream_off,
                        stream_chan=tb.stream_chan, keep=tb.keep, id_of_slot=tb.id_of_slot,
                        repeat_id=repeat_id, repeat_rows=rep, must_slots=must_slots, **extra)


def _edge_slots(n, max_fan):
    """Slots that name channel 0, n - 2 and n - 1 as the first and as the second stream of
    two-stream slots, alone, and in 3 / 4 / 5-stream slots; and one with no stream."""
    e = [[0], [n - 1], [n - 2], []]
    if max_fan >= 2:
        e += [[0, n - 1], [n - 1, 0], [n - 2, n - 1], [n - 1, n - 2], [0, n - 2], [n - 2, 0]]
    if max_fan >= 3:
        e += [[0, n - 1, n - 2]]
    if max_fan >= 4:
        e += [[n - 1, n - 2, 0, 1]]
    if max_fan >= 5:
        e += [[n - 1, 1, n - 2, 2, 0]]
    return e


def _mixed_slots(n_chans, n_slots, max_fan, seed):
    """Edge slots first, then slots of 0..max_fan distinct channels."""
    r = random.Random(seed)
    edge = _edge_slots(n_chans, max_fan)
    rest = [r.sample(range(n_chans), (j + len(edge)) % (max_fan + 1))
            for j in range(n_slots - len(edge))]
    return edge + rest, list(range(len(edge)))


def _seg_global(name, n_rows, want_seg):
    n = 1 << 20
    slots, edge = _mixed_slots(n, 1500, 3, 101)
    groups = want_seg // (STEP * constants()["NXG_DISP_U"])
    return _dispatch_case(name, f"seg_rows {want_seg}: {groups} step groups per "
                          "segment, counters and cursors in global memory, no row cache, "
                          "top scan past one round", n, n_rows, slots, 7 + want_seg, edge,
                          want_seg=want_seg)


def _top_fused(name, n_rows, nb):
    slots, edge = _mixed_slots(1024, 3000, 2, 202)
    return _dispatch_case(name, f"fused top scan with {nb} block totals", 1024, n_rows, slots,
                          nb, edge, want_nb=nb)


def _cache(n_chans):
    slots, edge = _mixed_slots(n_chans, 1300, 5, 300 + n_chans)
    return _dispatch_case(f"cache_{n_chans}", "row cache encoding boundary", n_chans, 3000, slots,
                          n_chans, edge)


def _dup_slots(n, seed):
    r = random.Random(seed)
    a, b, c, d, e = r.sample(range(n), 5)
    z = n - 1
    two = [[a, a], [z, z], [0, 0]]                      # the cached form
    few = [[a, b, a], [a, a, b], [b, a, a], [a, b, c, b], [a, b, b, a], [0, z, z], [a] * 3,
           [a] * 4, [c, c, d, d]]                       # 3 or 4 streams
    many = [[a] * 5, [a] * 6, [a, b, a, c, a, b], [a, b, c, d, e, a], [0, z, 0, z, 0],
            [e, d, c, b, a, e, d]]                      # more than RF streams
    plain = [[a], [a, b], [], [a, b, c], [a, b, c, d], [a, b, c, d, e]]
    rand = []
    for j in range(300):
        pool = r.sample(range(n), 3)
        rand.append([r.choice(pool) for _ in range(2 + j % 6)])
    slots = two + few + many + plain + rand
    return slots, {"two": range(0, 3), "few": range(3, 12), "many": range(12, 18)}


def _dup(name, n_chans):
    """Steps (64 rows) by number k: k % 4 == 0 holds exactly one row that repeats a channel
    among rows that do not, none with more than RF streams (only the `dup` test sends the wave to
    the match loop); k % 4 == 1 rows of at most RF streams, repeats among them; the others
    anything, the named slots included."""
    rf = constants()["RF"]
    slots, groups = _dup_slots(n_chans, 400 + n_chans)
    must = [s for g in groups.values() for s in g]
    fan = np.array([len(s) for s in slots])
    rpt = np.array([len(set(s)) < len(s) for s in slots])
    plain = np.flatnonzero((fan <= rf) & ~rpt)
    narrow_dup = np.flatnonzero((fan <= rf) & rpt)
    narrow = np.flatnonzero(fan <= rf)

    def fill(ids, tb, rng):
        i = np.arange(len(ids))
        k = i // STEP
        ids[:] = tb.id_of_slot[rng.integers(0, len(slots), len(ids))]
        for sel, pool in ((k % 4 == 0, plain), (k % 4 == 1, narrow),
                          ((k % 4 == 0) & (i % STEP == (k * 5) % STEP), narrow_dup)):
            ids[sel] = tb.id_of_slot[pool[rng.integers(0, len(pool), int(sel.sum()))]]

    c = _dispatch_case(name, "rows that name one channel 2..6 times: the scatter's dup "
                       "branch, its cached two-stream form, the match loop", n_chans, 3000,
                       slots, 500 + n_chans, must, fill=fill, free=lambda i: (i // STEP) % 4 >= 2,
                       repeat_slot=int(plain[np.argmax(fan[plain] > 0)]), groups=groups)
    # the sprinkled Ids may have overwritten a single repeating row: put it back
    i = np.arange(c.n_rows)
    one = ((i // STEP) % 4 == 0) & (i % STEP == ((i // STEP) * 5) % STEP)
    rng = np.random.default_rng(550 + n_chans)
    c.ids[one] = c.id_of_slot[narrow_dup[rng.integers(0, len(narrow_dup), int(one.sum()))]]
    return c


def _fan(name, n_chans):
    """Steps (64 rows) by number k: k % 3 == 0 holds exactly one row with more than RF streams
    among rows with at most RF, k % 3 == 1 holds none, k % 3 == 2 a mix."""
    rf = constants()["RF"]
    r = random.Random(600 + n_chans)
    narrow = [r.sample(range(n_chans), j % (rf + 1)) for j in range(400)]
    wide = [r.sample(range(n_chans), rf + 1 + j % 5) for j in range(60)]
    n_rows = 5050  # 78 steps and a partial one that still holds its wide row

    def fill(ids, tb, rng):
        nid = tb.id_of_slot[: len(narrow)]
        wid = tb.id_of_slot[len(narrow):]
        ids[:] = nid[rng.integers(0, len(nid), len(ids))]
        i = np.arange(len(ids))
        k = i // STEP
        one = (k % 3 == 0) & (i % STEP == (k * 7) % STEP)
        mix = (k % 3 == 2) & (rng.random(len(ids)) < 0.4)
        put = one | mix
        ids[put] = wid[rng.integers(0, len(wid), int(put.sum()))]

    c = _dispatch_case(name, f"fan-out {rf + 1}..{rf + 5}: the match loop reading a row's "
                       "streams from memory", n_chans, n_rows, narrow + wide, 700 + n_chans,
                       fill=fill, n_narrow=len(narrow))
    # the sprinkled Ids may have overwritten a single wide row: put it back
    i = np.arange(n_rows)
    k = i // STEP
    one = (k % 3 == 0) & (i % STEP == (k * 7) % STEP)
    rng = np.random.default_rng(800 + n_chans)
    wid = c.id_of_slot[len(narrow):]
    c.ids[one] = wid[rng.integers(0, len(wid), int(one.sum()))]
    return c


def _none_match():
    slots, _ = _mixed_slots(7, 50, 3, 900)
    c = _dispatch_case("none_match", "a batch in which nothing matches: every total 0", 7, 300,
                       slots, 901)
    i = np.arange(300)
    holes = np.flatnonzero(c.slot_of_id == NO_SLOT).astype(np.uint64)
    c.ids[:] = holes[i % len(holes)]
    _sprinkle(c.ids, len(c.slot_of_id))
    c.repeat_id, c.repeat_rows = None, []
    return c


def _no_chans():
    return _dispatch_case("no_chans", "n_chans == 0: M = 0, no scan, no scatter; last_row and "
                          "n_unmatched still due", 0, 300, [[] for _ in range(40)], 910)


def _no_slots():
    return _dispatch_case("no_slots", "a table with no slots", 4, 300, [], 920)


def _simple(name, reaches, n_chans, n_rows, n_slots, max_fan, seed, **extra):
    slots, edge = _mixed_slots(n_chans, n_slots, max_fan, seed)
    return _dispatch_case(name, reaches, n_chans, n_rows, slots, seed + 1, edge, **extra)


_DISPATCH = {
    "seg256_global": lambda: _seg_global("seg256_global", 8321, 256),
    "seg512_global": lambda: _seg_global("seg512_global", 16500, 512),
    "seg256_lds": lambda: _simple(
        "seg256_lds", "seg_rows 256 with LDS cursors and masks carried from one step group to "
        "the next; fused top scan over 8193 block totals", 1024, 8388737, 5000, 1, 303,
        want_seg=256),
    "top_fused_1024": lambda: _top_fused("top_fused_1024", 524288, 1024),
    "top_fused_1025": lambda: _top_fused("top_fused_1025", 524289, 1025),
    "top_unfused": lambda: _simple(
        "top_unfused", "scan_top + scan_add past one round, wide cache", 40000, 13500, 2000, 3,
        404),
    "dup_lds": lambda: _dup("dup_lds", 5),
    "dup_global": lambda: _dup("dup_global", 2000),
    "fan_global": lambda: _fan("fan_global", 3000),
    "fan_lds": lambda: _fan("fan_lds", 1000),
    "none_match": _none_match,
    "no_chans": _no_chans,
    "no_slots": _no_slots,
}
CACHE_CHANS = (253, 254, 255, 256, 65533, 65534, 65535, 65536)
for _n in CACHE_CHANS:
    _DISPATCH[f"cache_{_n}"] = functools.partial(_cache, _n)
DISPATCH_CASES = tuple(_DISPATCH)
LARGE_ROWS = 100_000   # cases above this: the Python restatement runs on a prefix
PREFIX_ROWS = 20_000


@functools.lru_cache(maxsize=32)
def _dispatch_cached(name):
    return _DISPATCH[name]()


def dispatch_case(name):
    """The case (shared between tests: do not modify it). The 8.4 M-row case is rebuilt on every
    call instead of being held."""
    return _DISPATCH[name]() if name == "seg256_lds" else _dispatch_cached(name)


# ---- commit cases ------------------------------------------------------------------------------
A = int(np.float64(1.5).view(np.uint64))  # the table's current value of every slot
B = int(np.float64(2.5).view(np.uint64))


class CommitCase(types.SimpleNamespace):
    """name, reaches, n_clients, the batch (ids, kind, to_client, fixed: F64 bits) and the
    NxgPubTable arrays (slot_of_id, client_off, client, cur_fixed); pair: the repeated rows."""

    @property
    def n_rows(self):
        return len(self.ids)

    @property
    def n_slots(self):
        return len(self.client_off) - 1

    def columns(self):
        """(tag, aux, cur_tag, cur_aux): every value is an F64."""
        return (np.full(self.n_rows, 9, np.uint8), np.zeros(self.n_rows, np.uint32),
                np.full(self.n_slots, 9, np.uint8), np.zeros(self.n_slots, np.uint32))


def _pub_table(n_slots, n_clients, n_extra_ids=3):
    """Identity Id -> slot (ascending Ids walk the slot bitmap word by word), 1 or 2 clients per
    slot; the first slots name client 0, n - 2 and n - 1 first and second."""
    s = np.arange(n_slots, dtype=np.int64)
    fan = 1 + (s % 2)
    first = (s * 7919) % n_clients
    step = np.ones(n_slots, np.int64)
    edge = [(0, 1, 1), (n_clients - 1, 2, 1), (n_clients - 2, 2, 1), (0, 2, n_clients - 1),
            (n_clients - 1, 1, 1), (n_clients - 2, 1, 1), (0, 2, n_clients - 2)]
    for j, (f, k, st) in enumerate(edge[: n_slots]):
        first[j], fan[j], step[j] = f % n_clients, k if n_clients > 1 else 1, st
    off = np.zeros(n_slots + 1, np.uint32)
    off[1:] = np.cumsum(fan)
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), fan)
    client = ((np.repeat(first, fan) + within * np.repeat(step, fan)) % n_clients).astype(np.uint32)
    slot_of_id = np.full(n_slots + n_extra_ids, NO_SLOT, np.uint32)
    slot_of_id[:n_slots] = np.arange(n_slots, dtype=np.uint32)
    return slot_of_id, off, client, np.full(n_slots, A, np.uint64)


def _commit_case(name, reaches, n_clients, ids, kind, to_client, fixed, n_slots, **extra):
    soi, off, client, cur = _pub_table(n_slots, n_clients)
    return CommitCase(name=name, reaches=reaches, n_clients=n_clients,
                      ids=np.ascontiguousarray(ids, np.uint64),
                      kind=np.ascontiguousarray(kind, np.uint8),
                      to_client=np.ascontiguousarray(to_client, np.uint32),
                      fixed=np.ascontiguousarray(fixed, np.uint64), slot_of_id=soi,
                      client_off=off, client=client, cur_fixed=cur, **extra)


# the two rows of the single repeat, by name (n = 2000 rows; `stride` takes the CU count)
PAIRS = {
    "adjacent": (700, 701),         # one run of equal bitmap words, neighbouring lanes
    "same_word_far": (642, 669),    # one run, 27 lanes apart
    "other_run": (645, 680),        # one wave, the second row a run of its own
    "lane63_64": (703, 704),        # two waves of one workgroup
    "wg_edge": (255, 256),          # two workgroups
    "first_last": (0, 1999),
}
VARIANTS = ("same", "back")  # B, then B as UpdateChanged (not pushed) / then A (pushed)
ORDERS = ("asc", "perm")     # Ids ascending (the runs path) / permuted (one atomic per lane)


def single_repeat(where, order, variant, cus=None):
    """Every Id once, except that row q names row p's Id again: row p is Update(B), row q
    UpdateChanged(B) -- equal to the row before it, not pushed -- or UpdateChanged(A): pushed.
    Compared with the table (current = A) instead, either answer flips."""
    k = constants()
    if where == "stride":
        grid = cus * k["NXG_PUB_GCAP"]
        n = 2 * grid * k["PUB_TPB"] + 300
        p = 5 * k["PUB_TPB"] + 17
        q = p + grid * k["PUB_TPB"]
    else:
        n = 2000
        p, q = PAIRS[where]
    rng = np.random.default_rng(1000 + 10 * (list(PAIRS) + ["stride"]).index(where) +
                                ORDERS.index(order))
    ids = (np.arange(n) if order == "asc" else rng.permutation(n)).astype(np.uint64)
    kind = rng.integers(0, 2, n).astype(np.uint8)
    fixed = np.where(rng.random(n) < 0.5, np.uint64(A), np.uint64(B))
    to = np.zeros(n, np.uint32)
    i = np.arange(n)
    if order == "perm":
        # directed rows and unpublished Ids (each once) among the permuted rows
        d = (i % 53 == 9) & (i != p) & (i != q)
        kind[d] = PUB_UPDATE_CLIENT
        to[d] = (i[d] % 7).astype(np.uint32)  # n_clients = 5: 5 and 6 are dropped
        u = (i % 61 == 11) & (i != p) & (i != q) & ~d
        ids[u] = (n + 3 + i[u]).astype(np.uint64)
        ids[np.flatnonzero(u)[0]] = np.uint64(U64_MAX)
    ids[q] = ids[p]
    kind[p], fixed[p] = PUB_UPDATE, B
    kind[q], fixed[q] = PUB_UPDATE_CHANGED, (B if variant == "same" else A)
    return _commit_case(f"single_repeat_{where}-{order}-{variant}",
                        "one repeated Id: the repeated-Id flag decides whether prev() exists",
                        5, ids, kind, to, fixed, n, pair=(p, q), pushed=variant == "back",
                        order=order)


def repeat_only_directed(with_sort, variant):
    """Id X is named by three directed rows (value B) and by one UpdateChanged row: that row
    compares with the table (A), never with a directed row. `with_sort`: another Id does repeat,
    so the radix sort runs and must leave the directed rows out."""
    n = 1500
    rng = np.random.default_rng(2000 + with_sort)
    ids = rng.permutation(n).astype(np.uint64)
    kind = rng.integers(0, 2, n).astype(np.uint8)
    fixed = np.where(rng.random(n) < 0.5, np.uint64(A), np.uint64(B))
    to = np.zeros(n, np.uint32)
    q = 900
    for r, cl in ((200, 1), (300, 2), (400, 1)):
        ids[r], kind[r], fixed[r], to[r] = ids[q], PUB_UPDATE_CLIENT, B, cl
    kind[q], fixed[q] = PUB_UPDATE_CHANGED, (B if variant == "same" else A)
    if with_sort:
        ids[60] = ids[50]
        kind[50], fixed[50] = PUB_UPDATE, B
        kind[60], fixed[60] = PUB_UPDATE_CHANGED, B
    return _commit_case(f"repeat_only_directed-{'sort' if with_sort else 'nosort'}-{variant}",
                        "an Id repeated only by directed rows", 5, ids, kind, to, fixed, n,
                        pair=(400, q), pushed=variant == "same", with_sort=with_sort)


def slot_bits_31_32():
    """Repeats on the slots either side of a bitmap word edge (31 | 32, 63 | 64); their
    neighbours 30, 33, 62, 65 occur once."""
    n = 600
    rng = np.random.default_rng(2100)
    ids = np.arange(n, dtype=np.uint64)
    kind = rng.integers(0, 2, n).astype(np.uint8)
    fixed = np.where(rng.random(n) < 0.5, np.uint64(A), np.uint64(B))
    again = {31: B, 32: A, 63: A, 64: B}
    for j, (s, v) in enumerate(again.items()):
        kind[s], fixed[s] = PUB_UPDATE, B
        r = 300 + 67 * j
        ids[r], kind[r], fixed[r] = s, PUB_UPDATE_CHANGED, v
    for s in (30, 33, 62, 65):
        kind[s] = PUB_UPDATE_CHANGED
    return _commit_case("slot_bits_31_32", "repeats on slots 31 | 32 and 63 | 64", 5, ids, kind,
                        np.zeros(n, np.uint32), fixed, n,
                        again={300 + 67 * j: s for j, s in enumerate(again)})


RADIX_SLOTS = 1 << 24


def radix_4_passes():
    """2^24 slots: the radix sort's fourth pass. Rows name the 40 lowest and the 40 highest slots
    with repeats; the highest slot's low 24 bits equal those of the key of a row without a slot,
    so only the fourth digit keeps directed rows out of its run (rows 10..12)."""
    n, ns = 5000, RADIX_SLOTS
    rng = np.random.default_rng(2200)
    pool = np.concatenate([np.arange(40), np.arange(ns - 40, ns), [ns - 1] * 20]).astype(np.uint64)
    ids = pool[rng.integers(0, len(pool), n)]
    i = np.arange(n)
    ids[i % 37 == 4] = (ns + 3 + i[i % 37 == 4] % 9).astype(np.uint64)  # unpublished
    kind = rng.choice(np.array([0, 1, 1, 2], np.uint8), n)
    to = rng.integers(0, 8, n).astype(np.uint32)  # n_clients = 6
    c = int(np.float64(-3.0).view(np.uint64))
    fixed = rng.choice(np.array([A, B, c], np.uint64), n)
    x = ns - 1
    ids[10:13] = x
    kind[10], fixed[10] = PUB_UPDATE, B
    kind[11], fixed[11], to[11] = PUB_UPDATE_CLIENT, A, 2
    kind[12], fixed[12] = PUB_UPDATE_CHANGED, B  # equal to row 10: not pushed
    return _commit_case("radix_4_passes", "n_slots = 2^24: four radix passes", 6, ids, kind, to,
                        fixed, ns, pair=(10, 12), pushed=False)


DIRECTED_CLIENTS = (253, 254, 65533, 65534)


def directed_edges(n_clients):
    """Directed rows to client 0, n - 1, n (dropped) and 2^32 - 1 (dropped) with n_clients on
    either side of the row cache's two bounds."""
    n, ns = 3000, 1200
    rng = np.random.default_rng(2300 + n_clients)
    ids = rng.integers(0, ns + 3, n).astype(np.uint64)
    kind = rng.choice(np.array([0, 1, 2, 2], np.uint8), n)
    fixed = np.where(rng.random(n) < 0.5, np.uint64(A), np.uint64(B))
    targets = np.array([0, n_clients - 1, n_clients, 0xFFFFFFFF, n_clients - 2, 1], np.uint32)
    to = targets[np.arange(n) % len(targets)]
    ids[:8] = np.arange(8)  # the slots whose clients are 0, n - 2, n - 1
    kind[:8] = PUB_UPDATE
    return _commit_case(f"directed_edges_{n_clients}", "directed rows at the cache bounds",
                        n_clients, ids, kind, to, fixed, ns, targets=targets)


def _commit_names():
    names = []
    for w in list(PAIRS) + ["stride"]:
        for o in ORDERS:
            for v in VARIANTS:
                names.append(f"single_repeat_{w}-{o}-{v}")
    for s in ("sort", "nosort"):
        for v in VARIANTS:
            names.append(f"repeat_only_directed-{s}-{v}")
    names += ["slot_bits_31_32", "radix_4_passes"]
    names += [f"directed_edges_{c}" for c in DIRECTED_CLIENTS]
    return tuple(names)


COMMIT_CASES = _commit_names()


def commit_case(name, cus=256):
    """The case of that name; `cus` (the device's compute units) sizes the `stride` cases."""
    if name.startswith("single_repeat_"):
        where, order, variant = name[len("single_repeat_"):].split("-")
        return single_repeat(where, order, variant, cus)
    if name.startswith("repeat_only_directed-"):
        _, s, v = name.split("-")
        return repeat_only_directed(s == "sort", v)
    if name.startswith("directed_edges_"):
        return directed_edges(int(name.rsplit("_", 1)[1]))
    return {"slot_bits_31_32": slot_bits_31_32, "radix_4_passes": radix_4_passes}[name]()


def unsubscribe_case(n_clients):
    """(ids, clients): unsubscribes to clients on both sides of n_clients, the top client and its
    neighbours included (the all-mode-2 route through the row cache)."""
    n = 3000
    rng = np.random.default_rng(2400 + n_clients)
    ids = rng.integers(0, 10 ** 6, n, dtype=np.uint64)
    edge = np.array([0, 1, n_clients - 2, n_clients - 1, n_clients, n_clients + 1, 0xFFFFFFFF],
                    np.uint32)
    cl = rng.integers(0, n_clients, n).astype(np.uint32)
    i = np.arange(n)
    cl[i % 3 == 0] = edge[(i[i % 3 == 0] // 3) % len(edge)]
    return ids, cl


def prefix(case, n):
    """The first n rows of a case, on the same table."""
    c = case.__class__(**vars(case))
    for f in ("ids", "kind", "to_client", "fixed"):
        if hasattr(case, f):
            setattr(c, f, getattr(case, f)[:n].copy())
    if hasattr(case, "repeat_rows"):
        c.repeat_rows = [r for r in case.repeat_rows if r < n]
    return c
