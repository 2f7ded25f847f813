"""The case tables of nxg_archive_index_records and nxg_archive_scan_index
(tests/test_archive_index_cpu.py, tests/test_gpu_archive_index.py).

`constants()` reads the kernels' constants out of netidx_amd/csrc/nxg_archive_index.hip; `plan()`
and `scan_plan()` compute from them which branches a case reaches, and every case states what it
is there for (`want`). A retune then names the case that no longer sits on its edge.
"""
import os
import re

import numpy as np

import archive_index_model as am
from archive_index_model import NO_SLOT, Case

HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc",
                   "nxg_archive_index.hip")
M64 = (1 << 64) - 1


def constants():
    src = open(HIP).read()

    def const(name, pat=r"(\d+)"):
        m = re.search(r"constexpr \w+ %s = %s" % (name, pat), src)
        assert m, f"{name} not found in nxg_archive_index.hip"
        return int(m.group(1), 0)

    assert re.search(r"\(k \* AIX_HASH_MUL\) >> \(64 - A\.slot_bits\)", src), "the table's hash"
    return dict(block=const("AIX_KEYS_PER_BLOCK"), tile=const("AIX_KEYS_PER_TILE"),
                top=const("AIX_TOP_WIDTH"), min_bits=const("AIX_MIN_SLOT_BITS"),
                mul=const("AIX_HASH_MUL", r"(0x[0-9A-Fa-f]+)ull"), piece=const("AIX_PIECE_BYTES"),
                scan_block=const("AIX_SCAN_BLOCK"))


def slot_bits(n_keys, K):
    b = K["min_bits"]
    while (1 << b) < 2 * n_keys:
        b += 1
    return b


def home(rec, ident, bits, K):
    """The slot the key (rec, ident) probes from."""
    return (((rec << 32 | ident) * K["mul"]) & M64) >> (64 - bits)


# ---- the writer: the branches a case reaches -----------------------------------------------------
def plan(case, K=None):
    K = K or constants()
    n = case.n_keys
    recs = am.indexes_python(case)
    off = [int(x) for x in case.seg_off]
    kept = np.zeros(n, bool)
    for p in range(off[0], off[-1]):
        kept[p] = am.kept_id(case, p) is not None
    firsts = sum(len(o) for _, o in recs)
    bits = slot_bits(n, K)
    # the table's clusters do not depend on the order of insertion
    taken, displaced, wrapped = set(), 0, False
    for c, (_, order) in enumerate(recs):
        for i in order:
            h = home(c, i, bits, K)
            while h in taken:
                displaced += 1
                h += 1
                if h == 1 << bits:
                    h, wrapped = 0, True
            taken.add(h)
    ids_in = {}
    for c, (_, order) in enumerate(recs):
        for i in order:
            ids_in[i] = ids_in.get(i, 0) + 1
    inner = [len(b) - am.varint_len(len(b)) for b, _ in recs if b]
    blocks = -(-n // K["block"])
    return dict(blocks=blocks, groups=-(-blocks // K["top"]), tiles=-(-n // K["tile"]),
                recs=case.n_recs, empty=sum(1 for b, _ in recs if not b),
                count_widths={am.varint_len(len(o)) for _, o in recs if o},
                len_widths={am.varint_len(len(b)) for b, _ in recs if b},
                id_widths={am.varint_len(i) for _, o in recs for i in o},
                inner=set(inner), counts={len(o) for _, o in recs},
                dropped=int((~kept[off[0]:off[-1]]).sum()), dups=int(kept.sum()) - firsts,
                shared=sum(1 for v in ids_in.values() if v > 1), outside=n - (off[-1] - off[0]),
                displaced=displaced, wrapped=wrapped, bits=bits)


def reaches(p, want):
    """Does the plan p have what the case is there for? Sets: at least these; numbers: exactly;
    ("min", v): at least v."""
    for k, v in want.items():
        if isinstance(v, set):
            if not v <= p[k]:
                return False
        elif isinstance(v, tuple):
            if p[k] < v[1]:
                return False
        elif p[k] != v:
            return False
    return True


def ids_for_inner(target):
    """Distinct Ids whose RecordIndex has exactly `target` bytes from the count on: one-byte Ids
    0.., then two-byte Ids 128.. ."""
    for ones in range(0, 128):
        for cw in (1, 2):
            rest = target - cw - ones
            if rest < 0 or rest % 2:
                continue
            twos = rest // 2
            if twos <= 16384 - 128 and am.varint_len(ones + twos) == cw:
                return list(range(ones)) + list(range(128, 128 + twos))
    raise AssertionError(target)


ID_WIDTHS = [0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28,
             0xFFFFFFFF, 0xFFFFFFFE]


def colliding_ids(rec, bits, K, slot, count, start=0):
    out, i = [], start
    while len(out) < count:
        if home(rec, i, bits, K) == slot:
            out.append(i)
        i += 1
    return out


def cases(K=None):
    """name -> (Case, want)."""
    K = K or constants()
    B, T, W = K["block"], K["tile"], K["top"]
    out = {}

    def add(name, case, want):
        assert name not in out
        out[name] = (case, want)

    def mixed(n):  # duplicates near and far, two records
        p = np.arange(n, dtype=np.uint64)
        return Case((p * np.uint64(7)) % np.uint64(n // 2 + 1), [0, n // 3, n])

    # position counts: one wave, one block, one tile, two tiles and the top scan's width, each +- 1
    for name, n, want in [
            ("n1", 1, dict(blocks=1)), ("wave-1", 63, dict(blocks=1)), ("wave", 64, dict(blocks=1)),
            ("wave+1", 65, dict(blocks=1)), ("block-1", B - 1, dict(blocks=1)),
            ("block", B, dict(blocks=1)), ("block+1", B + 1, dict(blocks=2)),
            ("tile-1", T - 1, dict(tiles=1)), ("tile", T, dict(tiles=1)),
            ("tile+1", T + 1, dict(tiles=2)), ("tiles2+1", 2 * T + 1, dict(tiles=3)),
            ("top-1", (W - 1) * B, dict(blocks=W - 1, groups=1)),
            ("top", W * B, dict(blocks=W, groups=1)),
            ("top+1", (W + 1) * B, dict(blocks=W + 1, groups=2))]:
        add(name, mixed(n), want)

    n = 3 * T + 5
    p = np.arange(n, dtype=np.uint64)
    add("all_distinct", Case(p * np.uint64(3), [0, 7, n]), dict(dups=0, tiles=4))
    add("one_id_1e5", Case(np.full(100_000, 77), [0, 100_000]), dict(dups=99_999, counts={1}))
    add("one_id_3_records", Case(np.full(100_000, 77), [0, 1, 50_000, 100_000]),
        dict(dups=99_997, counts={1}, shared=1))
    add("dup_a_tile_apart", Case(p[:3 * T] % np.uint64(T) + np.uint64(1000), [0, 3 * T]),
        dict(dups=2 * T, tiles=3))
    add("same_ids_every_record", Case(p[:5 * 300] % np.uint64(100), [0, 300, 600, 900, 1200, 1500]),
        dict(shared=100, recs=5, counts={100}))

    # the table: 60 keys that share one home slot, and 40 at the table's last slot
    bits = slot_bits(200, K)
    ids = colliding_ids(0, bits, K, 5, 60) + colliding_ids(0, bits, K, (1 << bits) - 1, 40)
    add("table_collide_wrap", Case(np.array(ids + ids[::-1]), [0, 200]),
        dict(wrapped=True, displaced=("min", 59 * 60 // 2 + 39 * 40 // 2), bits=bits, dups=100))
    # ... and keys of two records that share one home slot
    bits = slot_bits(60, K)
    ids1 = colliding_ids(1, bits, K, 9, 30)
    add("table_collide_two_records", Case(np.array(colliding_ids(0, bits, K, 9, 30) + ids1),
                                          [0, 30, 60]),
        dict(displaced=("min", 59 * 60 // 2), recs=2))

    # Ids of every varint width
    add("id_widths", Case(np.array(ID_WIDTHS * 3), [0, 5, len(ID_WIDTHS) * 3]),
        dict(id_widths={1, 2, 3, 4, 5}))

    # the widths of varint(L): inner of 126 | 127 bytes and of 16381 | 16382 bytes are the edges
    # (len_wrapped_len(126) = 127, (127) = 129, (16381) = 16383, (16382) = 16385); 16383 as well
    for t, w in ((126, 1), (127, 2), (16381, 2), (16382, 3), (16383, 3)):
        ids = ids_for_inner(t)
        add(f"inner_{t}", Case(np.array(ids + ids[:40]), [0, len(ids) + 40]),
            dict(inner={t}, len_widths={w}))
    # the width of the count
    for c in (127, 128):
        add(f"count_{c}", Case(np.arange(2 * c) % c + 300, [0, 2 * c]), dict(counts={c}))

    # runs of empty records
    add("empty_first", Case(p[:700] % np.uint64(90), [0, 0, 0, 0, 300, 700]), dict(empty=3))
    add("empty_middle", Case(p[:700] % np.uint64(90), [0, 300, 300, 300, 300, 700]), dict(empty=3))
    add("empty_last", Case(p[:700] % np.uint64(90), [0, 300, 700, 700, 700, 700]), dict(empty=3))
    add("all_empty", Case(p[:10], [4] * 9), dict(empty=8, outside=10))
    add("keys_outside_records", Case(np.where((p[:900] < 100) | (p[:900] >= 800),
                                              np.uint64(1 << 40), p[:900] % np.uint64(50)),
                                     [100, 400, 800]), dict(outside=200, recs=2))

    rng = np.random.default_rng(0xA1D)
    sizes = rng.integers(0, 40, 1000)
    off = np.concatenate([[0], np.cumsum(sizes)])
    add("recs1000", Case(rng.integers(0, 300, int(off[-1])), off),
        dict(recs=1000, empty=("min", 1), shared=("min", 100)))

    # SubIds through the recorder's table: dropped ones, and SubIds at and past n_subs
    tab = np.where(np.arange(500) % 4 == 1, NO_SLOT, (np.arange(500) * 37) % 200 + 3)
    add("table", Case(rng.integers(0, 520, 2 * T + 9), [0, 40, T, T, 2 * T + 9], tab),
        dict(dropped=("min", 200), dups=("min", 100), recs=4))
    add("table_drops_all", Case(p[:T + 3] % np.uint64(8), [0, 9, T + 3], np.full(8, NO_SLOT)),
        dict(empty=2, dropped=T + 3))
    add("table_sub_past_end", Case(np.where(p[:300] % 3 == 1, np.uint64(M64), p[:300] % np.uint64(2)),
                                   [0, 300], np.array([9, 300])), dict(dropped=100, counts={2}))
    add("table_empty", Case(p[:50], [0, 50], np.zeros(0)), dict(dropped=50, empty=1))
    return out


def refusal_cases(K=None):
    """name -> (Case, what am.refusal names)."""
    K = K or constants()
    T = K["tile"]
    p = np.arange(2 * T + 1, dtype=np.uint64)
    out = {"seg_decreases": (Case(p[:50], [0, 20, 10, 30, 25, 50]), ("seg", 1)),
           "seg_past_keys": (Case(p[:50], [0, 20, 51]), ("seg", 1))}
    for pos, (lo, hi) in (("first", (1, 2 * T)), ("middle", (T + 1, 2 * T)),
                          ("last", (2 * T - 1, 2 * T))):
        k = p.copy()
        k[0] = M64  # in front of the first record: not read
        k[lo] = 1 << 32
        k[hi] = (1 << 32) + 5
        out[f"wide_{pos}"] = (Case(k, [1, 9, 2 * T + 1]), ("wide", lo))
    return out


# ---- the scan ---------------------------------------------------------------------------------------
class ScanCase:
    """One record from its RecordIndex to its end (`data`), the filter (`keep`, indexed by Id),
    and what the case is there for."""

    def __init__(self, data, keep_ids, n_ids, want, tail=b""):
        self.data, self.tail = bytes(data), bytes(tail)  # tail: bytes behind the record's end
        self.keep = np.zeros(n_ids, np.uint8)
        for i in keep_ids:
            self.keep[i] = 1
        self.want = want

    def verdict(self):
        return am.scan_index_at(self.data, 0, len(self.data), self.keep)


def scan_plan(sc, phase, K=None):
    """verdict; the pieces (waves) the body spans when the index starts at 16-byte phase `phase`;
    where the deciding varint lies."""
    K = K or constants()
    d = sc.data
    v = sc.verdict()
    plan = dict(verdict=v, pieces=0, where=None)
    try:
        L, used = am.decode_varint(d, 0)
    except Exception:
        return plan
    if L == 0:
        return plan
    body = d[used:used + L - am.varint_len(L)]
    a0 = (phase + used) & ~15
    plan["pieces"] = -(-(phase + used + len(body) - a0) // K["piece"]) if body else 0
    plan["clipped"] = used + L - am.varint_len(L) > len(d)
    # the deciding varint
    p = 0
    while p < len(body):
        try:
            i, q = am.decode_varint(body, p)
        except Exception:
            break
        i &= 0xFFFFFFFF
        if i < len(sc.keep) and sc.keep[i]:
            break
        p = q
    if v != am.NONE:
        addr = phase + used + p - a0
        end = min(addr + 10, phase + used + len(body) - a0)
        plan["where"] = dict(piece=addr // K["piece"], step=addr // (64 * K["scan_block"]),
                             byte=(phase + used + p) % 16,
                             crosses_block=addr // 16 != (end - 1) // 16,
                             crosses_step=addr // 1024 != (end - 1) // 1024,
                             crosses_piece=addr // K["piece"] != (end - 1) // K["piece"])
    return plan


V = am.encode_varint


def wrap(body, claim=None):
    """varint(L) body, L the canonical length of `body` (or of `claim` body bytes)."""
    n = len(body) if claim is None else claim
    return V(am.len_wrapped_len(n)) + body


def scan_cases(K=None):
    """name -> ScanCase. Every case is run at each 16-byte phase of idx_off."""
    K = K or constants()
    P = K["piece"]
    out = {}
    N = 1 << 17

    def add(name, *a, **kw):
        assert name not in out
        out[name] = ScanCase(*a, **kw)

    ids = [3, 200, 70000, 5, 1 << 22, (1 << 29) + 1, 9]
    idx = am.record_index(ids)
    add("none", idx, [4, 6, 199], N, dict(verdict=am.NONE))
    add("match_first", idx, [3], N, dict(verdict=am.MATCH))
    add("match_last", idx, [9], N, dict(verdict=am.MATCH))
    add("match_wide_id", idx, [70000], N, dict(verdict=am.MATCH))
    add("count_is_walked", idx, [len(ids)], N, dict(verdict=am.MATCH))  # the quirk: count 7
    add("image_0200_kept", b"\x02\x00", [0], N, dict(verdict=am.MATCH))
    add("image_0200_not_kept", b"\x02\x00", [1], N, dict(verdict=am.NONE))
    add("id_truncated_to_u32", wrap(V(1) + V((1 << 32) + 5)), [5], N, dict(verdict=am.MATCH))
    add("id_past_n_ids", am.record_index([40, 41, 1 << 30]), [1, 39], 40, dict(verdict=am.NONE))
    add("no_ids_kept_at_all", idx, [], 0, dict(verdict=am.NONE))
    # index_len
    add("len_missing", b"", [0], N, dict(verdict=am.ERR_SHORT), tail=b"\x02\x00")
    add("len_cut", b"\x85\x80", [0], N, dict(verdict=am.ERR_SHORT), tail=b"\x00\x00")
    add("len_ten_continuations", b"\x80" * 10 + b"\x00", [0], N, dict(verdict=am.ERR_FORMAT))
    add("len_nine_continuations", b"\x80" * 9 + b"\x01" + b"\x00" * 4, [0], N,
        dict(verdict=am.MATCH, clipped=True))  # 2^63: a body clipped to 4 bytes, Id 0 kept
    add("len_zero", b"\x00\x00\x00", [0], N, dict(verdict=am.ERR_FORMAT))
    add("len_non_canonical_empty", b"\x81\x00\x00", [0], N, dict(verdict=am.NONE, pieces=0))
    add("len_non_canonical", b"\x85\x00" + V(2) + V(300) + b"\x07" + b"\x09", [9], N,
        dict(verdict=am.NONE))  # 5 - varint_len(5) = 4 body bytes behind the two consumed
    add("len_non_canonical_hit", b"\x85\x00" + V(2) + V(300) + b"\x07" + b"\x09", [7], N,
        dict(verdict=am.MATCH))
    # the body
    add("body_ends_in_varint", wrap(V(2) + V(5) + b"\x80\x80"), [9], N, dict(verdict=am.ERR_SHORT))
    add("body_clipped_at_varint_edge", wrap(V(3) + V(5) + V(300), claim=40), [9], N,
        dict(verdict=am.NONE, clipped=True), tail=V(9) * 40)
    add("body_clipped_inside_varint", wrap(V(3) + V(5) + b"\xac", claim=40), [9], N,
        dict(verdict=am.ERR_SHORT, clipped=True), tail=b"\x02" + V(9) * 40)
    add("body_nine_continuations", wrap(V(2) + b"\x85" + b"\x80" * 8 + b"\x00" + V(9)), [9], N,
        dict(verdict=am.MATCH))
    add("body_nine_continuations_value", wrap(V(2) + b"\x85" + b"\x80" * 8 + b"\x01" + V(8)), [5],
        N, dict(verdict=am.MATCH))  # 5 | 1 << 63, truncated
    add("body_ten_continuations", wrap(V(2) + b"\x85" + b"\x80" * 9 + b"\x00" + V(9)), [9], N,
        dict(verdict=am.ERR_FORMAT))
    add("body_eleven_continuations", wrap(V(2) + b"\x85" + b"\x80" * 10 + b"\x00" + V(9)), [9], N,
        dict(verdict=am.ERR_FORMAT))
    add("body_ten_continuations_at_end", wrap(V(2) + b"\x80" * 10), [9], N,
        dict(verdict=am.ERR_FORMAT))
    add("body_nine_continuations_at_end", wrap(V(2) + b"\x80" * 9), [9], N,
        dict(verdict=am.ERR_SHORT))
    add("hit_before_error", wrap(V(3) + V(9) + b"\x80" * 12), [9], N, dict(verdict=am.MATCH))
    add("error_before_hit", wrap(V(3) + b"\x80" * 12 + b"\x00" + V(9)), [9], N,
        dict(verdict=am.ERR_FORMAT))
    # a varint start at each byte of a block: k one-byte Ids, then the hit (every phase is run)
    for k in range(16):
        add(f"start_after_{k}", wrap(V(k + 1) + bytes([100] * k) + V(70001) + b"\x64" * 3), [70001],
            N, dict(verdict=am.MATCH))
    # long indexes: three-byte Ids, so that varints cross every block, step and piece edge
    wide = [(1 << 14) + 5 * i for i in range(2 * P // 3 + 50)]
    long_idx = am.record_index(wide)
    add("long_none", long_idx, [7], 1 << 15, dict(verdict=am.NONE, pieces=("min", 3)))
    add("long_hit_last", long_idx, [wide[-1]], 1 << 15,
        dict(verdict=am.MATCH, pieces=("min", 3), last_piece=True))
    for name, at in (("step_edge", 1024 // 3), ("piece_edge", P // 3)):
        for d in range(-3, 4):
            add(f"long_hit_{name}{d:+d}", long_idx, [wide[at + d]], 1 << 15, dict(verdict=am.MATCH))
    bad = bytearray(long_idx)
    cut = len(long_idx) - len(wide) * 3
    bad[cut + 3 * (P // 3 + 100):cut + 3 * (P // 3 + 104)] = b"\x80" * 12  # 10+ continuations
    add("long_hit_piece0_error_piece1", bytes(bad), [wide[10]], 1 << 15, dict(verdict=am.MATCH))
    add("long_error_piece1_hit_piece2", bytes(bad), [wide[-1]], 1 << 15,
        dict(verdict=am.ERR_FORMAT))
    return out


def scan_reaches(sc, K=None):
    """The case's `want` under every phase (where the want does not depend on the phase)."""
    K = K or constants()
    for phase in range(16):
        p = scan_plan(sc, phase, K)
        for k, v in sc.want.items():
            if k == "last_piece":
                if p["where"]["piece"] != p["pieces"] - 1:
                    return False
            elif isinstance(v, tuple):
                if p[k] < v[1]:
                    return False
            elif p.get(k) != v:
                return False
    return True


# ---- null arguments ---------------------------------------------------------------------------------
# name of the refused argument -> what to null in a call that is otherwise well-formed. The checks
# come before the ctx is looked at, so they are reached with any pointers (tests/
# test_archive_index_cpu.py: host arrays, no ctx) and with a ctx (tests/test_gpu_archive_index.py).
WRITER_NULLS = ["seg_off", "out", "out->idx_off", "out->idx_ids", "key", "tab->arch_id_of_sub"]
SCAN_NULLS = ["dbuf", "idx_off", "idx_end", "verdict", "keep"]


def raw_index_records(ctx, ptrs, null=None, n_keys=8, n_recs=2, n_subs=4):
    """nxg_archive_index_records through ctypes with the argument named `null` a null pointer.
    ptrs: key, seg_off, table, out, idx_off, idx_ids (addresses). Returns (ok, message)."""
    import ctypes as C
    import netidx_amd
    from netidx_amd import codec
    p = dict(ptrs)
    tab = codec.NxgRecordTable(n_subs, None if null == "tab->arch_id_of_sub" else p["table"])
    out = codec.NxgArchiveIndexes(64, p["out"], None if null == "out->idx_off" else p["idx_off"],
                                  None if null == "out->idx_ids" else p["idx_ids"], 0, 0)
    err = codec.NetidxError()
    ok = netidx_amd.lib().nxg_archive_index_records(
        ctx, None if null == "key" else p["key"], n_keys,
        None if null == "seg_off" else p["seg_off"], n_recs, C.byref(tab),
        None if null == "out" else C.byref(out), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    netidx_amd.lib().nxg_error_free(C.byref(err))
    return bool(ok), msg


def raw_scan_index(ctx, ptrs, null=None, n=1, n_ids=16, buf_len=64, off=(3,), end=(40,)):
    """nxg_archive_scan_index through ctypes with the argument named `null` a null pointer. ptrs:
    dbuf, keep (addresses). Returns (ok, message, verdict)."""
    import ctypes as C
    import netidx_amd
    from netidx_amd import codec
    o, e = np.array(off, np.uint64), np.array(end, np.uint64)
    verdict = np.full(max(n, 1), 0xEE, np.uint8)
    nm, err = C.c_uint64(0), codec.NetidxError()
    ok = netidx_amd.lib().nxg_archive_scan_index(
        ctx, None if null == "dbuf" else ptrs["dbuf"], buf_len,
        None if null == "idx_off" else o.ctypes.data, None if null == "idx_end" else e.ctypes.data,
        n, None if null == "keep" else ptrs["keep"], n_ids,
        None if null == "verdict" else verdict.ctypes.data, C.byref(nm), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    netidx_amd.lib().nxg_error_free(C.byref(err))
    return bool(ok), msg, verdict
