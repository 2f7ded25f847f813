"""GPU tests of the value table (nxg_value_table_init / _apply / _rebuild / _set_unsubscribed)
against the sequential model (tests/value_table_model.py). Every array of a table sits between
guard bands; after each call the arrays are read back and compared with the model's byte for byte
(rows, the written heap, the written children: the layout is a function of the call sequence),
rebuilt into trees and compared by identity, and the counters must equal the model's. A refused
call must name the model's slot and cause and leave every byte of the table as it was. The cases
and the branches they are there for are tests/value_table_cases.py's."""
import random
import struct

import numpy as np
import pytest

import subscribe_route_model as sm
import test_publish_values_cpu as P
import to_twin as tw
import value_table_cases as VC
from guards import SENTINEL
from value_table_model import (CAUSE_TEXT, OLD_SUFFIX, Capacity, Model, Refused, Source, sizes,
                               table_trees, NULL, ROW)

pytestmark = pytest.mark.gpu
SPARE = 512  # guard elements on both sides of every array


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


# ---- harness -----------------------------------------------------------------------------------
class Table:
    """A ValueTable whose arrays lie between SPARE sentinel elements, with its model."""

    def __init__(self, codec, n_slots, cap_bytes=0, cap_children=0, f64=False, init=True):
        import torch
        from netidx_amd.codec import ValueTable
        self.full, view = {}, {}
        caps = {"slots": n_slots, "bytes": cap_bytes, "children": cap_children}
        for name, dt, kind in ValueTable.ARRAYS:
            isz = {"uint8": 1, "int64": 8, "int32": 4}[dt]
            raw = torch.full(((2 * SPARE + caps[kind]) * isz,), SENTINEL, dtype=torch.uint8,
                             device="cuda")
            self.full[name] = raw
            view[name] = raw.view(getattr(torch, dt))[SPARE:]
        torch.cuda.synchronize()
        self.caps = caps
        self.vt = ValueTable(codec, n_slots, cap_bytes, cap_children, f64, tensors=view)
        assert self.vt.t["fixed"].data_ptr() % 16 == 0
        assert f64 or self.vt.t["heap"].data_ptr() % 16 == 0  # so heap_used is the 16-byte phase
        self.m = Model(n_slots, cap_bytes, cap_children, f64)
        if init:
            self.vt.init()

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        return ({k: v.cpu().numpy().tobytes() for k, v in self.full.items()
                 if self.vt.t[k] is not None}, self.vt.counters())

    def check_guards(self):
        from netidx_amd.codec import ValueTable
        for name, dt, kind in ValueTable.ARRAYS:
            if self.vt.t[name] is None:
                continue
            isz = {"uint8": 1, "int64": 8, "int32": 4}[dt]
            b = self.full[name].cpu().numpy()
            lo, hi = SPARE * isz, (SPARE + self.caps[kind]) * isz
            assert (b[:lo] == SENTINEL).all(), f"{name}: written in front of the array"
            bad = np.flatnonzero(b[hi:] != SENTINEL)
            assert not len(bad), f"{name}[{self.caps[kind] + int(bad[0]) // isz}] was written"

    def check(self):
        """The device table is the model's: arrays, trees, counters; guards intact."""
        vt, m = self.vt, self.m
        got, want = vt.numpy(), m.arrays()
        if m.f64:
            assert np.array_equal(got["fixed"], want["fixed"])
        else:
            assert vt.counters() == m.counters()
            for k in ("tag", "fixed", "aux", "heap", "ctag", "cfixed", "caux"):
                assert np.array_equal(got[k], want[k]), k
            assert table_trees(got, vt.heap_used, vt.child_used) == m.vals
        self.check_guards()


def dev(a, dt=None):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(dt) if dt is not None else a.copy()).cuda()
    torch.cuda.synchronize()
    return t


def batch_of(S):
    """(device Columns, device heap | None) of a Source, with its bounds as the counts."""
    import netidx_amd
    ids = np.zeros(len(S.fixed), np.uint64)
    kids = (S.ctag, S.cfixed, S.caux) if S.ctag is not None else (None, None, None)
    cols = netidx_amd.columns_from_arrays(ids, S.fixed, S.tag, S.aux, *kids)
    cols.s.n_rows, cols.s.n_children = S.n_rows, S.n_children
    heap = dev(np.frombuffer(S.heap, np.uint8)) if len(S.heap) else None
    return cols, heap, S.heap_len


def expect_refusal(call, e):
    from netidx_amd import CodecError
    with pytest.raises(CodecError) as g:
        call()
    msg = str(g.value)
    assert msg.startswith(f"slot {e.slot}: ") and CAUSE_TEXT[e.cause] in msg, (msg, e)
    assert msg.endswith(OLD_SUFFIX) == e.old, (msg, e)  # which value it was: the new or the held


def apply(tb, S, src_row, heap=None):
    """One apply on the device and in the model: the same result, or the same refusal with the
    table left as it was."""
    from netidx_amd.codec import ValueCapacity
    src_row = np.asarray(src_row, np.uint64)
    cols, dheap, heap_len = batch_of(S)
    drow = dev(src_row, np.int64)
    call = lambda: tb.vt.apply(cols, drow, dheap if heap is None else heap, heap_len)
    try:
        want = tb.m.apply(S, src_row)
    except (Refused, Capacity) as e:
        snap = tb.snapshot()
        if isinstance(e, Refused):
            expect_refusal(call, e)
        else:
            with pytest.raises(ValueCapacity) as g:
                call()
            assert (g.value.need_bytes, g.value.need_children, g.value.live_bytes,
                    g.value.live_children) == (e.need_bytes, e.need_children, e.live_bytes,
                                               e.live_children)
        assert tb.snapshot() == snap, "a refused call changed the table"
        return e
    got = call()
    if tb.m.f64:
        assert got["n_applied"] == want["n_applied"]
    else:
        assert got == want
    tb.check()
    return got


def rebuild(codec, tb, n_slots, cap_bytes, cap_children, S=None, src_row=None):
    """tb rebuilt into a fresh guarded table of these capacities (returned), or the refusal."""
    from netidx_amd.codec import ValueCapacity
    d = Table(codec, n_slots, cap_bytes, cap_children, tb.m.f64, init=False)
    cols, dheap, heap_len = batch_of(S) if S is not None else (None, None, 0)
    drow = dev(np.asarray(src_row, np.uint64), np.int64) if src_row is not None else None
    call = lambda: tb.vt.rebuild(d.vt, cols, drow, dheap, heap_len)
    src_snap = tb.snapshot()
    try:
        d.m, want = tb.m.rebuild(n_slots, cap_bytes, cap_children, S, src_row)
    except Capacity as e:
        snap = d.snapshot()
        with pytest.raises(ValueCapacity) as g:
            call()
        assert (g.value.need_bytes, g.value.need_children) == (e.need_bytes, e.need_children)
        assert d.snapshot() == snap and tb.snapshot() == src_snap
        return None
    except Refused as e:
        snap = d.snapshot()
        expect_refusal(call, e)
        assert d.snapshot() == snap and tb.snapshot() == src_snap
        return e
    got = call()
    assert tb.m.f64 or got == want
    d.check()
    assert tb.m.f64 or (d.vt.heap_used == d.vt.heap_live and d.vt.child_used == d.vt.child_live)
    assert tb.snapshot() == src_snap
    return d


# ---- an F64 table ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,branch", VC.slot_cases(VC.plan()))
def test_f64_table(codec, name, n, branch):
    rng = np.random.default_rng(n)
    tb = Table(codec, n, f64=True)
    tb.check()  # init: every slot 0
    rows = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    S = Source(None, rows, None)
    assert apply(tb, S, np.arange(n, 0, -1))["n_applied"] == n          # all, descending rows
    S2 = Source(None, rows[::-1].copy() ^ np.uint64(0xFF), None)
    sel = rng.permutation(n).astype(np.uint64) + 1
    sel[1::2] = 0
    assert apply(tb, S2, sel)["n_applied"] == (n + 1) // 2               # every other, random rows
    assert apply(tb, S2, np.zeros(n))["n_applied"] == 0                  # none
    # a MIXED batch of F64 rows is taken; one other tag is NXG_NOT_F64 and changes nothing
    M = VC.source_of([VC.f64(float(i)) for i in range(n)])
    apply(tb, M, rng.permutation(n) + 1)
    M.tag[n // 2] = 6
    e = apply(tb, M, np.arange(1, n + 1))
    assert isinstance(e, Refused) and e.slot == n // 2
    assert isinstance(apply(tb, S, np.full(n, n + 1)), Refused)          # a row past the batch
    d = rebuild(codec, tb, n + 3, 0, 0, S, np.where(np.arange(n) % 3 == 0, np.arange(n) + 1, 0))
    assert d.m.fixed[n:].tolist() == [0, 0, 0]


# ---- every kind of value -----------------------------------------------------------------------
def test_every_value_kind(codec):
    vals = VC.SCALARS + [v for v, _ in VC.VALUES.values()]
    n = len(vals)
    tb = Table(codec, n, 8192, 4096)
    tb.check()  # init: every slot Null
    S = VC.source_of(vals)
    apply(tb, S, np.arange(1, n + 1))
    apply(tb, S, np.arange(n, 0, -1))                # descending rows
    apply(tb, S, np.full(n, n - 2))                  # one nested row named by every slot
    # rows that share children: two Array rows over one child block
    S.fixed[0], S.tag[0], S.aux[0] = S.fixed[n - 1], S.tag[n - 1], S.aux[n - 1]
    apply(tb, S, np.where(np.arange(n) < 5, 1, n))
    # an F64-layout batch into a mixed table: tag 9, aux 0
    apply(tb, Source(None, np.arange(n, dtype=np.uint64) << np.uint64(52), None),
          np.arange(1, n + 1))
    assert tb.vt.heap_live == 0 and tb.vt.child_live == 0 and tb.vt.heap_used > 0


@pytest.mark.parametrize("phase", range(16))
def test_text_lengths_at_every_phase(codec, phase):
    p = VC.plan()
    vals = [VC.text(n, tag, n + tag) for tag in (12, 13, 18) for n in VC.TEXT_LENS]
    tb = Table(codec, len(vals) + 1, phase + sum(len(v[2]) for v in vals), 0)
    if phase:
        apply(tb, VC.source_of([VC.text(phase)]), [1] + [0] * len(vals))
    assert tb.vt.heap_used == phase
    lens = [len(v[2]) for v in vals if v[2]]
    wide, narrow = VC.copy_branch(p, 0, phase, lens)
    assert wide >= 3 * (100_000 // 16 - 1) and narrow >= 3  # both paths of the copy kernel
    apply(tb, VC.source_of(vals), [0] + list(range(1, len(vals) + 1)))
    assert tb.vt.heap_used == tb.caps["bytes"]  # filled to the last byte, the guard behind intact


def test_depth_limit(codec):
    tb = Table(codec, 2, 0, 80)
    S = VC.source_of([VC.nested(32), VC.nested(33)])
    apply(tb, S, [1, 0])
    e = apply(tb, S, [1, 2])
    assert isinstance(e, Refused) and e.slot == 1


def test_replacement_matrix(codec):
    kinds = [VC.f64(2.5), VC.text(21), VC.VALUES["array_strings"][0], VC.VALUES["nest3"][0]]
    pairs = [(a, b) for a in kinds for b in kinds]
    tb = Table(codec, len(pairs), 4096, 512)
    apply(tb, VC.source_of([a for a, _ in pairs]), np.arange(1, len(pairs) + 1))
    r = apply(tb, VC.source_of([b for _, b in pairs]), np.arange(1, len(pairs) + 1))
    assert r["live_bytes"] == sum(sizes(b)[0] for _, b in pairs)
    assert r["live_children"] == sum(sizes(b)[1] for _, b in pairs)
    # one at a time, back again: the live counts follow each replacement
    for s, (a, _) in enumerate(pairs):
        row = np.zeros(len(pairs), np.uint64)
        row[s] = 1
        apply(tb, VC.source_of([a]), row)


# ---- capacity and rebuild ----------------------------------------------------------------------
def test_capacity_then_rebuild(codec):
    v = ("arr", [VC.text(30), VC.text(10, 13)])
    S = VC.source_of([v, VC.text(7)])
    tb = Table(codec, 3, 100, 5)
    apply(tb, S, [1, 2, 0])           # 47 bytes, 2 children
    apply(tb, S, [1, 0, 0])           # 87 used / 47 live, 4 / 2
    e = apply(tb, S, [1, 0, 2])       # 47 more do not fit, though 54 live bytes would
    assert isinstance(e, Capacity) and (e.need_bytes, e.live_bytes) == (47, 54)
    assert (e.need_children, e.live_children) == (2, 2)
    assert rebuild(codec, tb, 3, e.live_bytes - 1, 8, S, [1, 0, 2]) is None   # dst too small
    assert rebuild(codec, tb, 3, e.live_bytes, 1, S, [1, 0, 2]) is None
    d = rebuild(codec, tb, 6, e.live_bytes + 40, 4, S, [1, 0, 2])
    assert d.m.vals == [v, VC.text(7), VC.text(7), NULL, NULL, NULL]
    apply(d, S, [0, 0, 0, 1, 0, 0])   # now it fits, to the last byte and child slot
    assert d.vt.heap_used == d.caps["bytes"] and d.vt.child_used == d.caps["children"]
    # pure compaction (no batch) of the table that was full
    c = rebuild(codec, tb, 3, 47, 2)
    assert c.m.vals == tb.m.vals and c.vt.counters() == (47, 47, 2, 2)


# ---- refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.REFUSALS))
def test_refusals_name_the_lowest_slot(codec, name):
    v, edit, cause = VC.REFUSALS[name]
    n = VC.plan()["block"] + 44
    tb = Table(codec, n, 8192, 512)
    good = VC.source_of([VC.text(9), VC.f64(1.0), VC.f64(2.0)])
    apply(tb, good, np.arange(n) % 3 + 1)
    for lo, hi in ((0, 5), (n // 2, n - 10), (n - 2, n - 1)):
        S = VC.source_of([v, v, VC.f64(3.0)])
        src_row = np.full(n, 3, np.uint64)
        src_row[lo], src_row[hi] = 2, 1
        if edit is not None:
            edit(S, 0)
            edit(S, 1)
        elif cause == ROW:
            src_row[lo], src_row[hi] = 4, 2 ** 40
        e = apply(tb, S, src_row)
        assert isinstance(e, Refused) and (e.slot, e.cause) == (lo, cause)
        apply(tb, good, (np.arange(n) + lo) % 3 + 1)  # the same ctx and table go on working


def edit_both(tb, field, idx, val):
    """One element of the table's arrays, in the model and on the device (through the tensor: a
    table is its caller's memory)."""
    import torch
    arr = getattr(tb.m, field)
    was = int(arr[idx])
    arr[idx] = val
    tb.vt.t[field][idx] = val
    torch.cuda.synchronize()
    return was


@pytest.mark.parametrize("name", list(VC.OLD_REFUSALS))
def test_refusals_of_a_value_the_table_holds(codec, name):
    """A slot whose held value is out of range (edited in place) refuses the apply that replaces
    it, the rebuild that carries it over and the set_unsubscribed that drops it: the lowest such
    slot, its cause, the suffix that says it is the held value, nothing changed; once the arrays
    are put back the same calls work."""
    from netidx_amd import CodecError
    v, edit, cause = VC.OLD_REFUSALS[name]
    n = VC.plan()["block"] + 44
    tb = Table(codec, n, 8192, 1024)
    good = VC.source_of([v, VC.f64(1.0), VC.f64(2.0)])
    apply(tb, good, np.where(np.arange(n) % 7 == 0, 1, np.arange(n) % 2 + 2))
    holders = [s for s in range(n) if s % 7 == 0]
    for lo, hi in ((holders[0], holders[1]), (holders[len(holders) // 2], holders[-2]),
                   (holders[-2], holders[-1])):
        undo = []
        for s in (hi, lo):
            field, idx, val = edit(tb.m, s)
            undo.append((field, idx, edit_both(tb, field, idx, val)))
        src_row = np.zeros(n, np.uint64)
        src_row[lo], src_row[hi], src_row[1] = 2, 3, 1
        e = apply(tb, good, src_row)                      # the replaced value is walked
        assert isinstance(e, Refused) and (e.slot, e.cause, e.old) == (lo, cause, True)
        e = rebuild(codec, tb, n + 1, 8192, 1024)         # a value carried over is walked
        assert isinstance(e, Refused) and (e.slot, e.cause, e.old) == (lo, cause, True)
        snap = tb.snapshot()
        with pytest.raises(Refused) as m:
            tb.m.set_unsubscribed([hi, lo, hi, 1])
        assert (m.value.slot, m.value.cause, m.value.old) == (lo, cause, True)
        expect_refusal(lambda: tb.vt.set_unsubscribed([hi, lo, hi, 1]), m.value)
        assert tb.snapshot() == snap
        for field, idx, was in reversed(undo):
            edit_both(tb, field, idx, was)
        assert not isinstance(apply(tb, good, src_row), Exception)   # the same call, clean
        assert rebuild(codec, tb, n + 1, 8192, 1024).m.vals[:n] == tb.m.vals
        apply(tb, good, np.where(np.arange(n) % 7 == 0, 1, 0))       # the holders hold v again


def test_source_layout_does_not_matter(codec):
    """A batch whose child blocks are not in preorder and whose payloads are not packed: the
    table's arrays are the canonical ones all the same (the model reads trees and writes them
    as Layout does)."""
    vals = [VC.VALUES[k][0] for k in ("nest3", "nest_map_of_arrays", "array_strings", "map")]
    vals += [VC.nested(5, VC.text(7)), VC.text(33), VC.dec(5)]
    S, C = VC.scrambled_source(vals), VC.source_of(vals)
    assert not np.array_equal(S.ctag, C.ctag) and S.heap != C.heap and len(S.ctag) == len(C.ctag)
    a, b = Table(codec, len(vals), 1024, 256), Table(codec, len(vals), 1024, 256)
    order = np.arange(len(vals), 0, -1)
    apply(a, S, order)
    apply(b, C, order)
    assert a.snapshot() == b.snapshot()  # byte for byte what the canonical source gives
    d = rebuild(codec, a, len(vals), 1024, 256, S, np.arange(1, len(vals) + 1))
    assert d.m.vals == vals


def test_encode_out_of_the_table(codec):
    """commit -> encode -> apply -> next commit: the table's rows, children and heap are
    nxg_encode_updates' input as they are (as_columns), after two applies have moved them."""
    import torch
    vals = [("txt", 12, b"hello"), ("txt", 12, b""), VC.dec(15, 1), VC.ABSTRACT, ("txt", 18, b"e"),
            ("arr", [("txt", 12, b"ab"), VC.f64(2.0), ("arr", [("txt", 12, b"deep"), VC.dec(2)])]),
            ("map", [(("sc", 6, 1, 0), ("txt", 13, bytes(range(200, 230))))]),
            ("err", ("txt", 12, b"bad")), ("err", ("arr", [])), VC.f64(-0.0), ("sc", 6, VC.I64 - 5, 0),
            ("sc", 14, 0, 0), ("arr", []), VC.nested(32)]
    n = len(vals)
    tb = Table(codec, n, 1024, 256)
    apply(tb, VC.source_of(vals), np.arange(1, n + 1))
    apply(tb, VC.source_of(vals), (np.arange(n) + 5) % n + 1)
    ids = np.arange(n, dtype=np.int64) * 1000 + 7
    cols = tb.vt.as_columns(dev(ids))
    wire = codec.encode_batch(cols, tb.vt.t["heap"])
    mg = tw.mg()
    want = b"".join(mg.update(int(i), golden(v)) for i, v in zip(ids, tb.m.vals))
    assert wire.cpu().numpy().tobytes() == want
    back, st = codec.decode_batch(wire)  # and the frame decodes to the same rows
    assert st.n_rows == n


def test_misuse_is_refused_on_the_host(codec):
    from netidx_amd import CodecError
    tb = Table(codec, 4, 64, 4)
    cols, heap, _ = batch_of(VC.source_of([VC.text(3)]))
    snap = tb.snapshot()
    with pytest.raises(CodecError, match="overlaps"):   # src_row inside the table's own arrays
        tb.vt.apply(cols, tb.vt.t["fixed"], heap)
    with pytest.raises(CodecError, match="overlaps"):   # a heap that is the table's
        tb.vt.apply(cols, dev(np.zeros(4, np.uint64), np.int64), tb.vt.t["heap"], 8)
    with pytest.raises(CodecError, match="null"):
        tb.vt.apply(cols, None, heap)
    with pytest.raises(CodecError, match="slots"):      # dst smaller than src
        tb.vt.rebuild(Table(codec, 3, 64, 4, init=False).vt)
    assert tb.snapshot() == snap


# ---- determinism, and a table past one step of the top scan ------------------------------------
def test_same_calls_same_bytes(codec):
    def run():
        rng = random.Random(77)
        tb = Table(codec, 300, 1 << 16, 1 << 14)
        for _ in range(3):
            vals = [P.rand_value(rng) for _ in range(200)]
            row = [rng.randrange(201) for _ in range(300)]
            apply(tb, VC.source_of(vals), row)
        return tb.snapshot()
    assert run() == run()


def test_second_step_of_the_top_scan(codec):
    p = VC.plan()
    n = VC.top_step_slots(p)
    assert VC.slots_branch(p, n)[1] == 2
    tb = Table(codec, n, 4096, 64)
    vals = [VC.VALUES["nest3"][0], VC.text(33), VC.VALUES["array_strings"][0]]
    row = np.zeros(n, np.uint64)
    B, T = p["block"], p["top"]
    for k, s in enumerate((0, B - 1, B * (T - 1) + 7, B * T - 1, B * T)):
        row[s] = k % 3 + 1
    apply(tb, VC.source_of(vals), row)
    apply(tb, VC.source_of(vals), np.roll(row, -1)[::-1].copy())


# ---- the publisher's chain ---------------------------------------------------------------------
def golden(v):
    k = v[0]
    if k == "sc":
        t, f = v[1], v[2]
        return (t, None) if t in (14, 15, 16) else (t, f - (1 << 64) if t == 6 and f >> 63 else f)
    if k == "txt":
        return (v[1], v[2])
    if k == "dec":
        return (20, v[1])
    if k == "arr":
        return (19, [golden(x) for x in v[1]])
    if k == "map":
        return (21, [(golden(a), golden(b)) for a, b in v[1]])
    return (22, golden(v[1]))


def has_17(v):
    if v[0] == "sc":
        return v[1] == 17
    return v[0] in ("arr", "map", "err") and any(has_17(x) for x in
                                                 (v[1] if v[0] == "arr" else
                                                  [y for kv in v[1] for y in kv] if v[0] == "map"
                                                  else [v[1]]))


def test_publisher_chain(codec):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns, PathTable, SubscribeTable, WriteCols, _value_len
    rng = random.Random(5)
    n_ids, n_rows, n_clients = 40, 60, 4
    rows, kind, to_client, by_id, slot_ids = P.random_case(rng, n_rows, n_ids, n_clients)
    slot_of = {i: s for s, i in enumerate(slot_ids)}
    n = len(slot_ids)
    tb = Table(codec, n, 1 << 16, 1 << 12)
    apply(tb, VC.source_of([by_id[i][1] for i in slot_ids]), np.arange(1, n + 1))
    pushed_equal = twins_dropped = 0
    for step in range(5):
        if step:
            # rows that equal the current value under Value::eq but not bitwise among them
            twins = {("sc", 9, 0, 0): VC.f64(-0.0), VC.f64(-0.0): ("sc", 9, 0, 0),
                     VC.f64(float("nan")): ("sc", 9, 0xFFF8000000000001, 0)}
            rows, twin_rows = [], set()
            for _ in range(n_rows):
                i = rng.randrange(n_ids + 1)
                v = P.rand_value(rng)
                if i in by_id and rng.random() < 0.4:
                    c = by_id[i][1]
                    v = (twins.get(c, c) if c[0] == "sc" else
                         ("dec", P.DECIMALS[3]) if c == ("dec", P.DECIMALS[2]) else c)
                    if v != c:  # equal under Value::eq, other bits
                        twin_rows.add(len(rows))
                rows.append((i, v))
            kind = [rng.choice([0, 1, 1, 1, 2]) for _ in range(n_rows)]
            to_client = [rng.randrange(n_clients + 1) for _ in range(n_rows)]
        want, became = P.commit(rows, kind, to_client, by_id, n_clients)
        a = P.case_arrays(rows, kind, to_client, by_id, slot_ids, n_ids)
        ct, cf, ca = a["children"]
        batch = netidx_amd.columns_from_arrays(a["ids"], a["fixed"], a["tag"], a["aux"], ct, cf, ca)
        heap = dev(a["heap"])
        pub = tb.vt.pub_table(a["soi"], a["off"], a["cl"], n_clients)
        d = codec.publish_commit(pub, batch, dev(a["kind"]), dev(a["to"], np.int32), heap=heap)
        got = {c: list(zip(*[x[int(d.chan_off[c]):int(d.chan_off[c + 1])].cpu().numpy()
                             .view(np.uint64).tolist() for x in (d.ent_sub, d.ent_row)]))
               for c in range(n_clients) if int(d.chan_off[c + 1]) > int(d.chan_off[c])}
        assert got == want  # the commit read `current` out of the table
        last = d.last_row.cpu().numpy().view(np.uint64)
        assert {slot_ids[s]: int(last[s]) - 1 for s in range(n) if last[s]} == became
        # apply(last_row), on the device array as it is
        S = Source(a["tag"], a["fixed"], a["aux"], ct, cf, ca, bytes(a["heap"][:-1]))
        res = tb.m.apply(S, last)
        assert tb.vt.apply(batch, d.last_row, heap, len(S.heap)) == res
        tb.check()
        for idv, r in became.items():
            by_id[idv][1] = rows[r][1]
        assert tb.m.vals == [by_id[i][1] for i in slot_ids]
        sent = {r for v in want.values() for _, r in v}
        dropped = [i for i, k in enumerate(kind) if k == 1 and rows[i][0] in by_id
                   and i not in sent]
        pushed_equal += len(dropped)
        if step:
            # a twin still equal to `current` when its turn came (no row of its Id in front of
            # it in this batch) and with subscribers: dropped only if the table held the value
            first = {}
            for i, (idv, _) in enumerate(rows):
                first.setdefault(idv, i)
            twins_dropped += sum(1 for i in dropped if i in twin_rows and first[rows[i][0]] == i)
    assert pushed_equal  # UpdateChanged rows were dropped as equal to what the table held
    assert twins_dropped  # ... among them rows equal under Value::eq but not bitwise
    # Subscribed replies out of the table, for every Id whose value has no tag 17
    ids = [i for i in slot_ids if not has_17(by_id[i][1])]
    paths = [b"/v/%d" % i for i in ids]
    wire = b"".join(tw.subscribe(p, timestamp=k, permissions=0, token=b"")
                    for k, p in enumerate(paths))
    frame = dev(np.frombuffer(wire, np.uint8))
    cols = Columns(len(wire) // 5 + 1, len(wire) + 1, len(wire) // 3 + 1,
                   netidx_amd.LAYOUT_MIXED, "cuda")
    codec.decode_writes(frame, cols, WriteCols(len(wire) // 5 + 1, "cuda"))
    pt = PathTable(codec, len(paths), sum(len(p) for p in paths))
    pt.insert(paths, ids)
    soi = np.full(n_ids, netidx_amd.NO_SLOT, np.uint32)
    for i in slot_ids:
        soi[i] = slot_of[i]
    pub = tb.vt.pub_table(soi, [0] * (n + 1), [], 0)
    mv = max(_value_len(golden(by_id[i][1])) for i in ids)
    r = codec.route_subscribes(SubscribeTable(pt, pub, max_value_len=mv), frame, cols)
    want = b"".join(sm.subscribed(p, i, golden(by_id[i][1])) for p, i in zip(paths, ids))
    assert r.numpy()["reply"] == want and r.n_sub == len(ids)


# ---- the subscriber's chain --------------------------------------------------------------------
def test_subscriber_chain(codec):
    import torch
    import netidx_amd
    from netidx_amd.codec import SubTable
    def ascii_text(n):  # a String must be UTF-8 to pass the decoder
        return ("txt", 12, bytes(97 + (3 * i + n) % 26 for i in range(n)))
    vals = [ascii_text(n) for n in (5, 0, 40, 17)] + [VC.f64(1.5), VC.dec(15, 1),
                                                       VC.text(300, 13), ("sc", 6, 7, 0)]
    vals = vals * 3
    n_ids = 10
    ids = np.array([(7 * k) % (n_ids + 1) for k in range(len(vals))], np.uint64)  # Id 10: none
    S = VC.source_of(vals)
    cols0 = netidx_amd.columns_from_arrays(ids, S.fixed, S.tag, S.aux)
    wire = codec.encode_batch(cols0, dev(np.frombuffer(S.heap, np.uint8)))
    W = wire.numel()
    cols, st = codec.decode_batch(wire)
    assert st.n_rows == len(vals)
    subs = {i: (100 + i, [i % 2], i % 3 != 0) for i in range(n_ids)}  # slot_has_last mixed
    table = SubTable.from_subscriptions(subs, 2, n_ids)
    d = codec.dispatch_updates(table, cols.id, len(vals))
    last = d.last_row.cpu().numpy().view(np.uint64)
    want_last = np.zeros(n_ids, np.uint64)
    for r, i in enumerate(ids.tolist()):
        if i < n_ids and subs[i][2]:
            want_last[i] = r + 1
    assert np.array_equal(last, want_last) and (want_last == 0).any() and want_last.any()
    tb = Table(codec, n_ids, 2048, 0)
    h = cols.numpy()
    F = Source(h["tag"][:len(vals)], h["fixed"][:len(vals)], h["aux"][:len(vals)],
               heap=wire.cpu().numpy().tobytes())
    want = tb.m.apply(F, last)
    assert tb.vt.apply(cols, d.last_row, wire, W) == want
    wire.fill_(0xAA)  # the frame buffer is reused: the table owns its bytes
    torch.cuda.synchronize()
    tb.check()
    assert tb.m.vals == [vals[int(r) - 1] if r else NULL for r in want_last]
    # Event::Unsubscribed, after the apply: a slot named twice counts once
    live = tb.vt.counters()
    drop = [4, 1, 4, 2]
    tb.m.set_unsubscribed(drop)
    tb.vt.set_unsubscribed(drop)
    tb.check()
    assert tb.vt.heap_live < live[1] and tb.vt.heap_used == live[0]
    snap = tb.snapshot()
    with pytest.raises(Refused) as e:
        tb.m.set_unsubscribed([3, n_ids + 2, n_ids])
    expect_refusal(lambda: tb.vt.set_unsubscribed([3, n_ids + 2, n_ids]), e.value)
    assert tb.snapshot() == snap
