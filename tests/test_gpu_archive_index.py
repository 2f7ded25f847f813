"""GPU tests of nxg_archive_index_records and nxg_archive_scan_index against
tests/archive_index_model.py, byte for byte, over the cases of tests/archive_index_cases.py. `out`,
`idx_off` and `idx_ids` lie between guard bands. A refused call names what the model names and
leaves every byte of `out` as it was, and the ctx works afterwards.

Not run: the MAX_VEC refusal (count * 4 > MAX_VEC) needs 2^29 + 1 distinct Ids in one record."""
import json
import os
import types

import numpy as np
import pytest

import archive_index_cases as ac
import archive_index_model as am
import guards
from guards import SENTINEL

pytestmark = pytest.mark.gpu
SPARE = 512
K = ac.constants()
CASES = ac.cases(K)
REFUSALS = ac.refusal_cases(K)
SCANS = ac.scan_cases(K)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_want = {}


def want_of(name):
    """(blob, idx_off, idx_ids) of a case, computed once."""
    if name not in _want:
        _want[name] = am.expected(CASES[name][0])
    return _want[name]


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


# ---- harness -----------------------------------------------------------------------------------
def dev(a, dt=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(0, dtype=getattr(torch, np.dtype(dt or a.dtype).name), device="cuda")
    t = torch.from_numpy(a.view(dt) if dt is not None else a.copy()).cuda()
    torch.cuda.synchronize()
    return t


def guarded_words(n):
    """n int64 elements between SPARE sentinel elements: (whole tensor, the n in the middle)."""
    import torch
    raw = torch.full(((2 * SPARE + n) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return raw, raw.view(torch.int64)[SPARE:SPARE + n]


def words_guards_ok(raw, n, name):
    b = raw.cpu().numpy()
    assert (b[:SPARE * 8] == SENTINEL).all(), f"{name}: written in front of the array"
    assert (b[(SPARE + n) * 8:] == SENTINEL).all(), f"{name}: written behind its {n} elements"


class Call:
    """One writer case on the device: its keys, records and table, uploaded once."""

    def __init__(self, case):
        self.case = case
        self.key = dev(case.key, np.int64)
        self.seg_off = dev(case.seg_off, np.int64)
        self.table = None if case.table is None else dev(case.table, np.int32)
        self.n_recs = case.n_recs
        self.n_keys = None

    def run(self, codec, cap=None, phase=0, size_only=False):
        """(n_bytes, idx_off, idx_ids, n_ids_total, out bytes | None). `cap`: the capacity stated.
        Guards checked in every outcome."""
        import torch
        from netidx_amd import CodecError
        nr = self.n_recs
        raw_off, idx_off = guarded_words(nr + 1)
        raw_ids, idx_ids = guarded_words(nr)
        buf = None if size_only else guards.guarded_buffer(cap, phase)
        ptr = None if size_only else guards.out_ptr(buf, phase)
        try:
            r = codec.index_records_into(self.key, self.seg_off, self.table, ptr,
                                         0 if size_only else cap, idx_off, idx_ids, self.n_keys)
            failed = None
        except CodecError as e:
            r, failed = None, e
        torch.cuda.synchronize()
        words_guards_ok(raw_off, nr + 1, "idx_off")
        words_guards_ok(raw_ids, nr, "idx_ids")
        if buf is not None:
            guards.assert_outside_untouched(buf, phase, cap)
        if failed is not None:
            if buf is not None:
                assert (guards.written(buf, phase, cap) == SENTINEL).all(), \
                    "a refused call wrote to out"
            failed.idx_off_host = idx_off.cpu().numpy().view(np.uint64)
            failed.idx_ids_host = idx_ids.cpu().numpy().view(np.uint64)
            raise failed
        n, off, ids, total = r
        got = None if size_only else guards.written(buf, phase, cap)[:n].tobytes()
        return (n, off.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64), total, got)


def check_equal(res, want):
    blob, idx_off, idx_ids = want
    n, off, ids, total, got = res
    assert n == len(blob)
    assert np.array_equal(off, idx_off)
    assert np.array_equal(ids, idx_ids)
    assert total == int(idx_ids.sum())
    if got is not None:
        assert got == blob


# ---- the writer: every case -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_case_matches_model(codec, name):
    want = want_of(name)
    call = Call(CASES[name][0])
    phase = sum(name.encode()) % 16
    sized = call.run(codec, size_only=True)
    check_equal(sized, want)
    first = call.run(codec, cap=len(want[0]), phase=phase)  # the capacity exact
    check_equal(first, want)
    again = call.run(codec, cap=len(want[0]), phase=phase)
    check_equal(again, want)
    assert again[4] == first[4], "a rerun differs"


@pytest.mark.parametrize("name", ["id_widths", "tile+1", "recs1000"])
def test_out_at_each_16_byte_phase(codec, name):
    want = want_of(name)
    call = Call(CASES[name][0])
    for phase in range(16):
        check_equal(call.run(codec, cap=len(want[0]) + phase % 3, phase=phase), want)


@pytest.mark.parametrize("name", ["recs1000", "inner_16382", "table"])
def test_capacity_one_short(codec, name):
    from netidx_amd import CodecError
    want = want_of(name)
    call = Call(CASES[name][0])
    with pytest.raises(CodecError) as g:  # (run() checks that out is all sentinel)
        call.run(codec, cap=len(want[0]) - 1, phase=5)
    assert "output buffer too small" in str(g.value) and str(len(want[0])) in str(g.value)
    assert g.value.n_bytes == len(want[0])
    assert np.array_equal(g.value.idx_off_host, want[1])
    assert np.array_equal(g.value.idx_ids_host, want[2])
    check_equal(call.run(codec, cap=len(want[0]), phase=5), want)


def test_smaller_call_after_a_larger_one(codec):
    """The table is sized per call and cleared per call: a small call after a large one, and the
    large one again."""
    for name in ("top+1", "n1", "table_collide_wrap", "top+1"):
        check_equal(Call(CASES[name][0]).run(codec, cap=len(want_of(name)[0])), want_of(name))


def test_keys_behind_the_records_are_not_read(codec):
    """n_keys states fewer positions than the tensor holds."""
    case = CASES["tile+1"][0]
    call = Call(am.Case(np.concatenate([case.key, np.full(700, 1 << 40, np.uint64)]), case.seg_off))
    call.n_keys = case.n_keys
    check_equal(call.run(codec, cap=len(want_of("tile+1")[0])), want_of("tile+1"))


# ---- the writer: refusals ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_names_the_lowest_and_writes_nothing(codec, name):
    from netidx_amd import CodecError
    case, what = REFUSALS[name]
    assert am.refusal(case) == what
    call = Call(case)
    for size_only in (True, False):
        with pytest.raises(CodecError) as g:
            call.run(codec, cap=1 << 16, phase=3, size_only=size_only)
        msg = str(g.value)
        if what[0] == "wide":
            assert msg.startswith(f"position {what[1]}: Id {int(case.key[what[1]])} ") and \
                "2^32" in msg, msg
        else:
            assert f"at record {what[1]}:" in msg and "seg_off" in msg, msg
    check_equal(Call(CASES["block+1"][0]).run(codec, cap=len(want_of("block+1")[0])),
                want_of("block+1"))


def test_writer_misuse(codec):
    from netidx_amd import CodecError
    from netidx_amd import synth
    from netidx_amd.codec import Columns, LAYOUT_F64
    import netidx_amd
    case = CASES["table"][0]
    want = want_of("table")
    call = Call(case)

    def refused(word, **kw):
        c = types.SimpleNamespace(**{**call.__dict__, **kw})
        with pytest.raises(CodecError) as g:
            Call.run(c, codec, cap=len(want[0]))
        assert word in str(g.value), str(g.value)

    refused("device memory", key=call.key.cpu())
    refused("device memory", seg_off=call.seg_off.cpu())
    refused("device memory", table=call.table.cpu())
    refused("too many positions", n_keys=(1 << 28) + 1)
    # async work pending on the ctx
    ids, vals = synth.f64_columns(100)
    wire = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    out = Columns(100, 0, 0, LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), out)
    refused("pending")
    codec.sync()
    check_equal(call.run(codec, cap=len(want[0])), want)


@pytest.mark.parametrize("null", ac.WRITER_NULLS)
def test_writer_null_argument_then_a_clean_call(codec, null):
    """Each null argument alone, with a live ctx and device memory everywhere else."""
    import torch
    t = {k: torch.zeros(64, dtype=torch.int64, device="cuda")
         for k in ("key", "seg_off", "table", "out", "idx_off", "idx_ids")}
    t["seg_off"][1:3] = 8
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ok, msg = ac.raw_index_records(codec.ctx, ptrs, null)
    assert not ok and msg == f"null argument ({null})", msg
    assert all(int(v.abs().sum()) == (16 if k == "seg_off" else 0) for k, v in t.items())
    ok, msg = ac.raw_index_records(codec.ctx, ptrs)  # the same arguments, none null
    assert ok, msg
    assert t["idx_ids"][:2].tolist() == [1, 0] and t["idx_off"][:3].tolist() == [0, 3, 3]
    assert t["out"].view(torch.uint8)[:3].tolist() == [3, 1, 0]
    check_equal(Call(CASES["block+1"][0]).run(codec, cap=len(want_of("block+1")[0])),
                want_of("block+1"))


def test_no_records_or_no_keys(codec):
    import torch
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    n, off, ids, total = codec.index_records_into(z, dev(np.array([0], np.uint64), np.int64), None,
                                                  None, 0)
    assert (n, total) == (0, 0) and off.cpu().tolist() == [0]
    n, off, ids, total = codec.index_records_into(z, dev(np.zeros(4, np.uint64), np.int64), None,
                                                  None, 0)
    assert (n, total) == (0, 0) and off.cpu().tolist() == [0] * 4 and ids.cpu().tolist() == [0] * 3


# ---- the chain: decode -> dispatch -> record_entries + index_records --------------------------------
def test_decode_dispatch_record_and_index(codec):
    """Each channel's index holds exactly the Ids of the items nxg_decode_archive_batch reads back
    from the record nxg_record_entries wrote for it, in order of first occurrence."""
    from netidx_amd import synth
    from netidx_amd.codec import Columns, HINT_MIXED, LAYOUT_MIXED, SubTable
    import netidx_amd
    n, n_chans = 5000, 7
    m = synth.mixed_columns(n)
    mc = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
    frame = codec.encode_batch(mc, dev(m.heap))
    cols = Columns.for_frame(frame.numel(), LAYOUT_MIXED, "cuda")
    codec.decode_into(frame, frame.numel(), cols, flags=HINT_MIXED)
    rng = np.random.default_rng(11)
    subs = {int(i): (int(3 * i + 1), [int(x) for x in rng.integers(0, n_chans, rng.integers(0, 4))],
                     True) for i in rng.choice(n, n * 3 // 4, replace=False)}
    disp = codec.dispatch_updates(SubTable.from_subscriptions(subs, n_chans, n), cols.id, n)
    # several SubIds share an archive Id, so records repeat Ids
    arch = np.where(np.arange(3 * n + 2) % 5 == 0, am.NO_SLOT, np.arange(3 * n + 2) % 900 * 7)
    table = dev(arch.astype(np.uint32), np.int32)
    got, off, items, _ = codec.record_entries(cols, disp, table, frame)
    ne = int(disp.n_entries)
    idx, ioff, iids = codec.index_records(disp.ent_sub[:ne], disp.chan_off, table)
    off, ioff = off.cpu().tolist(), ioff.cpu().tolist()
    idx = idx.cpu().numpy().tobytes()
    repeats = 0
    for c in range(n_chans):
        rec = got[off[c]:off[c + 1]]
        mine = idx[ioff[c]:ioff[c + 1]]
        if not rec.numel():
            assert mine == b"" and int(iids[c]) == 0
            continue
        out = Columns(int(items[c]), rec.numel(), 0, LAYOUT_MIXED, "cuda")
        st, _ = codec.decode_archive(rec.contiguous(), rec.numel(), out)
        ids = [int(x) for x in out.numpy()["id"][:st.n_rows]]
        order = list(dict.fromkeys(ids))
        repeats += len(ids) - len(order)
        assert mine == am.record_index(order) and int(iids[c]) == len(order)
    assert repeats > 0


# ---- the scan ---------------------------------------------------------------------------------------------
def laid_out(chunks):
    """(device buffer, offs, ends): record i is chunks[i] = (phase, data, tail), its index placed
    at the 16-byte phase asked for, its tail right behind its end."""
    buf, offs, ends = bytearray(b"\xee" * 256), [], []
    for phase, data, tail in chunks:
        buf += b"\xee" * (-len(buf) % 16 + phase)
        offs.append(len(buf))
        buf += data
        ends.append(len(buf))
        buf += tail + b"\x85" * 24
    return dev(np.frombuffer(bytes(buf), np.uint8)), offs, ends


@pytest.mark.parametrize("name", sorted(SCANS))
def test_scan_case_at_each_16_byte_phase(codec, name):
    sc = SCANS[name]
    dbuf, offs, ends = laid_out([(ph, sc.data, sc.tail) for ph in range(16)])
    assert [o % 16 for o in offs] == list(range(16)) and dbuf.data_ptr() % 16 == 0
    keep = dev(sc.keep) if len(sc.keep) else None
    verdict, n_match = codec.scan_index(dbuf, offs, ends, keep)
    want = sc.verdict()
    assert verdict.tolist() == [want] * 16
    assert n_match == (16 if want == am.MATCH else 0)


def test_scan_many_records_one_call(codec):
    """Every case that shares the small filter, shuffled into one call, twice."""
    names = [n for n in sorted(SCANS) if len(SCANS[n].keep) == 1 << 17 and
             SCANS[n].keep.sum() == 1 and SCANS[n].keep[9]]
    assert len(names) >= 10
    rng = np.random.default_rng(3)
    order = [names[i] for i in rng.permutation(np.repeat(np.arange(len(names)), 40))]
    dbuf, offs, ends = laid_out([(int(rng.integers(0, 16)), SCANS[n].data, SCANS[n].tail)
                                 for n in order])
    want = [SCANS[n].verdict() for n in order]
    keep = dev(SCANS[names[0]].keep)
    for _ in range(2):
        verdict, n_match = codec.scan_index(dbuf, offs, ends, keep)
        assert verdict.tolist() == want and n_match == want.count(am.MATCH)


def test_scan_golden_indexed_records(codec):
    m = json.load(open(os.path.join(G, "zstd_manifest.json")))["records"]
    rec = open(os.path.join(G, "zstd_records.bin"), "rb").read()
    ents = [e for e in m if e["indexed"]]
    dbuf = dev(np.frombuffer(rec, np.uint8))
    offs = [e["rec_off"] + 4 for e in ents]
    ends = [e["rec_off"] + e["rec_len"] for e in ents]
    rng = np.random.default_rng(8)
    for frac in (0.0, 0.002, 0.05, 1.0):
        keep = (rng.random(1 << 16) < frac).astype(np.uint8)
        want = [am.scan_index_at(rec, o, e, keep) for o, e in zip(offs, ends)]
        verdict, n_match = codec.scan_index(dbuf, offs, ends, dev(keep))
        assert verdict.tolist() == want and n_match == want.count(am.MATCH)
    assert len(set(want)) == 1 and want[0] == am.MATCH


def test_written_indexes_select_the_model_s_records(codec):
    """Indexes written by nxg_archive_index_records, scanned where they lie by
    nxg_archive_scan_index, select exactly the records the model selects."""
    case = CASES["recs1000"][0]
    idx, ioff, _ = codec.index_records(dev(case.key, np.int64), dev(case.seg_off, np.int64))
    host = idx.cpu().numpy().tobytes()
    assert host == want_of("recs1000")[0]
    ioff = ioff.cpu().tolist()
    offs, ends = ioff[:-1], ioff[1:]
    for pick in ([3], [17, 250], list(range(0, 300, 7)), []):
        keep = np.zeros(300, np.uint8)
        keep[pick] = 1
        want = [am.scan_index_at(host, o, e, keep) for o, e in zip(offs, ends)]
        verdict, n_match = codec.scan_index(idx, offs, ends, dev(keep), buf_len=len(host))
        assert verdict.tolist() == want and n_match == want.count(am.MATCH)
        # a record without an index has no bytes to scan: BufferShort, as in the reference
        assert {v for v, o, e in zip(want, offs, ends) if o == e} <= {am.ERR_SHORT}
        assert (want.count(am.MATCH) > 0) == bool(pick)


def test_scan_misuse(codec):
    from netidx_amd import CodecError
    sc = SCANS["none"]
    dbuf, offs, ends = laid_out([(3, sc.data, sc.tail)])
    keep = dev(sc.keep)
    n = dbuf.numel()
    for word, args in (("device", (dbuf.cpu(), offs, ends, keep)),
                       ("device", (dbuf, offs, ends, keep.cpu())),
                       ("not a range", (dbuf, [ends[0] + 1], ends, keep)),
                       ("not a range", (dbuf, offs, [n + 1], keep))):
        with pytest.raises(CodecError) as g:
            codec.scan_index(*args)
        assert word in str(g.value), str(g.value)
    # each null argument alone, with a live ctx
    ptrs = dict(dbuf=dbuf.data_ptr(), keep=keep.data_ptr())
    kw = dict(n_ids=keep.numel(), buf_len=n, off=offs, end=ends)
    for null in ac.SCAN_NULLS:
        ok, msg, out = ac.raw_scan_index(codec.ctx, ptrs, null, **kw)
        assert not ok and msg == f"null argument ({null})" and (out == 0xEE).all(), msg
    ok, msg, out = ac.raw_scan_index(codec.ctx, ptrs, **kw)
    assert ok and out.tolist() == [am.NONE], msg
    # async work pending on the ctx
    from netidx_amd import synth
    from netidx_amd.codec import Columns, LAYOUT_F64
    import netidx_amd
    ids, vals = synth.f64_columns(100)
    wire = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    cols = Columns(100, 0, 0, LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), cols)
    with pytest.raises(CodecError) as g:
        codec.scan_index(dbuf, offs, ends, keep)
    assert "pending" in str(g.value), str(g.value)
    codec.sync()
    verdict, n_match = codec.scan_index(dbuf, [], [], keep)  # n == 0 launches nothing
    assert len(verdict) == 0 and n_match == 0
    verdict, _ = codec.scan_index(dbuf, [n], [n], keep)  # an empty record at the buffer's end
    assert verdict.tolist() == [am.ERR_SHORT]
    verdict, _ = codec.scan_index(dbuf, offs, ends, keep)
    assert verdict.tolist() == [am.NONE]
