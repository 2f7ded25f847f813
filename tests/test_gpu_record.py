"""GPU tests of nxg_record_entries against tests/record_model.py, byte for byte, over the cases of
tests/record_cases.py. `out`, `rec_off` and `rec_items` lie between guard bands; every case runs in
MIXED layout and, where every value is an F64, in F64 layout. A refused call names what the model
names and leaves every byte of `out` as it was, and the ctx works afterwards."""
import types

import numpy as np
import pytest

import guards
import record_cases as rc
import record_model as rm
import reply_route_cases as rrc
import reply_route_model as rrm
from guards import SENTINEL
from value_table_model import Source

pytestmark = pytest.mark.gpu
SPARE = 512
K = rc.constants()
CASES = rc.cases(K)
REFUSALS = rc.refusal_cases(K)
LAYOUTS = [(n, "mixed") for n in sorted(CASES)] + [(n, "f64") for n in sorted(CASES)
                                                   if CASES[n][2]]
_want = {}


def want_of(name):
    """(blob, rec_off, rec_items, n_dropped) of a case, computed once."""
    if name not in _want:
        _want[name] = rm.expected(CASES[name][0])
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


def batch_of(S):
    """(device Columns, device heap | None) of a Source (tag None: F64 layout)."""
    import netidx_amd
    ids = np.zeros(len(S.fixed), np.uint64)
    kids = (S.ctag, S.cfixed, S.caux) if S.ctag is not None else (None, None, None)
    cols = netidx_amd.columns_from_arrays(ids, S.fixed, S.tag, S.aux, *kids)
    cols.s.n_rows, cols.s.n_children = S.n_rows, S.n_children
    heap = dev(np.frombuffer(S.heap, np.uint8)) if len(S.heap) else None
    return cols, heap


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
    """One case on the device: its batch, entry list and table, uploaded once."""

    def __init__(self, case, n_entries=None):
        from netidx_amd.codec import Dispatch
        self.case = case
        self.cols, self.heap = batch_of(case.src)
        self.disp = Dispatch(dev(case.chan_off, np.int64), dev(case.ent_sub, np.int64),
                             dev(case.ent_row, np.int64), None,
                             case.n_entries if n_entries is None else n_entries, 0)
        self.table = dev(case.arch, np.int32)
        self.n_chans = case.n_chans

    def run(self, codec, cap=None, phase=0, size_only=False):
        """(n_bytes, rec_off, rec_items, n_items, n_dropped, out bytes | None). `cap`: the
        capacity stated (default: exactly what the model needs). Guards checked in every outcome."""
        from netidx_amd import CodecError
        nc = self.n_chans
        raw_off, rec_off = guarded_words(nc + 1)
        raw_items, rec_items = guarded_words(nc)
        buf = None
        if not size_only:
            buf = guards.guarded_buffer(cap, phase)
        ptr = None if size_only else guards.out_ptr(buf, phase)
        try:
            r = codec.record_entries_into(self.cols, self.disp, self.table, self.heap, ptr,
                                          0 if size_only else cap, rec_off, rec_items)
            failed = None
        except CodecError as e:
            r, failed = None, e
        import torch
        torch.cuda.synchronize()
        words_guards_ok(raw_off, nc + 1, "rec_off")
        words_guards_ok(raw_items, nc, "rec_items")
        if buf is not None:
            guards.assert_outside_untouched(buf, phase, cap)
        if failed is not None:
            if buf is not None:
                assert (guards.written(buf, phase, cap) == SENTINEL).all(), \
                    "a refused call wrote to out"
            failed.rec_off_host = rec_off.cpu().numpy().view(np.uint64)
            failed.rec_items_host = rec_items.cpu().numpy().view(np.uint64)
            raise failed
        n, off, items, n_items, n_dropped = r
        got = None if size_only else guards.written(buf, phase, cap)[:n].tobytes()
        return (n, off.cpu().numpy().view(np.uint64), items.cpu().numpy().view(np.uint64),
                n_items, n_dropped, got)


def check_equal(res, want):
    blob, rec_off, rec_items, n_dropped = want
    n, off, items, n_items, dropped, got = res
    assert n == len(blob)
    assert np.array_equal(off, rec_off)
    assert np.array_equal(items, rec_items)
    assert n_items == int(rec_items.sum()) and dropped == n_dropped
    if got is not None:
        assert got == blob


# ---- every case, both layouts ------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", LAYOUTS)
def test_case_matches_model(codec, name, layout):
    case = CASES[name][0]
    want = want_of(name)
    call = Call(case if layout == "mixed" else case.f64_layout())
    phase = sum(name.encode()) % 16
    sized = call.run(codec, size_only=True)
    check_equal(sized, want)
    first = call.run(codec, cap=len(want[0]), phase=phase)  # the capacity exact
    check_equal(first, want)
    again = call.run(codec, cap=len(want[0]), phase=phase)
    check_equal(again, want)
    assert again[5] == first[5], "a rerun differs"
    assert np.array_equal(sized[1], first[1]) and np.array_equal(sized[2], first[2])


@pytest.mark.parametrize("name", ["values_all", "tile+1", "chan1000"])
def test_out_at_each_16_byte_phase(codec, name):
    want = want_of(name)
    call = Call(CASES[name][0])
    for phase in range(16):
        check_equal(call.run(codec, cap=len(want[0]) + phase % 3, phase=phase), want)


@pytest.mark.parametrize("name", ["values_all", "count_varint", "big_text_mid_tile"])
def test_capacity_one_short(codec, name):
    from netidx_amd import CodecError
    want = want_of(name)
    call = Call(CASES[name][0])
    with pytest.raises(CodecError) as g:  # (run() checks that out is all sentinel)
        call.run(codec, cap=len(want[0]) - 1, phase=5)
    assert "output buffer too small" in str(g.value) and str(len(want[0])) in str(g.value)
    assert g.value.n_bytes == len(want[0])
    assert np.array_equal(g.value.rec_off_host, want[1])
    assert np.array_equal(g.value.rec_items_host, want[2])
    check_equal(call.run(codec, cap=len(want[0]), phase=5), want)


# ---- refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_names_the_lowest_and_writes_nothing(codec, name):
    from netidx_amd import CodecError
    case, what = REFUSALS[name]
    assert rm.refusal(case) == what
    call = Call(case)
    for size_only in (True, False):
        with pytest.raises(CodecError) as g:
            call.run(codec, cap=1 << 16, phase=3, size_only=size_only)
        msg = str(g.value)
        if what[0] == "entry":
            assert msg.startswith(f"entry {what[1]}: ") and rm.CAUSE_TEXT[what[2]] in msg, msg
        else:
            assert f"at channel {what[1]}:" in msg and "not a dispatch's" in msg, msg
    good = CASES["block+1"][0]
    check_equal(Call(good).run(codec, cap=len(want_of("block+1")[0])), want_of("block+1"))


def test_misuse(codec):
    import torch
    from netidx_amd import CodecError
    from netidx_amd.codec import Columns, Dispatch, LAYOUT_F64
    case = CASES["block+1"][0]
    want = want_of("block+1")
    call = Call(case)

    def refused(word, **kw):
        c = types.SimpleNamespace(**{**call.__dict__, **kw})
        with pytest.raises(CodecError) as g:
            Call.run(c, codec, cap=len(want[0]))
        assert word in str(g.value), str(g.value)

    d = call.disp
    refused("cap_entries", disp=Dispatch(d.chan_off, d.ent_sub, d.ent_row, None,
                                         case.n_entries + 1, 0))
    refused("device memory", heap=np.zeros(16, np.uint8))
    refused("device memory", disp=Dispatch(d.chan_off.cpu(), d.ent_sub, d.ent_row, None,
                                           case.n_entries, 0))
    refused("device memory", table=call.table.cpu())
    # async work pending on the ctx
    fc, _ = batch_of(case.f64_layout().src)
    wire = codec.encode_batch(fc)
    out = Columns(case.src.n_rows, 0, 0, LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), out)
    refused("pending")
    codec.sync()
    check_equal(call.run(codec, cap=len(want[0])), want)


# ---- MAX_VEC -------------------------------------------------------------------------------------
def test_max_vec_too_big(codec):
    """kMaxVecBytes / 24 + 1 entries that all name one F64 row, size only: TooBig, naming channel
    0; one entry fewer succeeds with the closed-form length."""
    import torch
    from netidx_amd import CodecError
    from netidx_amd.codec import Dispatch
    n = rm.MAX_ITEMS + 1
    assert n == 89_478_486
    S = Source(None, np.array([0x4000000000000000], np.uint64), None)
    cols, _ = batch_of(S)
    zeros = torch.zeros(n, dtype=torch.int64, device="cuda")  # ent_sub and ent_row alike
    table = dev(np.array([0], np.uint32), np.int32)
    for ne, ok in ((n, False), (n - 1, True)):
        disp = Dispatch(dev(np.array([0, ne], np.uint64), np.int64), zeros, zeros, None, ne, 0)
        if not ok:
            with pytest.raises(CodecError) as g:
                codec.recorded_len(cols, disp, table)
            assert "channel 0" in str(g.value) and "TooBig" in str(g.value), str(g.value)
            continue
        nb, off, items, dropped = codec.recorded_len(cols, disp, table)
        assert nb == rm.f64_closed_form(ne, 0) and dropped == 0
        assert off.cpu().tolist() == [0, nb] and items.cpu().tolist() == [ne]


# ---- against the library itself ----------------------------------------------------------------------
def library_records(codec, cols, heap, disp, table, n_chans):
    """What the library offered before this call: per channel, torch gathers of the columns by
    ent_row, a translated and masked id column, one nxg_encode_archive_batch."""
    import torch
    from netidx_amd.codec import Columns, LAYOUT_MIXED
    spare = Columns(1, 1, 1, LAYOUT_MIXED, "cuda")  # (the call wants every array of the layout)
    off = disp.chan_off.cpu().tolist()
    tab = table.to(torch.int64) & 0xFFFFFFFF
    f64 = cols.t.get("tag") is None
    out = []
    for c in range(n_chans):
        sub, row = disp.ent_sub[off[c]:off[c + 1]], disp.ent_row[off[c]:off[c + 1]]
        known = (sub >= 0) & (sub < tab.numel())
        aid = torch.where(known, tab[torch.where(known, sub, 0)], 0xFFFFFFFF)
        keep = aid != 0xFFFFFFFF
        aid, row = aid[keep], row[keep]
        if not aid.numel():
            out.append(b"")
            continue
        span = row < 0  # NXG_ENT_SPAN is the sign bit
        r = torch.where(span, 0, row)
        tag = torch.where(span, 0x40, 9 if f64 else cols.tag[r].to(torch.int64)).to(torch.uint8)
        fixed = torch.where(span, 0, cols.fixed[r])
        aux = torch.zeros_like(r, dtype=torch.int32) if f64 else torch.where(span, 0, cols.aux[r])
        s = spare.s
        s.cap_rows = s.n_rows = aid.numel()
        s.cap_children = s.n_children = cols.s.n_children
        s.id, s.tag, s.fixed, s.aux = (aid.data_ptr(), tag.data_ptr(), fixed.data_ptr(),
                                       aux.data_ptr())
        if cols.s.n_children:
            s.ctag, s.cfixed, s.caux = cols.s.ctag, cols.s.cfixed, cols.s.caux
        torch.cuda.synchronize()
        rec = codec.encode_archive(types.SimpleNamespace(s=s, id=aid), heap)
        out.append(rec.cpu().numpy().tobytes())
    return out


@pytest.mark.parametrize("name", ["values_repeat_descending", "chan16_edges", "unsubscribed"])
def test_equals_encode_archive_batch_per_channel(codec, name):
    call = Call(CASES[name][0])
    want = library_records(codec, call.cols, call.heap, call.disp, call.table, call.n_chans)
    got, off, _, _ = codec.record_entries(call.cols, call.disp, call.table, call.heap)
    got, off = got.cpu().numpy().tobytes(), off.cpu().tolist()
    assert [got[off[c]:off[c + 1]] for c in range(call.n_chans)] == want


# ---- end to end ----------------------------------------------------------------------------------------
def host_case(cols, frame_bytes, disp, arch):
    """The model's Case of decoded device columns and a device entry list."""
    h = cols.numpy()
    nk = int(cols.s.n_children)
    S = Source(h["tag"], h["fixed"], h["aux"], h["ctag"][:nk] if nk else None,
               h["cfixed"][:nk] if nk else None, h["caux"][:nk] if nk else None, frame_bytes)
    ne = int(disp.n_entries)
    return rm.Case(S, disp.ent_sub[:ne].cpu().numpy().view(np.uint64),
                   disp.ent_row[:ne].cpu().numpy().view(np.uint64),
                   disp.chan_off.cpu().numpy().view(np.uint64), arch)


def check_records_decode(codec, got, off, case):
    """nxg_decode_archive_batch of each record: the kept entries' (arch_id, tag, fixed-or-text,
    aux) as the model has them."""
    from netidx_amd.codec import Columns, LAYOUT_MIXED
    kept, aid = case.keep()
    span = case.is_span()
    S = case.src
    for c in range(case.n_chans):
        lo, hi = int(case.chan_off[c]), int(case.chan_off[c + 1])
        idx = lo + np.flatnonzero(kept[lo:hi])
        rec = got[off[c]:off[c + 1]]
        assert (rec.numel() == 0) == (len(idx) == 0)
        if not len(idx):
            continue
        out = Columns(len(idx), rec.numel(), 0, LAYOUT_MIXED, "cuda")
        st, used = codec.decode_archive(rec.contiguous(), rec.numel(), out)
        assert used == rec.numel() and st.n_rows == len(idx)
        o = out.numpy()
        rows = np.where(span[idx], 0, case.ent_row[idx]).astype(np.int64)
        tag = np.where(span[idx], rm.TAG_UNSUBSCRIBED, S.tag[rows])
        assert np.array_equal(o["id"], aid[idx].astype(np.uint64))
        assert np.array_equal(o["tag"], tag)
        text = np.isin(tag, (12, 13, 18, 27))
        plain = np.isin(tag, (4, 5, 6, 7, 9, 10, 11))
        assert np.array_equal(o["fixed"][plain], S.fixed[rows][plain])
        keep_aux = tag != rm.TAG_UNSUBSCRIBED
        assert np.array_equal(o["aux"][keep_aux], S.aux[rows][keep_aux])
        rb = rec.cpu().numpy().tobytes()
        for j in np.flatnonzero(text):
            f, a, g = int(o["fixed"][j]), int(o["aux"][j]), int(S.fixed[rows[j]])
            assert rb[f:f + a] == S.heap[g:g + a]


def test_decode_dispatch_record_decode(codec):
    from netidx_amd import synth
    from netidx_amd.codec import Columns, HINT_MIXED, LAYOUT_MIXED, SubTable
    import netidx_amd
    n, n_chans = 5000, 7
    m = synth.mixed_columns(n)
    mc = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
    frame = codec.encode_batch(mc, dev(m.heap))
    cols = Columns.for_frame(frame.numel(), LAYOUT_MIXED, "cuda")
    codec.decode_into(frame, frame.numel(), cols, flags=HINT_MIXED)
    assert cols.s.n_rows == n
    rng = np.random.default_rng(11)
    subs = {int(i): (int(3 * i + 1), [int(x) for x in rng.integers(0, n_chans, rng.integers(0, 4))],
                     True) for i in rng.choice(n, n * 3 // 4, replace=False)}
    disp = codec.dispatch_updates(SubTable.from_subscriptions(subs, n_chans, n), cols.id, n)
    arch = np.where(np.arange(3 * n + 2) % 5 == 0, rm.NO_SLOT, np.arange(3 * n + 2) * 7)
    arch = arch.astype(np.uint32)
    got, off, items, dropped = codec.record_entries(cols, disp, dev(arch, np.int32), frame)
    case = host_case(cols, frame.cpu().numpy().tobytes(), disp, arch)
    want = rm.expected(case)
    assert want[3] > 0 and int(want[2].sum()) > 0
    assert got.cpu().numpy().tobytes() == want[0]
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want[1])
    assert np.array_equal(items.cpu().numpy().view(np.uint64), want[2]) and dropped == want[3]
    check_records_decode(codec, got, off.cpu().tolist(), case)


def test_route_replies_record_unsubscribed(codec):
    import test_gpu_route_replies as T
    _, st, msgs, n_ids, n_chans, quirks = rrc.random_case(300, 200, 5, once=True)
    frame, cols = T.decode(codec, msgs, quirks)
    tab, _, _ = rrm.tables_of(st, n_ids, n_chans)
    t = T.device_table(codec, tab)
    r = codec.route_replies(t, frame, cols)
    arch = np.where(np.arange(2100) % 3 == 0, rm.NO_SLOT, np.arange(2100) + 9).astype(np.uint32)
    disp = types.SimpleNamespace(chan_off=r.chan_off, ent_sub=r.ent_sub, ent_row=r.ent_row,
                                 n_entries=r.n_entries)
    got, off, items, dropped = codec.record_entries(cols, disp, dev(arch, np.int32), frame)
    case = host_case(cols, frame.cpu().numpy().tobytes(), disp, arch)
    kept, _ = case.keep()
    assert (kept & case.is_span()).any(), "the case records no Unsubscribed"
    want = rm.expected(case)
    assert got.cpu().numpy().tobytes() == want[0] == b"".join(rm.records_python(case))
    assert np.array_equal(items.cpu().numpy().view(np.uint64), want[2]) and dropped == want[3]
    check_records_decode(codec, got, off.cpu().tolist(), case)
    t.pending.close()


def test_value_table_image_record(codec):
    """write_image (record.rs:165-179): two applies, then an identity entry list over the table's
    columns (ent_sub = the SubIds that have an image entry, ent_row = their slots)."""
    import torch
    from netidx_amd.codec import Dispatch, ValueTable
    P = rc.pool_source()
    n_slots = 40
    vt = ValueTable(codec, n_slots, 1 << 20, 1 << 12).init()
    cols, heap = batch_of(P)
    rng = np.random.default_rng(3)
    for _ in range(2):
        src = np.where(rng.random(n_slots) < 0.6, 1 + rng.integers(0, P.n_rows, n_slots), 0)
        vt.apply(cols, dev(src.astype(np.uint64), np.int64), heap)
    slots = np.array([s for s in range(n_slots) if s % 4 != 3], np.uint64)
    sub_of = slots * np.uint64(2) + np.uint64(1)
    arch = np.full(2 * n_slots + 2, rm.NO_SLOT, np.uint32)
    arch[sub_of.astype(np.int64)] = 100 + slots.astype(np.uint32) * 300
    disp = Dispatch(dev(np.array([0, len(slots)], np.uint64), np.int64), dev(sub_of, np.int64),
                    dev(slots, np.int64), None, len(slots), 0)
    view = vt.as_columns(torch.zeros(n_slots, dtype=torch.int64, device="cuda"))
    got, off, items, dropped = codec.record_entries(view, disp, dev(arch, np.int32), vt.t["heap"])
    h = vt.numpy()
    S = Source(h["tag"], h["fixed"], h["aux"], h["ctag"], h["cfixed"], h["caux"],
               h["heap"].tobytes())
    case = rm.Case(S, sub_of, slots, [0, len(slots)], arch)
    want = rm.expected(case)
    assert dropped == 0 and items.cpu().tolist() == [len(slots)]
    assert got.cpu().numpy().tobytes() == want[0] == b"".join(rm.records_python(case))
