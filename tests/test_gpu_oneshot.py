"""GPU tests of nxg_oneshot_pack_pathmap, nxg_oneshot_pack_deltas and nxg_oneshot_assemble_shard
against tests/oneshot_model.py, byte for byte, over the cases of tests/oneshot_cases.py. Every
output lies between guard bands (tests/guards.py). A refused call names what the model names and
leaves every byte of `out` as it was, and the ctx works afterwards.

The smallest shapes that reach each branch, from oneshot_cases.constants(): one row / Id, a wave
+- 1, a block +- 1, a tile +- 1, the top scan's width in blocks +- 1 block (2.6e5 rows of F64, the
largest case), and for the pathmap 2^21 + 300 Ids of which 6 have a path (the Id varint's fourth
byte). An Id varint of 5 bytes would need a path index of 2^28 Ids and is not run for the pathmap;
the deltas reach it with 60 rows over a 256 MiB `sel`."""
import json
import os
import types

import numpy as np
import pytest

import archive_index_model as am
import archive_window_model as awm
import guards
import oneshot_cases as oc
import oneshot_model as om
import record_model as rm
from guards import SENTINEL
from value_table_model import Source

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPARE = 512
K = oc.constants()
PATHMAPS = oc.pathmap_cases(K)
DELTAS = oc.deltas_cases(K)
REFUSALS = oc.deltas_refusal_cases(K)
_want = {}


def want_pm(name):
    if ("pm", name) not in _want:
        _want["pm", name] = om.pathmap_numpy(PATHMAPS[name][0])
    return _want["pm", name]


def want_dl(name):
    if ("dl", name) not in _want:
        _want["dl", name] = om.expected_deltas(DELTAS[name][0])
    return _want["dl", name]


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


def guarded(n, elem=8):
    """n elements of `elem` bytes between SPARE sentinel elements: (whole tensor, the middle)."""
    import torch
    raw = torch.full(((2 * SPARE + n) * elem,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mid = raw[SPARE * elem:(SPARE + n) * elem]
    return raw, mid.view(torch.int64) if elem == 8 else mid


def guards_ok(raw, n, name, elem=8):
    b = raw.cpu().numpy()
    assert (b[:SPARE * elem] == SENTINEL).all(), f"{name}: written in front of the array"
    assert (b[(SPARE + n) * elem:] == SENTINEL).all(), f"{name}: written behind its {n} elements"


class PmCall:
    """One pathmap case on the device, uploaded once."""

    def __init__(self, paths, path_off=None):
        self.n = paths.n_ids
        self.off = dev(paths.path_off() if path_off is None else path_off, np.int64)
        blob = paths.path_bytes()
        self.blob = dev(np.concatenate([np.zeros(10, np.uint8), blob]) if path_off is not None
                        else blob)
        self.keep = dev(paths.keep)

    def run(self, codec, cap=None, phase=0, size_only=False):
        """(n_bytes, sel, n_sel, out bytes | None); guards checked in every outcome."""
        import torch
        from netidx_amd import CodecError
        raw_sel, sel = guarded(self.n, 1)
        buf = None if size_only else guards.guarded_buffer(cap, phase)
        ptr = None if size_only else guards.out_ptr(buf, phase)
        try:
            r = codec.oneshot_pack_pathmap_into(self.off, self.blob, self.keep, ptr,
                                                0 if size_only else cap, sel if self.n else None)
            failed = None
        except CodecError as e:
            r, failed = None, e
        torch.cuda.synchronize()
        guards_ok(raw_sel, self.n, "sel", 1)
        if buf is not None:
            guards.assert_outside_untouched(buf, phase, cap)
        if failed is not None:
            if buf is not None:
                assert (guards.written(buf, phase, cap) == SENTINEL).all(), \
                    "a refused call wrote to out"
            failed.sel_host = sel.cpu().numpy()
            raise failed
        n, s, n_sel = r
        got = None if size_only else guards.written(buf, phase, cap)[:n].tobytes()
        return n, s.cpu().numpy()[:self.n], n_sel, got


def check_pm(res, want):
    blob, sel, n_sel = want
    n, gsel, gn, got = res
    assert n == len(blob) and gn == n_sel
    assert np.array_equal(gsel, sel)
    if got is not None:
        assert got == blob


class DlCall:
    """One deltas case on the device, uploaded once."""

    def __init__(self, win):
        import netidx_amd
        import torch
        S = win.src
        kids = (S.ctag, S.cfixed, S.caux) if S.ctag is not None else (None, None, None)
        self.cols = netidx_amd.columns_from_arrays(win.ids, S.fixed, S.tag, S.aux, *kids)
        self.cols.s.n_rows, self.cols.s.n_children = S.n_rows, S.n_children
        self.heap = dev(np.frombuffer(S.heap, np.uint8)) if len(S.heap) else None
        self.sel = torch.zeros(max(win.n_ids, 1), dtype=torch.uint8, device="cuda")[:win.n_ids]
        if win.selected:
            self.sel[torch.tensor(sorted(win.selected), device="cuda")] = 1
        torch.cuda.synchronize()
        self.win, self.infos = win, win.recs
        self.secs, self.nanos = win.secs, win.nanos

    def run(self, codec, cap=None, phase=0, size_only=False):
        """(n_bytes, rec_off, rec_items, n_items, n_dropped, n_kept_recs, out bytes | None)."""
        import torch
        from netidx_amd import CodecError
        nr = len(self.infos)
        raw_off, rec_off = guarded(nr + 1)
        raw_items, rec_items = guarded(nr)
        buf = None if size_only else guards.guarded_buffer(cap, phase)
        ptr = None if size_only else guards.out_ptr(buf, phase)
        try:
            r = codec.oneshot_pack_deltas_into(self.cols, self.infos, self.secs, self.nanos,
                                               self.sel if self.sel.numel() else None, self.heap,
                                               ptr, 0 if size_only else cap, rec_off,
                                               rec_items if nr else None)
            failed = None
        except CodecError as e:
            r, failed = None, e
        torch.cuda.synchronize()
        guards_ok(raw_off, nr + 1, "rec_off")
        guards_ok(raw_items, nr, "rec_items")
        if buf is not None:
            guards.assert_outside_untouched(buf, phase, cap)
        if failed is not None:
            if buf is not None:
                assert (guards.written(buf, phase, cap) == SENTINEL).all(), \
                    "a refused call wrote to out"
            failed.rec_off_host = rec_off.cpu().numpy().view(np.uint64)
            failed.rec_items_host = rec_items.cpu().numpy().view(np.uint64)
            raise failed
        n, off, items, n_items, dropped, kept = r
        got = None if size_only else guards.written(buf, phase, cap)[:n].tobytes()
        return (n, off.cpu().numpy().view(np.uint64), items.cpu().numpy().view(np.uint64)[:nr],
                n_items, dropped, kept, got)


def check_dl(res, want):
    blob, rec_off, rec_items, n_items, n_dropped, n_kept = want
    n, off, items, gi, gd, gk, got = res
    assert n == len(blob)
    assert np.array_equal(off, rec_off)
    assert np.array_equal(items, rec_items)
    assert (gi, gd, gk) == (n_items, n_dropped, n_kept)
    if got is not None:
        assert got == blob


# ---- the pathmap -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATHMAPS))
def test_pathmap_case_matches_model(codec, name):
    want = want_pm(name)
    call = PmCall(PATHMAPS[name][0])
    phase = sum(name.encode()) % 16
    sized = call.run(codec, size_only=True)
    check_pm(sized, want)
    first = call.run(codec, cap=len(want[0]), phase=phase)  # the capacity exact
    check_pm(first, want)
    again = call.run(codec, cap=len(want[0]) + 7, phase=phase)
    check_pm(again, want)


@pytest.mark.parametrize("name", ["tile+1", "long_two", "len128", "paths200_over_staging", "n1"])
def test_pathmap_out_at_each_16_byte_phase(codec, name):
    want = want_pm(name)
    call = PmCall(PATHMAPS[name][0])
    for phase in range(16):
        check_pm(call.run(codec, cap=len(want[0]) + phase % 3, phase=phase), want)


@pytest.mark.parametrize("name", ["n0", "keep_alternate", "long_mid", "paths200_over_staging"])
def test_pathmap_capacity_one_short(codec, name):
    from netidx_amd import CodecError
    want = want_pm(name)
    call = PmCall(PATHMAPS[name][0])
    with pytest.raises(CodecError) as g:  # (run() checks that out is all sentinel)
        call.run(codec, cap=len(want[0]) - 1, phase=5)
    assert "output buffer too small" in str(g.value) and str(len(want[0])) in str(g.value)
    assert g.value.n_bytes == len(want[0]) and g.value.n_sel == want[2]
    assert np.array_equal(g.value.sel_host, want[1])
    check_pm(call.run(codec, cap=len(want[0]), phase=5), want)


def test_pathmap_decreasing_path_off_names_the_lowest(codec):
    from netidx_amd import CodecError
    for name, (paths, off, lowest) in oc.pathmap_refusal_cases().items():
        call = PmCall(paths, off)
        for size_only in (True, False):
            with pytest.raises(CodecError) as g:
                call.run(codec, cap=1 << 16, phase=3, size_only=size_only)
            assert f"decreases at Id {lowest}:" in str(g.value), (name, str(g.value))
    check_pm(PmCall(PATHMAPS["block+1"][0]).run(codec, cap=len(want_pm("block+1")[0])),
             want_pm("block+1"))


def test_pathmap_misuse(codec):
    from netidx_amd import CodecError
    paths = PATHMAPS["block+1"][0]
    want = want_pm("block+1")
    call = PmCall(paths)

    def refused(word, **kw):
        c = types.SimpleNamespace(**{**call.__dict__, **kw})
        with pytest.raises(CodecError) as g:
            PmCall.run(c, codec, cap=len(want[0]))
        assert word in str(g.value), str(g.value)

    refused("device memory", off=call.off.cpu())
    refused("device memory", blob=call.blob.cpu())
    refused("device memory", keep=call.keep.cpu())
    pending(codec, lambda: refused("pending"))
    check_pm(call.run(codec, cap=len(want[0])), want)


def test_pathmap_max_vec_too_big(codec):
    """kMaxVecBytes / 12 + 1 Ids with a one-byte path each, all kept, size only: TooBig with the
    true n_sel; one Id fewer succeeds with the closed-form length."""
    import torch
    from netidx_amd import CodecError
    n = om.MAX_VEC // om.PATHMAP_ENTRY + 1
    assert n == 178_956_971
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    blob = torch.full((n,), 0x2F, dtype=torch.uint8, device="cuda")
    keep = torch.ones(n, dtype=torch.uint8, device="cuda")
    sel = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(CodecError) as g:
        codec.oneshot_pack_pathmap_into(off, blob, keep, None, 0, sel)
    assert "TooBig" in str(g.value) and str(n) in str(g.value), str(g.value)
    assert g.value.n_sel == n

    def closed(m):  # varint(m), then per Id varint(a) 01 2f
        return om.varint_len(m) + 2 * m + sum(
            (min(m, 1 << (7 * w)) - (1 << (7 * (w - 1)) if w > 1 else 0)) * w
            for w in range(1, 6) if m > (1 << (7 * (w - 1)) if w > 1 else 0))

    assert closed(129) == 2 + 2 * 129 + 128 + 2
    nb, s, n_sel = codec.oneshot_pack_pathmap_into(off[:n], blob, keep[:n - 1], None, 0, sel)
    assert n_sel == n - 1 and nb == closed(n - 1)
    assert bool(s.all())
    del off, blob, keep, sel


def test_assemble_shard_misuse_and_bounds(codec):
    """Host memory and pending async work are refused with nothing written; a good call writes
    exactly [out, out + shard_len) at an odd address."""
    import torch
    from netidx_amd import CodecError
    from netidx_amd.codec import Codec
    pm, im = dev(np.arange(1, 8, dtype=np.uint8)), dev(np.arange(20, 25, dtype=np.uint8))
    frags = [dev(np.arange(40, 70, dtype=np.uint8)), dev(np.zeros(0, np.uint8)),
             dev(np.arange(90, 99, dtype=np.uint8))]
    lay = Codec.oneshot_shard_layout(7, 5, 39, 2)
    raw = guards.guarded_buffer(int(lay.shard_len), 5)
    out = raw[raw.guard_margin + 5:raw.guard_margin + 5 + int(lay.shard_len)]

    def refused(word, **kw):
        a = dict(layout=lay, pathmap=pm, image=im, frags=frags, out=out)
        a.update(kw)
        with pytest.raises(CodecError) as g:
            codec.oneshot_assemble_shard(a["layout"], a["pathmap"], a["image"], a["frags"],
                                         a["out"])
        assert word in str(g.value), str(g.value)
        torch.cuda.synchronize()
        assert (raw.cpu().numpy() == SENTINEL).all(), "a refused call wrote"

    refused("device memory", pathmap=pm.cpu())
    refused("device memory", image=im.cpu())
    refused("device memory", frags=[frags[0], frags[1], frags[2].cpu()])
    refused("device memory", out=torch.full((int(lay.shard_len),), SENTINEL, dtype=torch.uint8))
    refused("do not sum", frags=frags[:2])
    refused("too small", out=out[:-1])
    pending(codec, lambda: refused("pending"))
    got = codec.oneshot_assemble_shard(lay, pm, im, frags, out)
    torch.cuda.synchronize()
    guards.assert_outside_untouched(raw, 5, int(lay.shard_len))
    m = om.shard_layout(7, 5, 39, 2)
    want = (m["len_head"] + bytes(range(1, 8)) + bytes(range(20, 25)) + m["count_head"] +
            bytes(range(40, 70)) + bytes(range(90, 99)))
    assert got.cpu().numpy().tobytes() == want and len(want) == lay.shard_len


def pending(codec, f):
    """f() with async work pending on the ctx."""
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import Columns, LAYOUT_F64
    ids, vals = synth.f64_columns(100)
    wire = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    cols = Columns(100, 0, 0, LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), cols)
    try:
        f()
    finally:
        codec.sync()


# ---- the deltas --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DELTAS))
def test_deltas_case_matches_model(codec, name):
    want = want_dl(name)
    call = DlCall(DELTAS[name][0])
    phase = sum(name.encode()) % 16
    sized = call.run(codec, size_only=True)
    check_dl(sized, want)
    first = call.run(codec, cap=len(want[0]), phase=phase)  # the capacity exact
    check_dl(first, want)
    again = call.run(codec, cap=len(want[0]) + 5, phase=phase)
    check_dl(again, want)
    assert again[6] == first[6], "a rerun differs"


@pytest.mark.parametrize("name", ["values_all", "tile+1", "recs1000x3", "n1"])
def test_deltas_out_at_each_16_byte_phase(codec, name):
    want = want_dl(name)
    call = DlCall(DELTAS[name][0])
    for phase in range(16):
        check_dl(call.run(codec, cap=len(want[0]) + phase % 3, phase=phase), want)


@pytest.mark.parametrize("name", ["values_all", "count_127_128", "big_text_mid_tile"])
def test_deltas_capacity_one_short(codec, name):
    from netidx_amd import CodecError
    want = want_dl(name)
    call = DlCall(DELTAS[name][0])
    with pytest.raises(CodecError) as g:  # (run() checks that out is all sentinel)
        call.run(codec, cap=len(want[0]) - 1, phase=5)
    assert "output buffer too small" in str(g.value) and str(len(want[0])) in str(g.value)
    assert g.value.n_bytes == len(want[0])
    assert np.array_equal(g.value.rec_off_host, want[1])
    assert np.array_equal(g.value.rec_items_host[:len(want[2])], want[2])
    check_dl(call.run(codec, cap=len(want[0]), phase=5), want)


def test_deltas_timestamps_are_written_verbatim(codec):
    """Negative seconds, nanos >= 10^9 (a leap second's 1 999 999 999) and 2^32 - 1, read back
    from the call's own bytes at the offsets the call reports."""
    win = DELTAS["recs1000x3"][0]
    assert min(win.secs) < 0 and max(win.nanos) == 0xFFFFFFFF and 1_999_999_999 in win.nanos
    assert 1_000_000_000 in win.nanos and min(win.secs) < -(1 << 62)
    n, off, items, _, _, kept, blob = DlCall(win).run(codec, cap=len(want_dl("recs1000x3")[0]),
                                                      phase=9)
    assert kept == 1000 and len(blob) == n
    for i in range(1000):
        o = int(off[i])
        assert int.from_bytes(blob[o:o + 8], "big", signed=True) == win.secs[i], i
        assert int.from_bytes(blob[o + 8:o + 12], "big") == win.nanos[i], i
        assert blob[o + 12] == int(items[i]) == 3


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_deltas_refusal_names_the_lowest_and_writes_nothing(codec, name):
    from netidx_amd import CodecError
    win, what = REFUSALS[name]
    assert om.deltas_refusal(win) == what
    call = DlCall(win)
    for size_only in (True, False):
        with pytest.raises(CodecError) as g:
            call.run(codec, cap=1 << 16, phase=3, size_only=size_only)
        msg = str(g.value)
        assert msg.startswith(f"window row {what[1]}: ") and rm.CAUSE_TEXT[what[2]] in msg, msg
    check_dl(DlCall(DELTAS["block+1"][0]).run(codec, cap=len(want_dl("block+1")[0])),
             want_dl("block+1"))


def test_deltas_max_vec_too_big(codec):
    """kMaxVecBytes / 24 + 1 rows of one record that all keep one Id, size only: TooBig, naming
    record 1; one row fewer succeeds with the closed-form length."""
    import torch
    from netidx_amd import CodecError
    from netidx_amd.codec import Columns, LAYOUT_MIXED
    n = rm.MAX_ITEMS + 1
    cols = Columns(n + 3, 0, 0, LAYOUT_MIXED, "cuda")
    for t in ("id", "fixed", "aux"):
        cols.t[t].zero_()
    cols.t["tag"].fill_(16)      # Null: one byte
    cols.s.n_rows = n + 3
    sel = torch.ones(1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(CodecError) as g:
        codec.oneshot_pack_deltas_into(cols, [(0, 3), (3, n)], [0, 0], [0, 0], sel, None, None, 0)
    assert "record 1's items" in str(g.value) and "TooBig" in str(g.value), str(g.value)
    r = codec.oneshot_pack_deltas_into(cols, [(0, 3), (3, n - 1)], [0, 0], [0, 0], sel, None, None, 0)
    assert r[0] == (12 + 1 + 3 * 2) + (12 + om.varint_len(n - 1) + 2 * (n - 1))
    assert r[3:] == (n + 2, 0, 2)
    del cols


def test_deltas_misuse(codec):
    import test_oneshot_cpu as cpu
    from netidx_amd import CodecError
    from netidx_amd.codec import Columns, LAYOUT_F64
    win = DELTAS["block+1"][0]
    want = want_dl("block+1")
    call = DlCall(win)

    def refused(word, **kw):
        c = types.SimpleNamespace(**{**call.__dict__, **kw})
        with pytest.raises(CodecError) as g:
            DlCall.run(c, codec, cap=len(want[0]))
        assert word in str(g.value), str(g.value)

    refused("device memory", sel=call.sel.cpu())
    refused("device memory", heap=np.zeros(16, np.uint8))
    refused("device MIXED-layout columns", cols=Columns(300, 0, 0, LAYOUT_F64, "cuda"))
    n = win.src.n_rows
    refused("leave the window's", infos=[(0, 10), (10, n)])
    refused("row_off must not decrease", infos=[(0, 10), (5, 10)])
    refused("row_off must not decrease", infos=[(20, 10), (0, 10)])
    pending(codec, lambda: refused("pending"))
    # each null argument alone, with a live ctx
    ptrs = dict(sel=call.sel.data_ptr(), rec_off=call.sel.data_ptr(), rec_items=call.sel.data_ptr(),
                out=0)
    for null in cpu.DELTA_NULLS[:-1]:
        ok, msg = cpu.raw_pack_deltas(codec.ctx, null, call.cols.s, ptrs)
        assert not ok and msg == f"null argument ({null})", msg
    check_dl(call.run(codec, cap=len(want[0])), want)


# ---- the chains ------------------------------------------------------------------------------------------
def answer(codec, ibuf, index_spans, dbuf, batch_spans, stamps, paths, n_ids, split_at):
    """do_oneshot over the device calls: the reply's bytes for one shard (index_spans: (off, end)
    in ibuf of each record from its RecordIndex; batch_spans: (off, len) in dbuf of its batch), and
    the records the index scan selected."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns, Codec
    pm, sel, n_sel = codec.oneshot_pack_pathmap(dev(paths.path_off(), np.int64),
                                                dev(paths.path_bytes()), dev(paths.keep))
    verdict, _ = codec.scan_index(ibuf, [o for o, _ in index_spans], [e for _, e in index_spans],
                                  sel)
    picked = [i for i, v in enumerate(verdict.tolist()) if v == am.MATCH]
    recs = [batch_spans[i] for i in picked]
    total = sum(n for _, n in recs)
    cols = Columns(total // 2 + 1, total + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    infos = codec.archive_decode_window(dbuf, recs, cols)
    img = codec.archive_build_image(cols, n_ids, sel)
    image = codec.encode_archive(img.columns(cols), dbuf)
    secs = [stamps[i][0] for i in picked]
    nanos = [stamps[i][1] for i in picked]
    k = min(split_at, len(picked))
    frags, n_deltas = [], 0
    for lo, hi in ((0, k), (k, len(picked))):  # two windows of read_deltas
        b, _, _, _, kept = codec.oneshot_pack_deltas(cols, infos[lo:hi], secs[lo:hi],
                                                     nanos[lo:hi], sel, dbuf)
        frags.append(b)
        n_deltas += kept
    lay = Codec.oneshot_shard_layout(pm.numel(), image.numel(), sum(f.numel() for f in frags),
                                     n_deltas)
    raw = guards.guarded_buffer(int(lay.shard_len), 3)
    out = raw[raw.guard_margin + 3:raw.guard_margin + 3 + int(lay.shard_len)]
    shard = codec.oneshot_assemble_shard(lay, pm, image, frags, out)
    torch.cuda.synchronize()
    guards.assert_outside_untouched(raw, 3, int(lay.shard_len))
    head, reply_len = Codec.oneshot_reply_head([shard.numel()])
    reply = head + shard.cpu().numpy().tobytes()
    assert len(reply) == reply_len
    return reply, picked


def model_answer(paths, win):
    """The do_oneshot port over the same archive: (reply bytes, (pathmap, image, deltas))."""
    import test_oneshot_cpu as cpu
    return cpu.reply_of(paths, win, [win])


def test_chain_recorded_archive_to_reply(codec):
    """record_entries + index_records write an indexed archive's records; pathmap -> sel -> index
    scan -> window -> image -> deltas (two windows) -> shard -> reply equals the model's reply, and
    decodes to what the do_oneshot port computes."""
    from netidx_amd.codec import Dispatch
    n_ids, n_recs = 300, 40
    P = oc.rc.pool_source()
    n = 1200
    src = oc._repeat(P, n)
    rng = np.random.default_rng(0x0e5)
    ids = rng.integers(0, n_ids, n).astype(np.uint64)
    ids[400:700] = rng.integers(200, 230, 300)        # records that hold unselected Ids only
    edges = np.sort(rng.choice(np.arange(1, n), n_recs - 1, replace=False))
    recs = oc.split(n, [int(e) for e in edges])
    stamps = [(1_700_000_000 + 3 * i - 20, (i * 250_000_001) % 2_000_000_000) for i in range(n_recs)]
    keep = ((np.arange(n_ids) % 3 != 1) & ~((np.arange(n_ids) >= 200) & (np.arange(n_ids) < 230)))
    paths = om.Paths([oc.path(4 + a % 50, a) if a % 11 else b"" for a in range(n_ids)],
                     keep.astype(np.uint8))
    # 1. the recorder: every row an entry, the table the identity
    import netidx_amd
    kids = (src.ctag, src.cfixed, src.caux)
    cols = netidx_amd.columns_from_arrays(ids, src.fixed, src.tag, src.aux, *kids)
    cols.s.n_rows, cols.s.n_children = src.n_rows, src.n_children
    heap = dev(np.frombuffer(src.heap, np.uint8))
    chan_off = dev(np.array([a for a, _ in recs] + [n], np.uint64), np.int64)
    disp = Dispatch(chan_off, dev(ids, np.int64), dev(np.arange(n, dtype=np.uint64), np.int64),
                    None, n, 0)
    table = dev(np.arange(n_ids, dtype=np.uint32), np.int32)
    batches, boff, _, _ = codec.record_entries(cols, disp, table, heap)
    idx, ioff, _ = codec.index_records(disp.ent_sub, chan_off)
    batches, idx = batches.cpu().numpy(), idx.cpu().numpy()
    boff, ioff = boff.cpu().tolist(), ioff.cpu().tolist()
    file, ispans, bspans = bytearray(b"\xee" * 19), [], []
    for i in range(n_recs):
        o = len(file)
        file += idx[ioff[i]:ioff[i + 1]].tobytes()
        bspans.append((len(file), boff[i + 1] - boff[i]))
        file += batches[boff[i]:boff[i + 1]].tobytes()
        ispans.append((o, len(file)))
        file += b"\xee" * (i % 5)
    dbuf = dev(np.frombuffer(bytes(file), np.uint8))
    # 2.-7.
    reply, picked = answer(codec, dbuf, ispans, dbuf, bspans, stamps, paths, n_ids, split_at=13)
    win = om.Window(src, ids, recs, [s for s, _ in stamps], [x for _, x in stamps], n_ids,
                    set(np.flatnonzero(om.pathmap_numpy(paths)[1]).tolist()))
    want, objs = model_answer(paths, win)
    assert 0 < len(picked) < n_recs
    assert reply == want
    (pm, im, dl), = om.decode_reply(reply)
    assert (pm, im, dl) == objs and len(dl) > 5 and len(im) > 50


def test_chain_compressed_golden_records(codec):
    """The indexed, compressed golden records: scanned where they lie, decompressed, decoded as a
    window, answered; the model reads the same batches through the host window model."""
    ents = json.load(open(os.path.join(GOLD, "zstd_manifest.json")))["records"]
    rec = np.frombuffer(open(os.path.join(GOLD, "zstd_records.bin"), "rb").read(), np.uint8)
    zd = codec.zstd_dict(open(os.path.join(GOLD, "zstd_dict.bin"), "rb").read())
    es = [e for e in ents if e["batch"] and e["dict"] and e["indexed"]]
    assert len(es) >= 3
    out, res = codec.archive_decompress(rec, [(e["rec_off"], e["rec_len"]) for e in es], True, zd)
    assert all(r[2] == 0 for r in res)
    host = out.cpu().numpy()
    m, minfos = awm.window(host, res)
    n_ids = int(m["id"].max()) + 2
    keep = (np.arange(n_ids) % 2 == 0).astype(np.uint8)
    paths = om.Paths([oc.path(3 + a % 40, a) if a % 7 else b"" for a in range(n_ids)], keep)
    stamps = [(-5 + i, 999_999_999 + i) for i in range(len(es))]
    # the index is scanned in the compressed records; the batches are the decompressed ones
    ispans = [(e["rec_off"] + 4, e["rec_off"] + e["rec_len"]) for e in es]
    bspans = [(r[0], r[1]) for r in res]
    reply, picked = answer(codec, dev(rec), ispans, out, bspans, stamps, paths, n_ids, split_at=1)
    assert 0 < len(picked) <= len(es)  # (a record without a selected Id keeps nothing in the model)
    nr = int(sum(f["n_rows"] for f in minfos))
    src = Source(m["tag"][:nr], m["fixed"][:nr], m["aux"][:nr], m["ctag"], m["cfixed"], m["caux"],
                 host.tobytes())
    win = om.Window(src, m["id"][:nr], [(f["row_off"], f["n_rows"]) for f in minfos],
                    [s for s, _ in stamps], [x for _, x in stamps], n_ids,
                    set(np.flatnonzero(om.pathmap_numpy(paths)[1]).tolist()))
    want, objs = model_answer(paths, win)
    assert reply == want
    assert om.decode_reply(reply) == [objs] and len(objs[2]) >= 1
