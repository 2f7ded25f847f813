"""GPU tests of nxg_replay_window / nxg_replay_image against tests/replay_model.py over the cases of
tests/replay_cases.py. Every output array lies between guard bands, on success and on every false
return; a refused call leaves the ctx working. The chains run a decoded window (golden archive
batches plus synthetic records) through replay, commit and the per-client encode, and compare
each client's bytes with the oracle's encode of the model's updates."""
import os

import numpy as np
import pytest

import archive_window_model as awm
import client_frames_model as cfm
import replay_cases as rc
import replay_model as rm
from guards import SENTINEL

pytestmark = pytest.mark.gpu
SPARE = 512
K = rc.constants()
CASES = rc.cases(K)
SHORT = rc.short_cases(K)
IMAGES = rc.image_cases(K)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ISZ = {"uint8": 1, "int32": 4, "int64": 8}
_want = {}


def want_of(case):
    if case.name not in _want or _want[case.name][0] is not case:
        _want[case.name] = (case, case.expected())
    return _want[case.name][1]


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


def window_columns(cols):
    import netidx_amd
    n = len(cols["id"])
    if n == 0:
        return netidx_amd.Columns(1, 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    c = netidx_amd.columns_from_arrays(cols["id"], cols["fixed"], cols["tag"], cols["aux"])
    c.s.n_rows = n
    return c


class Guarded:
    """A ReplayRows whose seven arrays lie between SPARE sentinel elements."""

    def __init__(self, cap_rows, n_recs, cap_miss):
        import torch
        from netidx_amd.codec import ReplayRows
        sizes = {k: (dt, cap_rows) for k, dt in ReplayRows.ROW_ARRAYS}
        sizes["rec_off"] = ("int64", n_recs + 1)
        sizes["miss_row"] = ("int64", cap_miss)
        self.sizes, self.raw, view = sizes, {}, {}
        for k, (dt, n) in sizes.items():
            raw = torch.full(((2 * SPARE + n) * ISZ[dt],), SENTINEL, dtype=torch.uint8, device="cuda")
            self.raw[k] = raw
            view[k] = raw.view(getattr(torch, dt))[SPARE:SPARE + n]
        torch.cuda.synchronize()
        self.rows = ReplayRows(cap_rows, n_recs, cap_miss, "cuda", arrays=view)

    def check_guards(self):
        import torch
        torch.cuda.synchronize()
        for k, (dt, n) in self.sizes.items():
            b = self.raw[k].cpu().numpy()
            lo, hi = SPARE * ISZ[dt], (SPARE + n) * ISZ[dt]
            assert (b[:lo] == SENTINEL).all(), f"{k}: written in front of the array"
            bad = np.flatnonzero(b[hi:] != SENTINEL)
            assert not len(bad), f"{k}[{n + int(bad[0]) // ISZ[dt]}] was written (capacity {n})"

    def untouched(self, k):
        dt, n = self.sizes[k]
        b = self.raw[k].cpu().numpy()
        return (b[SPARE * ISZ[dt]:(SPARE + n) * ISZ[dt]] == SENTINEL).all()


def check_result(g, want, cap_miss, short=False):
    r = g.rows
    assert (r.n_rows, r.n_dropped, r.n_done, r.n_miss) == (want.n_rows, want.n_dropped,
                                                            want.n_done, want.n_miss)
    assert np.array_equal(r.offsets(), want.rec_off)
    listed = min(want.n_miss, cap_miss)
    assert np.array_equal(r.misses(), want.miss[:listed])
    if short:
        for k, _ in r.ROW_ARRAYS:
            assert g.untouched(k), f"a refused call wrote {k}"
    else:
        got = r.numpy()
        for k in rm.ROW_COLS:
            assert np.array_equal(got[k], want.rows[k]), k


def run_window(codec, case, cap_rows=None):
    """The call into guarded arrays; guards checked in every outcome. Returns (Guarded, error)."""
    from netidx_amd import CodecError
    want = want_of(case)
    cap = rc.cap_rows_of(case, want) if cap_rows is None else cap_rows
    g = Guarded(cap, len(case.infos), case.cap_miss)
    err = None
    try:
        codec.replay_window(window_columns(case.cols), case.infos, dev(case.table, np.int64),
                            out=g.rows)
    except CodecError as e:
        err = e
    g.check_guards()
    return g, err


def clean_replay(codec):
    """The ctx still replays after a refusal."""
    case = CASES["empty_records_around"]
    g, err = run_window(codec, case)
    assert err is None
    check_result(g, want_of(case), case.cap_miss)


# ---- the window cases --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_window_case(codec, name):
    case = CASES[name]
    g, err = run_window(codec, case)
    assert err is None, err
    check_result(g, want_of(case), case.cap_miss)


@pytest.mark.parametrize("name", sorted(SHORT))
def test_window_capacity_short(codec, name):
    case = SHORT[name]
    want = want_of(case)
    g, err = run_window(codec, case)
    assert err is not None and "capacity" in str(err)
    assert err.rows is g.rows and g.rows.n_rows == want.n_rows  # the need
    check_result(g, want, case.cap_miss, short=True)
    clean_replay(codec)
    g, err = run_window(codec, case, cap_rows=want.n_rows)  # exactly the need: it fits
    assert err is None
    check_result(g, want, case.cap_miss)


def test_replays_from_record_n_done(codec):
    """The second call of the stop protocol: the infos from n_done on, the table updated."""
    case = CASES["two_records_miss"]
    want = want_of(case)
    table = case.table.copy()
    table[table == np.uint64(rm.MISS)] = 5555  # the host published them
    start, seen = want.n_done, []
    assert 0 < start < len(case.infos)
    w2 = rm.window_loop(case.cols, case.infos[start:], table)
    g = Guarded(len(case.cols["id"]), len(case.infos) - start, 4)
    codec.replay_window(window_columns(case.cols), case.infos[start:], dev(table, np.int64),
                        out=g.rows)
    g.check_guards()
    check_result(g, w2, 4)
    assert w2.n_done == len(case.infos) - start and w2.n_rows


def test_window_misuse_is_refused_on_the_host(codec):
    import torch
    import netidx_amd
    from netidx_amd import CodecError
    case = CASES["empty_records_around"]
    cols, table = window_columns(case.cols), dev(case.table, np.int64)
    n = len(case.cols["id"])

    def refused(match, wcols=cols, infos=case.infos, tab=table, edit=None):
        g = Guarded(n, len(infos), 4)
        if edit:
            edit(g.rows)
        with pytest.raises(CodecError, match=match):
            codec.replay_window(wcols, infos, tab, out=g.rows)
        g.check_guards()
        for k in g.sizes:
            assert g.untouched(k), f"a refused call wrote {k}"
        clean_replay(codec)

    refused("leave the window", infos=[(0, 10), (10, n)])
    refused("leave the window", infos=[(n + 1, 0)])
    refused("must not decrease", infos=[(20, 5), (10, 5)])
    refused("overlap", infos=[(0, 10), (5, 10)])
    f64 = netidx_amd.Columns(n, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
    f64.s.n_rows = n
    refused("MIXED", wcols=f64)
    host = netidx_amd.Columns(n, 1, 1, netidx_amd.LAYOUT_MIXED, "cpu")
    host.s.n_rows = n
    refused("MIXED", wcols=host)
    refused("device memory", tab=torch.zeros(40, dtype=torch.int64).pin_memory())
    refused("null", edit=lambda r: setattr(r.s, "rec_off", None))
    refused("null", edit=lambda r: setattr(r.s, "fixed", None))
    refused("null", edit=lambda r: setattr(r.s, "miss_row", None))
    pinned = torch.zeros(n, dtype=torch.int64).pin_memory()
    refused("device memory", edit=lambda r: setattr(r.s, "src_row", pinned.data_ptr()))
    # an async decode pending on the ctx
    from netidx_amd import synth
    ids, vals = synth.f64_columns(100)
    wire = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    out = netidx_amd.Columns(100, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), out)
    try:
        g = Guarded(n, len(case.infos), 4)
        with pytest.raises(CodecError, match="pending"):
            codec.replay_window(cols, case.infos, table, out=g.rows)
        g.check_guards()
    finally:
        codec.sync()
    clean_replay(codec)


# ---- the image cases ---------------------------------------------------------------------------
def device_image(image):
    from netidx_amd.codec import ArchiveImage
    n = len(image["id"])
    img = ArchiveImage(n, "cuda")
    for k in ("id", "tag", "fixed", "aux"):
        if n:
            getattr(img, k)[:n] = dev(image[k], {"id": np.int64, "fixed": np.int64,
                                                 "aux": np.int32, "tag": None}[k])
    import torch
    torch.cuda.synchronize()
    img.s.n_rows = n
    return img


def run_image(codec, case, cap_rows=None):
    from netidx_amd import CodecError
    want = want_of(case)
    n = len(case.order)
    cap = cap_rows if cap_rows is not None else want.n_rows if case.cap_rows == "exact" else n
    g = Guarded(cap, 1, case.cap_miss)
    err = None
    try:
        codec.replay_image(device_image(case.image), dev(case.order, np.int32),
                           dev(case.table, np.int64), out=g.rows)
    except CodecError as e:
        err = e
    g.check_guards()
    return g, err


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_image_case(codec, name):
    case = IMAGES[name]
    g, err = run_image(codec, case)
    assert err is None, err
    check_result(g, want_of(case), case.cap_miss)


def test_image_capacity_short_and_misuse(codec):
    import torch
    from netidx_amd import CodecError
    case = IMAGES["unsorted_order"]
    want = want_of(case)
    g, err = run_image(codec, case, cap_rows=want.n_rows - 1)
    assert err is not None and g.rows.n_rows == want.n_rows
    check_result(g, want, case.cap_miss, short=True)
    clean_replay(codec)
    g, err = run_image(codec, case, cap_rows=want.n_rows)
    assert err is None
    check_result(g, want, case.cap_miss)
    g = Guarded(len(case.order), 1, 4)
    with pytest.raises(CodecError, match="device memory"):
        codec.replay_image(device_image(case.image),
                           torch.zeros(10, dtype=torch.int32).pin_memory(),
                           dev(case.table, np.int64), out=g.rows)
    g.check_guards()
    clean_replay(codec)


# ---- the chains --------------------------------------------------------------------------------
N_CLIENTS = 3


def chain_window():
    """Golden archive batches and synthetic records with every kind of value. The last two golden
    batches carry Ids far past any table: the window stops in front of them."""
    import test_gpu_archive_window as taw
    gold = [open(os.path.join(GOLD, f"archive_{n}.bin"), "rb").read()
            for n in ("ref_basic", "empty", "long", "trailing", "mixed", "unsub_only")]
    buf1, recs1 = taw.image_window(60, 40, 77, taw.RICH)
    synth = [bytes(buf1[o:o + n]) for o, n in recs1]
    records = gold[:2] + synth[:20] + gold[2:4] + synth[20:] + gold[4:]
    buf, recs = taw.layout(records, gap=3, pad=5)
    return taw, buf, recs, len(records) - 2


def replay_table(n_ids):
    """Archive Id a -> publisher Id 3 a + 1; every seventh Id has no path."""
    return np.array([rm.DROP if a % 7 == 0 else 3 * a + 1 for a in range(n_ids)], np.uint64)


def publisher(table, codec_dev="cuda"):
    """(PubTable, {publisher Id: its clients}): every published Id a slot, clients by slot."""
    from netidx_amd.codec import PubTable
    pubs = [int(p) for p in table.tolist() if p not in (rm.DROP, rm.MISS)]
    soi = np.full(max(pubs) + 1, 0xFFFFFFFF, np.uint32)
    soi[pubs] = np.arange(len(pubs))
    fan = [[c for c in range(N_CLIENTS) if (s + c) % 4 != 0] for s in range(len(pubs))]
    off = np.concatenate([[0], np.cumsum([len(x) for x in fan])])
    pt = PubTable(soi, off, [c for x in fan for c in x], N_CLIENTS, np.full(len(pubs), 16, np.uint8),
                  np.zeros(len(pubs), np.uint64), np.zeros(len(pubs), np.uint32), device=codec_dev)
    return pt, {p: fan[s] for s, p in enumerate(pubs)}, pubs


def check_clients(codec, view, dbuf, pt, clients_of, want_rows, wcols, buf):
    """commit + encode_clients of the view; each client's bytes against the oracle's encode of the
    model's updates for that client."""
    import torch
    kind = torch.zeros(max(view.s.n_rows, 1), dtype=torch.uint8, device="cuda")  # PUB_UPDATE
    d = codec.publish_commit(pt, view, kind, heap=dbuf)
    assert d.n_unmatched == 0
    got, off = codec.encode_clients(view, d, dbuf)
    got, off = got.cpu().numpy().tobytes(), off.cpu().numpy().view(np.uint64)
    cols = dict(want_rows)
    cols.update({k: wcols[k] for k in ("ctag", "cfixed", "caux")})
    sent = 0
    for c in range(N_CLIENTS):
        mine = [k for k, p in enumerate(want_rows["id"].tolist()) if c in clients_of[p]]
        want = cfm.client_payload(cols, buf, mine) if mine else b""
        assert got[int(off[c]):int(off[c + 1])] == want, f"client {c}"
        sent += len(mine)
    assert sent > 100
    return d


def test_chain_window(codec):
    taw, buf, recs, n_live = chain_window()
    cols, infos, dbuf = taw.run_window(codec, buf, recs, 0)
    w = cols.numpy()
    pairs = [(f.row_off, f.n_rows) for f in infos]
    table = replay_table(64)
    want = rm.window_loop(w, pairs, table)
    assert want.n_done == n_live and want.n_miss and want.n_dropped  # stopped at the wide Ids
    assert {12, 19, 21, 22, 16} <= set(want.rows["tag"].tolist())
    rows = codec.replay_window(cols, infos, dev(table, np.int64))
    assert (rows.n_rows, rows.n_done, rows.n_dropped, rows.n_miss) == (
        want.n_rows, want.n_done, want.n_dropped, want.n_miss)
    got = rows.numpy()
    for k in rm.ROW_COLS:
        assert np.array_equal(got[k], want.rows[k]), k
    assert np.array_equal(rows.misses(), want.miss[:64])
    pt, clients_of, pubs = publisher(table)
    view = rows.columns(cols)
    d = check_clients(codec, view, dbuf, pt, clients_of, want.rows, w, buf)
    # Speed::Limited: record by record, the same arrays at an offset -- the same bytes per client
    whole, woff = codec.encode_clients(view, d, dbuf)
    whole, woff = whole.cpu().numpy().tobytes(), woff.cpu().numpy().view(np.uint64)
    parts = [b""] * N_CLIENTS
    import torch
    for i in range(rows.n_done):
        v = rows.record(i, cols)
        if v.s.n_rows == 0:
            continue
        di = codec.publish_commit(pt, v, torch.zeros(v.s.n_rows, dtype=torch.uint8, device="cuda"),
                                  heap=dbuf)
        b, o = codec.encode_clients(v, di, dbuf)
        b, o = b.cpu().numpy().tobytes(), o.cpu().numpy().view(np.uint64)
        for c in range(N_CLIENTS):
            parts[c] += b[int(o[c]):int(o[c + 1])]
    # a client's frame of many records is the records' frames: same messages, one after another
    for c in range(N_CLIENTS):
        assert parts[c] == whole[int(woff[c]):int(woff[c + 1])], f"client {c}"
    # the value table takes the view as it is: `current` becomes each Id's last update
    from netidx_amd.codec import ValueTable
    vt = ValueTable(codec, len(pubs), 1 << 16, 1 << 12).init()
    res = vt.apply(view, d.last_row, dbuf, dbuf.numel())
    last = d.last_row.cpu().numpy().view(np.uint64)
    assert res["n_applied"] == int((last != 0).sum()) > 10
    t = vt.numpy()
    for s in np.flatnonzero(last).tolist():
        k = int(last[s]) - 1
        assert awm.value(t["tag"][s], t["fixed"][s], t["aux"][s], t, t["heap"]) == \
            awm.value(want.rows["tag"][k], want.rows["fixed"][k], want.rows["aux"][k], w, buf)


def test_chain_image(codec):
    taw, buf, recs, n_live = chain_window()
    cols, infos, dbuf = taw.run_window(codec, buf, recs[:n_live], 0)
    w = cols.numpy()
    n_ids = 64
    img = codec.archive_build_image(cols, n_ids)
    image = img.numpy()
    assert 0x40 in image["tag"].tolist() and {12, 19} <= set(image["tag"].tolist())
    table = replay_table(n_ids + 8)
    table[5] = rm.MISS
    order = np.random.RandomState(3).permutation(n_ids + 12).astype(np.uint32)  # the pathmap
    want = rm.image_loop(image, order, table)
    assert want.n_miss and want.n_dropped and (want.rows["src_row"] == np.uint64(rm.U64_MAX)).any()
    rows = codec.replay_image(img, dev(order, np.int32), dev(table, np.int64))
    assert (rows.n_rows, rows.n_done, rows.n_dropped, rows.n_miss) == (
        want.n_rows, 1, want.n_dropped, want.n_miss)
    got = rows.numpy()
    for k in rm.ROW_COLS:
        assert np.array_equal(got[k], want.rows[k]), k
    assert np.array_equal(rows.misses(), want.miss[:64])
    pt, clients_of, _ = publisher(table)
    check_clients(codec, rows.columns(cols), dbuf, pt, clients_of, want.rows, w, buf)
