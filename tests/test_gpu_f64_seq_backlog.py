"""A backlog of sequential-id f64 frames in grouped launches (nxg_f64s_backlog_kernel,
netidx_amd/csrc/nxg_decode_f64_seq.hip; the grouping: plan_seq_backlog, nxg_api.cpp).

Every backlog here is decoded twice, with one launch per frame (NXG_F64S_GROUP=0, the reference)
and grouped (the default), into guarded columns (tests/guards.py) that start as sentinel bytes.
Both must leave the same bytes in every column array, capacity and guard band included, the same
row counts and the same status; the rows are then compared with the CPU oracle (tests/nxo.py).
NXG_F64S_GROUP_WGS caps the resident grid at 1, 2 or 3 workgroups (4, 8, 12 waves), so that at a
few thousand records a wave makes 1 to 5 rounds over tiles of 256 records, the last one partly
filled, and at a few hundred most waves have no tile at all.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import backlog_model as bm
import guards
import nxo

pytestmark = pytest.mark.gpu

WREC = 256
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 3000, 4097)
WGS = (1, 2, 3)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _codec(group, wgs):
    import netidx_amd
    with _env(NXG_F64S_GROUP=None if group else "0", NXG_F64S_GROUP_WGS=wgs, NXG_F64_PATH=None):
        return netidx_amd.Codec(0)


def _backlog_info(codec):
    a = (C.c_ulonglong * 4)()
    import netidx_amd
    netidx_amd.lib().nxg_debug_backlog(C.c_void_p(codec.ctx), a)
    return {"launches": int(a[0]), "frames": int(a[1]), "wgs": int(a[2]), "group": int(a[3])}


_wires = {}


def wire(n, first, seed=0):
    """(ids, vals, wire bytes) of n sequential ids from `first`; made once, never modified."""
    key = (n, first, seed)
    if key not in _wires:
        ids, vals = bm.seq_ids(n, first), bm.values(n, 7 * n + seed)
        _wires[key] = (ids, vals, nxo.encode_f64(ids, vals))
    return _wires[key]


class _View:
    """Columns that are a window of other memory (only .s is used by the codec)."""

    def __init__(self, id_ptr, fixed_ptr, cap_rows):
        import netidx_amd
        from netidx_amd.codec import NxgColumns
        self.s = NxgColumns()
        self.s.layout, self.s.mem = netidx_amd.LAYOUT_F64, 0
        self.s.cap_rows = cap_rows
        self.s.id, self.s.fixed = id_ptr, fixed_ptr


def _run(frames, caps, group, wgs, mixed=(), setup=None):
    """frames: (wire bytes or None for "given by setup", column set index) per frame, in backlog
    order; caps: cap_rows of column set k (sets in `mixed` have the MIXED layout).
    setup(dev_wires, cols) may return {frame index: (pointer, length)} and {set index: columns
    object} overrides. Returns what the backlog left behind, as host copies."""
    import torch
    import netidx_amd
    codec = _codec(group, wgs)
    try:
        cols = [guards.guarded_columns(cap, 8 if k in mixed else 0, 8 if k in mixed else 0,
                                       netidx_amd.LAYOUT_MIXED if k in mixed
                                       else netidx_amd.LAYOUT_F64, "cuda")
                for k, cap in enumerate(caps)]
        dev = [torch.from_numpy(np.ascontiguousarray(w).copy()).cuda()
               if w is not None and len(w) else torch.zeros(16, dtype=torch.uint8, device="cuda")
               for w, _ in frames]
        ptrs = [d.data_ptr() for d in dev]
        lens = [0 if w is None else len(w) for w, _ in frames]
        targets = [cols[c] for _, c in frames]
        if setup is not None:
            fo, co = setup(dev, cols)
            for j, (p, ln) in fo.items():
                ptrs[j], lens[j] = p, ln
            for j, t in co.items():
                targets[j] = t
        torch.cuda.synchronize()
        assert all(p % 16 == 0 for p in ptrs)
        codec.decode_frames_async(ptrs, lens, targets)
        err = None
        try:
            st = codec.sync(check=False)
            status = (int(st.n_rows), int(st.err_kind), int(st.n_heartbeat), int(st.path))
        except netidx_amd.CodecError as e:
            status, err = None, str(e)
        torch.cuda.synchronize()
        info = _backlog_info(codec)
        for c in cols:
            guards.assert_guards(c)
        return {
            "status": status, "error": err, "info": info,
            "n_rows": [int(t.s.n_rows) for t in targets],
            "id": [c.id.cpu().numpy().view(np.uint64) for c in cols],
            "fixed": [c.fixed.cpu().numpy().view(np.uint64) for c in cols],
            "wires": [d.cpu().numpy() for d in dev],
        }
    finally:
        codec.close()


def _both(frames, caps, wgs, launches=None, **kw):
    """The backlog ungrouped and grouped; asserts that they leave the same behind. Returns the
    grouped result."""
    ref = _run(frames, caps, False, wgs, **kw)
    got = _run(frames, caps, True, wgs, **kw)
    n_launch = sum(1 for w, _ in frames if w is None or len(w))
    assert ref["info"] == {"launches": n_launch, "frames": len(frames), "wgs": ref["info"]["wgs"],
                           "group": 0}
    assert got["info"]["group"] == 1 and got["info"]["frames"] == len(frames)
    assert got["info"]["wgs"] == (wgs if wgs else got["info"]["wgs"])
    if launches is not None:
        assert got["info"]["launches"] == launches
    assert got["status"] == ref["status"] and got["error"] == ref["error"]
    assert got["n_rows"] == ref["n_rows"]
    for k in range(len(caps)):
        assert got["id"][k].tobytes() == ref["id"][k].tobytes(), f"id column of set {k}"
        assert got["fixed"][k].tobytes() == ref["fixed"][k].tobytes(), f"value column of set {k}"
    for j in range(len(frames)):
        assert np.array_equal(got["wires"][j], ref["wires"][j])
    return got


def _assert_rows(got, k, ids, vals, lo=0):
    n = len(ids)
    assert np.array_equal(got["id"][k][lo:lo + n], ids), f"ids of set {k}"
    assert np.array_equal(got["fixed"][k][lo:lo + n], vals), f"values of set {k}"


def _assert_oracle(got, j, k, w):
    """Frame j (bytes w) is what column set k holds."""
    o = nxo.decode(np.ascontiguousarray(w)).trim()
    assert o["err_kind"] == 0 and got["n_rows"][j] == len(o["id"])
    _assert_rows(got, k, o["id"], o["fixed"])


@pytest.mark.parametrize("wgs", WGS)
def test_sizes_one_launch(wgs):
    # every size, from ids of one width and from ids that change width inside the first tile
    ws = [wire(n, 1000 + n) for n in SIZES] + [wire(n, 100) for n in SIZES]
    frames = [(w[2], j) for j, w in enumerate(ws)]
    got = _both(frames, [len(w[0]) for w in ws], wgs, launches=1)
    assert got["status"] == (SIZES[-1], 0, 0, 1)
    for j, w in enumerate(ws):
        _assert_oracle(got, j, j, w[2])


def _tiles_per_wave(w, wgs):
    tiles = (len(w) // 12 + 1 + WREC - 1) // WREC
    return (tiles + 4 * wgs - 1) // (4 * wgs)


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("n", (3000, 4097))
def test_width_change_positions(n, wgs):
    """The id width changes (at 2^7, 2^14, 2^21) at a tile's first record, at its last, at
    record 127 / 128 of a tile, and at the first and last record of a wave's range of tiles."""
    ws = []
    for b in (1 << 14, 1 << 21):
        k = _tiles_per_wave(wire(n, b - WREC)[2], wgs)  # (the frames below differ by < 1 tile)
        assert 1 <= k <= 5
        at = sorted({WREC, WREC - 1, 2 * WREC - 1, WREC + 127, WREC + 128,
                     k * WREC, k * WREC - 1, k * WREC + 1, 2 * k * WREC, 2 * k * WREC - 1})
        ws += [wire(n, b - r) for r in at if r < n]
        assert all(_tiles_per_wave(w[2], wgs) == k for w in ws[-len(at):])
    ws += [wire(n, (1 << 7) - r) for r in (1, 127, 128)]
    assert len(ws) <= 32
    frames = [(w[2], j) for j, w in enumerate(ws)]
    got = _both(frames, [n] * len(ws), wgs, launches=1)
    for j, w in enumerate(ws):
        _assert_oracle(got, j, j, w[2])


def test_a_wave_owns_one_to_five_tiles():
    ks = {(n, wgs): _tiles_per_wave(wire(n, 1000 + n)[2], wgs) for n in SIZES for wgs in WGS}
    assert set(ks.values()) == {1, 2, 3, 4, 5}
    assert ks[(4097, 1)] == 5 and ks[(3000, 1)] == 4 and ks[(1025, 2)] == 1


@pytest.mark.parametrize("n_frames,launches", ((1, 1), (2, 1), (3, 1), (32, 1), (33, 2), (40, 2)))
def test_launches_of_distinct_frames(n_frames, launches):
    ws = [wire(300 + j, 5000 + 400 * j) for j in range(n_frames)]
    frames = [(w[2], j) for j, w in enumerate(ws)]
    got = _both(frames, [len(w[0]) for w in ws], 2, launches=launches)
    for j, w in enumerate(ws):
        _assert_oracle(got, j, j, w[2])


def test_full_grid():
    # the grid the context chose for itself: every workgroup it keeps resident
    ws = [wire(n, 16000 + n) for n in (3000, 4097, 1025)]
    got = _both([(w[2], j) for j, w in enumerate(ws)], [len(w[0]) for w in ws], None, launches=1)
    assert got["info"]["wgs"] >= 256
    for j, w in enumerate(ws):
        _assert_oracle(got, j, j, w[2])


def test_empty_frame_in_the_middle():
    ws = [wire(1025, 9000), wire(300, 70), None, wire(3000, 16000), wire(257, 3)]
    frames = [((w[2] if w else np.zeros(0, np.uint8)), j) for j, w in enumerate(ws)]
    got = _both(frames, [len(w[0]) if w else 16 for w in ws], 1, launches=2)
    assert got["n_rows"][2] == 0
    assert (got["id"][2] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    for j, w in enumerate(ws):
        if w:
            _assert_oracle(got, j, j, w[2])


def test_shuffled_ids_in_the_middle_fall_back_alone():
    n = 3000
    rng = np.random.default_rng(11)
    pid, pv = bm.perm_ids(n, rng), bm.values(n, 5)
    seqs = [wire(n, 20000), wire(n, 40000)]
    fr = [seqs[0][2], bm.frame(pid, pv), seqs[1][2]]
    start = [(bm.seq_ids(n, 7), bm.values(n, 90 + c)) for c in range(3)]
    prog = bm.Program(n, fr, start, [bm.D(0, 0), bm.D(1, 1), bm.D(2, 2)], [(0, 3)])
    model = bm.run(prog)
    got = _both([(w, j) for j, w in enumerate(fr)], [n] * 3, 1, launches=1)
    assert got["status"] == (n, 0, 0, 1)
    for c in range(3):
        assert got["n_rows"][c] == model.cols[c]["n_rows"]
        _assert_rows(got, c, model.cols[c]["id"], model.cols[c]["fixed"])
    _assert_rows(got, 1, pid, pv)


def test_heartbeat_frame_in_the_middle_falls_back_alone():
    n = 1025
    a, b = wire(n, 300), wire(n, 70000)
    hid, hv = bm.seq_ids(n, 16000), bm.values(n, 3)
    h = bm.frame(hid, hv, heartbeat_at=600)
    got = _both([(a[2], 0), (h, 1), (b[2], 2)], [n] * 3, 2, launches=1, mixed=(1,))
    assert got["status"] == (n, 0, 0, 1)  # the last call's
    assert got["n_rows"] == [n, n, n]
    _assert_rows(got, 0, a[0], a[1])
    _assert_rows(got, 1, hid, hv)
    _assert_rows(got, 2, b[0], b[1])


def test_short_capacity_is_one_frames_error():
    import netidx_amd
    n = 1025
    ws = [wire(n, 1000), wire(n, 17000), wire(n, 33000)]
    got = _both([(w[2], j) for j, w in enumerate(ws)], [n, n - 1, n], 1, launches=1)
    assert got["status"][:2] == (n, netidx_amd.CAPACITY)  # the first failing call's
    _assert_rows(got, 0, ws[0][0], ws[0][1])
    _assert_rows(got, 1, ws[1][0][:n - 1], ws[1][1][:n - 1])
    _assert_rows(got, 2, ws[2][0], ws[2][1])
    # the neighbours alone complete without an error
    got = _both([(ws[0][2], 0), (ws[2][2], 1)], [n, n], 1, launches=1)
    assert got["status"] == (n, 0, 0, 1)


@pytest.mark.parametrize("wgs", WGS)
def test_seven_frames_into_three_rotating_sets(wgs):
    n = 4097
    ws = [wire(n, 16000, seed=j) for j in range(7)]  # the same ids (and length), other values
    assert len({len(w[2]) for w in ws}) == 1 and len({w[1].tobytes() for w in ws}) == 7
    got = _both([(w[2], j % 3) for j, w in enumerate(ws)], [n] * 3, wgs, launches=1)
    for k, j in ((0, 6), (1, 4), (2, 5)):
        _assert_rows(got, k, ws[j][0], ws[j][1])


@pytest.mark.parametrize("wgs", WGS)
def test_equal_length_other_count_later_frame_wins(wgs):
    # 1400 records of 13 bytes and 1300 of 14: the same length, so one launch; the later frame's
    # rows stay, and behind them the earlier frame's
    a, b = wire(1400, 1000), wire(1300, 20000)
    assert len(a[2]) == len(b[2]) == 18200
    got = _both([(a[2], 0), (b[2], 0)], [1400], wgs, launches=1)
    assert got["n_rows"] == [1300, 1300] and got["status"] == (1300, 0, 0, 1)
    _assert_rows(got, 0, b[0], b[1])
    _assert_rows(got, 0, a[0][1300:], a[1][1300:], lo=1300)
    got = _both([(b[2], 0), (a[2], 0)], [1400], wgs, launches=1)
    _assert_rows(got, 0, a[0], a[1])


def test_other_length_into_one_set_cuts():
    a, b = wire(3000, 1000), wire(2999, 50000)
    got = _both([(a[2], 0), (b[2], 0), (a[2], 1)], [3000, 3000], 1, launches=2)
    _assert_rows(got, 0, b[0], b[1])
    _assert_rows(got, 0, a[0][2999:], a[1][2999:], lo=2999)
    _assert_rows(got, 1, a[0], a[1])


def test_columns_shifted_by_128_rows_cut():
    n = 3000
    a, b = wire(n, 1000, seed=1), wire(n, 1000, seed=2)

    def setup(dev, cols):
        c = cols[0]
        return {}, {1: _View(c.id.data_ptr() + 128 * 8, c.fixed.data_ptr() + 128 * 8, n)}

    got = _both([(a[2], 0), (b[2], 0)], [n + 128], 1, launches=2, setup=setup)
    _assert_rows(got, 0, a[0][:128], a[1][:128])
    _assert_rows(got, 0, b[0], b[1], lo=128)


def test_wire_in_an_earlier_frames_columns_cuts():
    # the second frame's bytes are the value column that the first frame's decode leaves behind
    inner = wire(200, 5000)
    assert len(inner[2]) == 2600
    vals = np.frombuffer(inner[2].tobytes(), "<u8")
    ids = bm.seq_ids(len(vals), 300)
    outer = nxo.encode_f64(ids, vals)

    def setup(dev, cols):
        return {1: (cols[0].fixed.data_ptr(), len(inner[2]))}, {}

    got = _both([(outer, 0), (None, 1)], [len(vals), 200], 1, launches=2, setup=setup)
    assert got["status"] == (200, 0, 0, 1) and got["n_rows"] == [len(vals), 200]
    _assert_rows(got, 0, ids, vals)
    _assert_rows(got, 1, inner[0], inner[1])
    # the same between other frames, so that both launches are the backlog kernel's
    x, y = wire(1025, 9000), wire(257, 40000)

    def setup4(dev, cols):
        return {2: (cols[0].fixed.data_ptr(), len(inner[2]))}, {}

    got = _both([(x[2], 2), (outer, 0), (None, 1), (y[2], 3)], [len(vals), 200, 1025, 257], 1,
                launches=2, setup=setup4)
    _assert_rows(got, 0, ids, vals)
    _assert_rows(got, 1, inner[0], inner[1])
    _assert_rows(got, 2, x[0], x[1])
    _assert_rows(got, 3, y[0], y[1])


def test_columns_over_an_earlier_frames_wire_cut():
    # the second frame decodes into the memory that holds the first frame's bytes
    a, b = wire(3000, 1000), wire(2000, 30000)
    assert len(a[2]) >= 16 * 2000

    x, y = wire(1025, 9000), wire(257, 40000)

    def setup(dev, cols):
        p = dev[1].data_ptr()
        return {}, {2: _View(p, p + 8 * 2000, 2000)}

    got = _both([(x[2], 2), (a[2], 0), (b[2], 1), (y[2], 3)], [3000, 16, 1025, 257], 1,
                launches=2, setup=setup)
    assert got["status"] == (257, 0, 0, 1)
    _assert_rows(got, 0, a[0], a[1])
    _assert_rows(got, 2, x[0], x[1])
    _assert_rows(got, 3, y[0], y[1])
    mem = got["wires"][1][:16 * 2000].view(np.uint64)
    assert np.array_equal(mem[:2000], b[0]) and np.array_equal(mem[2000:], b[1])
