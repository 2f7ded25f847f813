"""The case table of the decoder bounds tests (tests/decode_bounds_cases.py), checked on the
oracle alone: the GPU tests compare the device's outcome with the oracle's case by case, so the
table itself has to hold what it says -- every "short" case is a capacity error and nothing else,
every "exact" case decodes, every frame is well formed -- and has to reach the shapes it is for."""
import numpy as np

import decode_bounds_cases as dbc
import nxo


def _outcome(key, caps):
    return int(nxo.decode(dbc.wire(key), cap_rows=caps[0], cap_children=caps[1],
                          cap_ctl=caps[2]).s.err_kind)


def test_decode_bounds_cases_cpu():
    table = dbc.all_cases()
    for jobs in dbc.backlog_cases().values():
        assert [s for _, _, s in jobs] == [False, True, False]
        table += [dbc.Case("backlog", k, dbc.LAYOUT_F64, 0, caps, short, "backlog")
                  for k, caps, short in jobs]
    assert len(table) > 150
    for key in {c.frame for c in table}:
        o = nxo.decode(dbc.wire(key))  # room to spare: the frame itself is well formed
        assert o.s.err_kind == 0, key
        assert dbc.need(key) == (o.s.n_rows, o.s.n_children, o.s.n_ctl)
    for c in table:
        nd = dbc.need(c.frame)
        if c.layout == dbc.LAYOUT_F64:
            assert nd[1:] == (0, 0), c
        assert c.short == any(cap < n for cap, n in zip(c.caps, nd)), c
        assert c.caps[0] >= 0 and min(c.caps[1:]) >= 1, c
        assert _outcome(c.frame, c.caps) == (dbc.CAPACITY if c.short else 0), c
    # every decoder has short and exact cases, the exact one of a frame first
    for d in dbc.DECODERS:
        for key in dbc.frames_of(d):
            cs = dbc.cases(d, key)
            assert not cs[0].short and any(c.short for c in cs), (d, key)
    assert [c.caps[0] for c in dbc.cases("seq", ("seq", 2, 0))] == [2, 1, 0]
    archive = dbc.archive_cases()
    assert [s for _, _, s in archive] == [False, True, True]
    for label, (cr, cc), short in archive:
        d, r = nxo.decode_archive(dbc.archive_wire(), cr, cc)
        assert d.s.err_kind == (dbc.CAPACITY if short else 0), label
        assert short or r == len(dbc.archive_wire())


def test_decode_bounds_frames_reach_their_branches():
    # sequential ids: 12-byte records at ids below 2^7, 13 up to 2^14, 14 from there
    for i0, first, last in ((0, 12, 13), (100, 12, 13), (16300, 13, 14)):
        w = dbc.wire(("seq", 3001, i0))
        assert w[0] == first and len(w) > 3001 * first
        assert dbc.need(("seq", 3001, i0)) == (3001, 0, 0)
    # uniform width in permuted order: every record 12 bytes, 2730 fill a 32 KiB tile
    for n in dbc.F64_N:
        w = dbc.wire(("run", n))
        assert len(w) == 12 * n and (w[::12] == 12).all()
    assert 12 * 2730 <= 32768 < 12 * 2731
    # three-byte ids in permuted order: every record 14 bytes, 2340 fill a tile, and no id is
    # within a tile's records of the next width (the length-run probe's two-run prediction)
    for key in [("run14", n) for n in dbc.RUN14_N] + [k for k, _, _ in dbc.backlog_cases()["run"]]:
        w, n = dbc.wire(key), key[1]
        assert len(w) == 14 * n and (w[::14] == 14).all()
        i14 = nxo.decode(w).id[:n].astype(np.int64)
        assert (np.diff(i14) != 1).any() and i14.min() >= 2**14 and i14.max() + 2341 < 2**21
    assert 14 * 2340 <= 32768 < 14 * 2341
    ids = nxo.decode(dbc.wire(("run", 6000))).id[:6000].astype(np.int64)
    assert (np.diff(ids) != 1).any()
    # mixed widths: records of 12 to 16 bytes
    o = nxo.decode(dbc.wire(("x", 6000)))
    widths = {int(x).bit_length() for x in o.id[:6000]}
    assert max(widths) > 28 and min(widths) <= 7
    # the flat frame: arrays of 2..5 scalars in every third Update, a Heartbeat every 50
    nd = dbc.need(("flat",))
    f = nxo.decode(dbc.wire(("flat",))).trim()
    assert nd[0] == 3000 and nd[2] == 60 and f["n_heartbeat"] == 60
    arr = f["tag"] == 19
    assert arr.sum() == 1000 and set(f["aux"][arr]) == {2, 3, 4, 5}
    assert not np.isin(f["ctag"], (19, 21, 22)).any()
    assert len(dbc.wire(("flat",))) > 8 * 4096
    # the rich frame: Maps, Error(Value) and containers inside containers inside containers
    r = nxo.decode(dbc.wire(("rich",))).trim()
    assert (r["tag"] == 21).any() and (r["tag"] == 22).any()
    inner = np.flatnonzero(np.isin(r["ctag"], (19, 21, 22)) & (r["caux"] > 0))
    firsts = r["cfixed"][inner].astype(np.int64)
    assert np.isin(r["ctag"][firsts], (19, 21, 22)).any()  # a third level
    assert len(r["ctl_row"]) > 10
