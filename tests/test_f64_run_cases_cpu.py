"""The case table of the length-run decoder and byte-range tests (tests/f64_run_cases.py), checked
without a GPU: the frames are well formed (the independent parser against the oracle), the tile
model gives every case's named tile its named class, the cases sit on the edges the table
promises, no frame holds an accidental candidate start, and the cut sets are as wide as promised.
A retune of the kernels' constants, or a rewrite of a statement the model restates, fails here.
"""
import numpy as np
import pytest

import f64_run_cases as fc
import nxo

K = fc.constants()
T = K["T"]
W_IDS = [c.name for c in fc.CASES]
R_FRAMES = {}
for _c in fc.RCASES:
    R_FRAMES.setdefault(_c.name.rsplit("-", 1)[0] if _c.offsets else _c.name, _c)


def _oracle(w):
    o = nxo.decode(np.ascontiguousarray(w), cap_rows=len(w) // 12 + 2, cap_children=1,
                   cap_ctl=4)
    return o.s, o.trim()


def test_constants_are_what_the_table_was_laid_out_for():
    got = {k: K[k] for k in fc.PINNED}
    assert got == fc.PINNED, ("the kernels' constants changed: read the cases of "
                              "tests/f64_run_cases.py against the new values, then update PINNED")


@pytest.mark.parametrize("name", W_IDS)
def test_frames_are_well_formed(name):
    c = fc.BY_NAME[name]
    w = fc.pristine(c) if c.corrupt else fc.wire(name)
    if c.heartbeat is not None:
        s, t = _oracle(w)
        assert (s.err_kind, s.n_rows, s.n_ctl, s.n_heartbeat) == (0, len(c.ids), 1, 1)
        assert np.array_equal(t["id"], c.ids) and np.array_equal(t["fixed"], fc.values(name))
        with pytest.raises(ValueError):
            fc.records(w)
        return
    r = fc.records(w)
    s, t = _oracle(w)
    assert s.err_kind == 0 and s.n_rows == len(r.start) == len(c.ids)
    assert np.array_equal(r.id, t["id"]) and np.array_equal(r.value, t["fixed"])
    assert np.array_equal(r.id, c.ids)
    assert int((r.start + r.length)[-1]) == len(w) and np.array_equal(r.start[1:],
                                                                      (r.start + r.length)[:-1])
    if c.corrupt:  # the corrupted frame differs in one byte, inside record c.corrupt[0]
        d = np.flatnonzero(fc.wire(name) != w)
        k = c.corrupt[0]
        assert len(d) == 1 and r.start[k] <= d[0] < r.start[k] + r.length[k]
        with pytest.raises(ValueError):  # no f64 frame any more
            fc.records(fc.wire(name))


@pytest.mark.parametrize("name", sorted(R_FRAMES))
def test_range_frames_are_well_formed(name):
    c = R_FRAMES[name]
    w = fc.rwire(c.name)
    assert 3 <= -(-len(w) // T) <= 5
    s, t = _oracle(w)
    if c.heartbeat is not None:
        assert (s.err_kind, s.n_rows, s.n_ctl, s.n_heartbeat) == (0, len(c.ids), 1, 1)
        assert np.array_equal(t["id"], c.ids) and np.array_equal(t["fixed"], fc.rvalues(c.name))
        return
    r = fc.records(w)
    assert s.err_kind == 0 and s.n_rows == len(r.start)
    assert np.array_equal(r.id, t["id"]) and np.array_equal(r.value, t["fixed"])


def _check_chain(plan, rec, W, begin, end):
    """Counts, entries and exits of a plan against the parser."""
    S = rec.start
    n = int(((S >= begin) & (S < end)).sum())
    assert sum(t.count for t in plan.tiles) == n
    for i, t in enumerate(plan.tiles):
        a0 = begin + i * T
        lim = min(end - a0, T)
        ent, ex, _, cnt = fc.expect_range(rec, W, a0, a0 + lim)
        assert (t.entry, t.count, t.x) == (ent - a0, cnt, ex - a0), (i, t)
        if i + 1 < len(plan.tiles):
            assert t.x == T + plan.tiles[i + 1].entry
    if plan.tiles:
        last = plan.tiles[-1]
        assert begin + (len(plan.tiles) - 1) * T + last.x == fc.expect_range(rec, W, end, end)[0]
        if end == W:
            assert begin + (len(plan.tiles) - 1) * T + last.x == W


@pytest.mark.parametrize("name", W_IDS)
def test_model_gives_the_named_tile_its_class(name):
    c = fc.BY_NAME[name]
    w = fc.pristine(c) if c.corrupt else fc.wire(name)
    assert 1 <= -(-len(w) // T) <= 9 and len(c.ids) <= 25000
    if c.heartbeat is not None:
        p = fc.tile_plan(w, flags=0)
        assert p.not_f64 and not p.bails and p.n_exact == 0
        a = fc.info(name)["heartbeat_at"]
        assert a == c.tile * T + 14 and len(fc.candidates(w[c.tile * T:c.tile * T + 16])) == 0
        return
    p = fc.tile_plan(w, flags=fc.F_NO_BAIL)
    assert not p.bails and not p.not_f64
    t = p.tiles[c.tile]
    assert t.cls == c.cls, (t, [x.cls for x in p.tiles])
    if c.ks is not None:
        assert t.ks == c.ks and t.L2 != t.L
    if c.count is not None:
        assert t.count == c.count
    assert p.n_exact == sum(x.cls == "exact" for x in p.tiles)
    _check_chain(p, fc.records(w), len(w), 0, len(w))
    # every tile on the exact walk, and the verdict without F_NO_BAIL
    px = fc.tile_plan(w, flags=fc.F_NO_BAIL | fc.F_FORCE_EXACT)
    assert px.n_exact == len(px.tiles) and [x.count for x in px.tiles] == [x.count for x in p.tiles]
    pb = fc.tile_plan(w, flags=0)
    assert pb.bails == (p.off_model * K["BAIL"] > len(p.tiles)) and not pb.not_f64
    if c.bail is not None:
        assert pb.bails == c.bail
    if c.planted is not None:  # the planted tile is exact, the others are runs
        assert [x.cls == "exact" for x in p.tiles] == [i == c.tile for i in range(len(p.tiles))]


def test_w1_frames_have_1_2_and_3_tiles():
    for L in (13, 14, 15, 16):
        for nt in (1, 2, 3):
            p = fc.tile_plan(fc.wire(f"W1-L{L}-{nt}t"), flags=fc.F_NO_BAIL)
            assert [t.cls for t in p.tiles] == ["one_run"] * nt and p.tiles[0].L == L


def test_w2_and_w3_cover_the_promised_splits():
    for nb in (1, 2, 3, 4):
        t0 = [c for c in fc.CASES if c.name.startswith(f"W2-x{7 * nb}-t0")]
        assert sorted(c.ks for c in t0) == sorted({1, 2, t0[0].count // 2, t0[0].count - 1})
        t1 = [c for c in fc.CASES if c.name.startswith(f"W2-x{7 * nb}-t1")]
        assert (len(t1) == 4) == (nb > 1)
        for c in t1:
            assert fc.tile_plan(fc.wire(c.name), flags=2).tiles[1].entry != 0
    for L, L2 in ((12, 13), (15, 16), (12, 14), (14, 12), (16, 15)):
        n1 = -(-T // L)
        step = (n1 + 62) // 63
        ks = sorted(c.ks for c in fc.CASES if c.name.startswith(f"W3-{L}to{L2}-"))
        assert ks[0] == 1 and ks[-1] == n1 - 1 and n1 // 2 in ks
        on = [k for k in ks if k % step == 0]
        assert len(on) == 1 and on[0] + 1 in ks and on[0] - 1 in ks
        c = fc.BY_NAME[f"W3-{L}to{L2}-ksn1-1"]  # only the last record of the tile is in run 2
        t = fc.tile_plan(fc.wire(c.name), flags=2).tiles[0]
        # (16-byte records end on the tile edge: record n1 - 1 and a 15-byte one behind it)
        assert t.ks == n1 - 1 and t.count - t.ks == (2 if L == 16 else 1)
        assert (t.L, t.L2) == (L, L2)


def test_w5_entries_are_sixteen_and_distinct():
    ent = []
    for c in fc.CASES:
        if c.family == "W5":
            p = fc.tile_plan(fc.wire(c.name), flags=fc.F_NO_BAIL)
            ent.append(p.tiles[1].entry)
            assert str(p.tiles[1].entry) == c.note and p.tiles[1].L == 12
            # a 12-byte record at an entry <= 3 puts two true starts in the window
            w = fc.wire(c.name)
            assert (len(fc.candidates(w[T:T + 17])) == 2) == (p.tiles[1].entry <= 3)
    assert sorted(ent) == list(range(16))


def test_w7_w8_w9_sit_where_the_table_says():
    EREC = K["EREC"]
    assert {len(fc.wire(c.name)) % T for c in fc.CASES if c.name.startswith("W7-T+")} == \
        {0, 1, 11, 12, 15, 16, 17}
    for c in fc.CASES:
        if c.wlen is not None:
            assert len(fc.wire(c.name)) == c.wlen, c.name
    assert len(fc.wire("W7-2T")) == 2 * T
    assert sorted(len(fc.wire(c.name)) for c in fc.CASES if "one-record" in c.name) == \
        [12, 13, 14, 15]
    for par in (0, 1):
        counts = sorted(c.count for c in fc.CASES if c.name.startswith(f"W8-base{par}-"))
        assert counts == [1, 63, 64, 65, EREC - 1, EREC, EREC + 1, 9 * EREC - 1, 9 * EREC,
                          9 * EREC + 1]
        for c in fc.CASES:
            if c.name.startswith(f"W8-base{par}-"):
                p = fc.tile_plan(fc.wire(c.name), flags=2)
                assert p.tiles[0].count & 1 == par and p.tiles[0].cls == "one_run"
    assert sorted(c.ks for c in fc.CASES if c.name.startswith("W8-split")) == \
        [EREC - 1, EREC, EREC + 1]
    assert fc.BY_NAME["W8-full-12"].count == -(-T // 12)
    # no run tile reaches 10 * EREC - 1 records: 13-byte records are the shortest a run tile
    # holds more than 128 of
    assert -(-T // 13) < 10 * EREC - 1
    g, u = fc.wire("W9-guarded"), fc.wire("W9-unguarded")
    assert np.array_equal(g, u[:len(g)])
    assert T + T + K["GUARD_AHEAD"] > len(g) and T + T + K["GUARD_AHEAD"] <= len(u)


def test_w10_frames_straddle_the_bail_ratio():
    keep, hand = fc.BY_NAME[f"W10-{K['BAIL']}-tiles"], fc.BY_NAME[f"W10-{K['BAIL'] - 1}-tiles"]
    pk, ph = (fc.tile_plan(fc.wire(c.name), flags=0) for c in (keep, hand))
    assert (len(fc.tile_plan(fc.wire(keep.name), flags=2).tiles), pk.off_model, pk.bails,
            pk.n_exact) == (K["BAIL"], 1, False, 1)
    assert (len(fc.tile_plan(fc.wire(hand.name), flags=2).tiles), ph.off_model, ph.bails,
            ph.n_exact) == (K["BAIL"] - 1, 1, True, 0)
    assert not 1 * K["BAIL"] > K["BAIL"] and 1 * K["BAIL"] > K["BAIL"] - 1


def test_w11_corrupts_a_record_the_probe_does_not_sample():
    for c in fc.CASES:
        if c.family != "W11":
            continue
        t = fc.tile_plan(fc.pristine(c), flags=2).tiles[0]
        m = t.count - 1
        sampled = {0, m // 2, m, t.ks - 1, t.ks}
        assert c.corrupt[0] not in sampled and c.corrupt[0] < t.count
        # the probe's verdict on the corrupted frame is the pristine frame's: it does not look
        assert fc.tile_plan(fc.wire(c.name), flags=2).tiles[0] == t
    assert {c.corrupt[1] for c in fc.CASES if c.corrupt} == {"tag", "variant", "length",
                                                            "continuation"}


def test_no_accidental_candidates():
    for c in fc.CASES:
        if c.heartbeat is not None:
            continue
        w = fc.pristine(c) if c.corrupt else fc.wire(c.name)
        extra = np.setdiff1d(fc.candidates(w), fc.records(w).start)
        if c.planted is None:
            assert len(extra) == 0, (c.name, extra[:4])
        else:
            fs = fc.info(c.name)["false_start"]
            assert list(extra) == [fs] and c.planted <= fs < c.planted + 16
            assert fc._rec(bytes(w), fs, len(w))[0] == 12  # it passes every per-record check
    for c in R_FRAMES.values():
        if c.heartbeat is not None:
            continue
        w = fc.rwire(c.name)
        extra = np.setdiff1d(fc.candidates(w), fc.records(w).start)
        if c.planted is None:
            assert len(extra) == 0, (c.name, extra[:4])
        else:
            assert list(extra) == [fc.rinfo(c.name)["false_start"]]


@pytest.mark.parametrize("prefix", ["R1-L12", "R1-L13", "R1-L14", "R1-L15", "R1-L16", "R1-split",
                                    "R5"])
def test_cut_sweeps_are_as_wide_as_promised(prefix):
    cs = [c for c in fc.RCASES if c.name.startswith(prefix + "-")]
    w = fc.rwire(cs[0].name)
    W, rec = len(w), fc.records(w)
    cuts = sorted({x[0] for c in cs for x in c.cuts})
    assert set(range(1, 81)) <= set(cuts) and set(range(W - 40, W + 1)) <= set(cuts)
    edges = (T,) if prefix != "R5" else (K["SUB"], K["X_WAVE_BYTES"], K["X_WG_BYTES"])
    for e in edges:
        assert set(range(e - 24, e + 25)) <= set(cuts)
    assert len([x for x in cuts if T < x < 2 * T]) >= 48
    for c in cs:  # every window holds all 16 phases
        assert {x[0] % 16 for x in c.cuts} == set(range(16)), c.name
    inner = np.array([x for x in cuts if x < W])
    k = np.searchsorted(rec.start, inner, side="right") - 1
    seen = {}
    for L, d in zip(rec.length[k], inner - rec.start[k]):
        seen.setdefault(int(L), set()).add(int(d))
    for L, ds in seen.items():
        assert ds == set(range(L)), (prefix, L, sorted(ds))
    if prefix == "R5":
        assert set(seen) == {12, 13, 14, 15, 16}
        assert fc.tile_plan(w, 0, W, 0).bails  # the run probe declines: record lengths vary


def test_other_range_cases_sit_where_the_table_says():
    for L in (13, 16):
        c = fc.RBY_NAME[f"R2-L{L}"]
        rec = fc.records(fc.rwire(c.name))
        holds = {}
        for a, e in c.cuts:
            n = int(((rec.start >= a) & (rec.start < e)).sum())
            holds.setdefault(e - a, set()).add(n > 0)
        assert set(holds) == {0, 1, 11, 12, 15, 16, 17, 31}
        for m, h in holds.items():  # with and without a start, wherever the length allows both
            assert h == ({False} if m == 0 else {True} if m >= L else {False, True}), (L, m, h)
    for name in ("R3-predicted", "R3-searched"):
        c = fc.RBY_NAME[name]
        rec = fc.records(fc.rwire(c.name))
        k = int(np.flatnonzero(np.diff(rec.length))[0]) + 1  # the first record of the new width
        assert [x[0] - int(rec.start[k]) for x in c.cuts] == [-1, 0, 1]
    for ctx in ("default", "run"):
        c = fc.RBY_NAME[f"R4-{ctx}"]
        fs = fc.rinfo(c.name)["false_start"]
        d = [fs - x[0] for x in c.cuts]
        assert set(range(0, 16)) <= set(d)        # (a) in [c, c + 16)
        assert set(range(-64, 0)) <= set(d)       # (b) in [c - 64, c); (c) is its last 16
    for name in ("R6-middle", "R6-tile-edge"):
        c = fc.RBY_NAME[name]
        assert len({b for b, _ in c.cuts}) == 1 and len(c.cuts) >= 32
        assert [e for _, e in c.cuts] == list(range(c.cuts[0][1], c.cuts[0][1] + len(c.cuts)))
    b = fc.RBY_NAME["R6-tile-edge"].cuts
    assert {e - b_ for b_, e in b} == set(range(T - 16, T + 17))


@pytest.mark.parametrize("name", [c.name for c in fc.RCASES])
def test_model_agrees_with_the_parser_on_ranges(name):
    """tile_plan() on a spread of the case's ranges: counts, entries and exits are the parser's."""
    c = fc.RBY_NAME[name]
    w = fc.rwire(name)
    if c.heartbeat is not None:
        # a range that begins where its first 16 bytes hold no record start is not f64 to the
        # probe; a Heartbeat deeper in a range is left to the emit's checks
        a = fc.rinfo(name)["heartbeat_at"]
        got = [[fc.tile_plan(w, b, e, 0).not_f64 for b, e in fc.ranges_of(len(w), cut)]
               for cut in c.cuts]
        assert [cut[0] - a for cut in c.cuts[:2]] == [-15, -14]
        assert got == [[False, True], [False, True], [False, False], [False, False],
                       [False, False, False]]
        return
    rec, W = fc.records(w), len(w)
    for cut in c.cuts[::max(1, len(c.cuts) // 6)]:
        for b, e in fc.ranges_of(W, cut):
            if b < e:
                _check_chain(fc.tile_plan(w, b, e, fc.F_NO_BAIL), rec, W, b, e)


def test_every_class_is_reached():
    cen = fc.class_census()
    for fam, d in cen.items():
        for cls, n in d.items():
            assert n > 0, (fam, cls, cen)
