"""The oneshot calls' expected results, checked without a GPU: the two restatements of
tests/oneshot_model.py agree on every case of tests/oneshot_cases.py, the model's bytes decode
through the decoder port to the filtered input, a hand-derived reply, the framing calls of the
library (host arithmetic: they load without a GPU) against the model at every width change of both
varints, every named case reaches the branch it names, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import oneshot_cases as oc
import oneshot_model as om
import record_model as rm
from value_table_cases import f64, source_of

K = oc.constants()
PATHMAPS = oc.pathmap_cases(K)
DELTAS = oc.deltas_cases(K)
REFUSALS = oc.deltas_refusal_cases(K)


# ---- the two restatements -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATHMAPS))
def test_pathmap_restatements_agree(name):
    paths = PATHMAPS[name][0]
    b1, sel1 = om.pathmap_python(paths)
    b2, sel2, n_sel = om.pathmap_numpy(paths)
    assert b1 == b2 and np.array_equal(sel1, sel2) and n_sel == int(sel1.sum())


@pytest.mark.parametrize("name", sorted(DELTAS))
def test_deltas_restatements_agree(name):
    win = DELTAS[name][0]
    assert om.deltas_refusal(win) is None
    assert om.deltas_python(win) == om.deltas_oracle(win)


@pytest.mark.parametrize("name", sorted(PATHMAPS))
def test_pathmap_case_reaches_its_branch(name):
    paths, want = PATHMAPS[name]
    p = oc.pathmap_plan(paths, K)
    assert oc.reaches(p, want), (want, {k: p[k] for k in want})


@pytest.mark.parametrize("name", sorted(DELTAS))
def test_deltas_case_reaches_its_branch(name):
    win, want = DELTAS[name]
    p = oc.deltas_plan(win, K)
    assert oc.reaches(p, want), (want, {k: p[k] for k in want})


def test_cases_cover_the_edges():
    plans = [oc.deltas_plan(w, K) for n, (w, _) in DELTAS.items()]
    assert {"scalar", "flat", "stack", "unsub"} <= set().union(*(p["walks"] for p in plans))
    assert any(p["direct"] for p in plans) and any(p["idle"] for p in plans)
    assert {1, 2, 3, 4, 5} <= set().union(*(p["id_widths"] for p in plans))
    pm = [oc.pathmap_plan(p, K) for p, _ in PATHMAPS.values()]
    assert {1, 2, 3, 4} <= set().union(*(p["id_widths"] for p in pm))
    assert {1, 2} <= set().union(*(p["len_widths"] for p in pm))
    assert any(p["direct"] and not p["long"] for p in pm) and any(p["long"] > 1 for p in pm)
    # (an Id of 5 bytes needs 2^28 Ids in a path index: not in the table)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_deltas_refusal_cases(name):
    win, what = REFUSALS[name]
    assert om.deltas_refusal(win) == what


def test_pathmap_refusal_cases():
    for name, (paths, off, lowest) in oc.pathmap_refusal_cases().items():
        o = off.astype(np.int64)
        bad = np.flatnonzero(o[1:] < o[:-1])
        assert len(bad) >= 2 or name.endswith("first"), name
        assert int(bad[0]) == lowest, name


# ---- model bytes -> decoder -> the filtered input ----------------------------------------------------------
def reply_of(paths, image_win, windows):
    """(reply bytes, (pathmap, image, deltas) objects) of one shard by restatement 1."""
    filterset, pathmap = om.do_oneshot_pathmap(paths)
    image = {}
    for _, batch in om.read_deltas(image_win):      # reimage: the last event per Id,
        for i, ev in batch:
            if i in filterset:                      # filtered (reader.rs reimage(Some(&filterset)))
                image[i] = ev
    image = {i: ev for i, ev in image.items() if i in pathmap}   # oneshot.rs:135
    deltas = []
    for w in windows:
        deltas.extend(om.do_oneshot_deltas(pathmap, om.read_deltas(w)))
    return om.pack_reply([om.pack_shard(pathmap, image, deltas)]), (pathmap, image, deltas)


def small_shard():
    paths = om.Paths([oc.path(5 + a % 9, a) if a % 4 else b"" for a in range(200)],
                     (np.arange(200) % 3 != 0).astype(np.uint8))
    sel = set(np.flatnonzero(om.pathmap_numpy(paths)[1]).tolist())
    src = oc._repeat(oc.rc.pool_source(), 400)
    ids = (np.arange(400, dtype=np.uint64) * np.uint64(7)) % np.uint64(230)
    w1 = om.Window(src, ids, oc.split(400, range(40, 400, 40)), range(10), [5] * 10, 200, sel)
    w2 = om.Window(src, ids[::-1].copy(), oc.split(400, [100, 101, 300]), [-1, 0, 1, 2],
                   [1_999_999_999, 0, 1, 2], 200, sel)
    return paths, w1, [w1, w2]


def test_model_bytes_decode_to_the_filtered_input():
    paths, iw, wins = small_shard()
    reply, (pathmap, image, deltas) = reply_of(paths, iw, wins)
    (pm, im, dl), = om.decode_reply(reply)
    assert pm == pathmap and im == image and dl == deltas
    assert all(i in pathmap for _, b in dl for i, _ in b) and all(b for _, b in dl)
    # restatement 2 and the framing model give the same bytes
    pmb = om.pathmap_numpy(paths)[0]
    imb = om.pack_hashmap(image, 12, lambda ev: ev)
    frags = [b"".join(om.deltas_oracle(w)) for w in wins]
    nd = sum(om.expected_deltas(w)[5] for w in wins)
    lay = om.shard_layout(len(pmb), len(imb), sum(map(len, frags)), nd)
    shard = lay["len_head"] + pmb + imb + lay["count_head"] + b"".join(frags)
    assert len(shard) == lay["shard_len"]
    head, rlen = om.reply_head([len(shard)])
    assert head + shard == reply and rlen == len(reply)


def test_known_answer_reply():
    """One shard, hand-derived. Paths: Id 1 -> "/a", Id 3 -> "/bc" (Id 2 has a path the filter
    does not match). Image: Id 1 = U32(7) (tag 0: 00 00000007), Id 3 Unsubscribed (40). Deltas:
    record 0 at (1, 2 ns) holds Id 2 only and is dropped whole; record 1 at (-1, 10^9 ns) holds
    Ids 3, 2, 1 and keeps 3 (Null: 10) and 1 (F64 1.0: 09 3ff0000000000000)."""
    paths = om.Paths([b"", b"/a", b"/x", b"/bc"], [1, 1, 0, 1])
    img = source_of([("sc", 0, 7, 0), ("sc", 0x40, 0, 0)])
    iw = om.Window(img, [1, 3], [(0, 2)], [0], [0], 4, {1, 3})
    src = source_of([f64(5.0), ("sc", 16, 0, 0), f64(6.0), f64(1.0)])
    w = om.Window(src, [2, 3, 2, 1], [(0, 1), (1, 3)], [1, -1], [2, 1_000_000_000], 4, {1, 3})
    reply, _ = reply_of(paths, iw, [w])
    pathmap = bytes.fromhex("02" "01" "02" "2f61" "03" "03" "2f6263")
    image = bytes.fromhex("02" "01" "0000000007" "03" "40")
    deltas = bytes.fromhex("01" "ffffffffffffffff" "3b9aca00" "02" "03" "10" "01" "093ff0000000000000")
    inner = pathmap + image + deltas
    assert len(inner) == 10 + 9 + 26
    shard = bytes([len(inner) + 1]) + inner            # 45 + 1 fits one byte
    want = bytes([1 + len(shard) + 1, 1]) + shard      # Lr counts itself and the shard count
    assert reply == want
    assert reply.hex() == ("3001" "2e" "0201022f6103032f6263" "020100000000070340"
                           "01ffffffffffffffff3b9aca0002031001093ff0000000000000")
    assert om.deltas_oracle(w) == [b"", deltas[1:]]
    assert om.expected_deltas(w)[3:] == (2, 2, 1)


# ---- the framing calls of the library ---------------------------------------------------------------------
def lib_layout(pm, im, dl, nd):
    from netidx_amd.codec import Codec
    lay = Codec.oneshot_shard_layout(pm, im, dl, nd)
    return dict(len_head=bytes(lay.len_head[:lay.len_head_len]),
                count_head=bytes(lay.count_head[:lay.count_head_len]),
                pathmap_off=lay.pathmap_off, image_off=lay.image_off, count_off=lay.count_off,
                deltas_off=lay.deltas_off, shard_len=lay.shard_len)


@pytest.mark.parametrize("inner", [125, 126, 127, 16381, 16382, 16383])
@pytest.mark.parametrize("n_deltas", [0, 127, 128])
def test_shard_layout_at_every_width_change(inner, n_deltas):
    cw = om.varint_len(n_deltas)
    pm, im = 40, 17
    dl = inner - pm - im - cw
    assert lib_layout(pm, im, dl, n_deltas) == om.shard_layout(pm, im, dl, n_deltas)
    widths = {125: 1, 126: 1, 127: 2, 16381: 2, 16382: 3, 16383: 3}
    assert len(om.shard_layout(pm, im, dl, n_deltas)["len_head"]) == widths[inner]


@pytest.mark.parametrize("inner", [125, 126, 127, 16381, 16382, 16383])
def test_reply_head_at_every_width_change(inner):
    from netidx_amd.codec import Codec
    for lens in ([inner - 1], [(inner - 1) // 2, inner - 1 - (inner - 1) // 2],
                 [1] * 127 + [inner - 1 - 127] if inner > 200 else [inner - 1]):
        assert Codec.oneshot_reply_head(lens) == om.reply_head(lens)
    many = [3] * 128       # the shard count's varint takes two bytes
    assert Codec.oneshot_reply_head(many) == om.reply_head(many)
    assert Codec.oneshot_reply_head([]) == om.reply_head([]) == (b"\x02\x00", 2)


def test_framing_refusals():
    from netidx_amd import CodecError
    from netidx_amd.codec import Codec
    top = om.MAX_ELEMS
    assert top == (1 << 31) // 64
    assert lib_layout(1, 1, 15 * top, top) == om.shard_layout(1, 1, 15 * top, top)
    with pytest.raises(CodecError) as g:
        Codec.oneshot_shard_layout(1, 1, 15 * (top + 1), top + 1)
    assert "TooBig" in str(g.value) and "delta records" in str(g.value)
    with pytest.raises(om.TooBig):
        om.shard_layout(1, 1, 15 * (top + 1), top + 1)
    # n_shards: the count alone decides (the lengths are not read past the refusal)
    import netidx_amd
    from netidx_amd.codec import NetidxError
    head, hl, err = (C.c_uint8 * 20)(), C.c_uint32(0), NetidxError()
    one = np.zeros(1, np.uint64)
    ok = netidx_amd.lib().nxg_oneshot_reply_head(one.ctypes.data, top + 1, head, C.byref(hl), None,
                                                 C.byref(err))
    assert not ok and b"TooBig" in err.msg and b"shards" in err.msg
    netidx_amd.lib().nxg_error_free(C.byref(err))
    with pytest.raises(om.TooBig):
        om.reply_head(range(top + 1))
    # lengths that would wrap the sum: each alone, and two together
    for lens in ([1 << 60], [(1 << 60) - 1, 1], [5, (1 << 59), (1 << 59)]):
        with pytest.raises(CodecError) as g:
            Codec.oneshot_reply_head(lens)
        assert "2^60" in str(g.value)
    assert Codec.oneshot_reply_head([(1 << 60) - 9]) == om.reply_head([(1 << 60) - 9])


def test_library_exports_and_binds_the_calls():
    import netidx_amd
    from netidx_amd import codec
    lib = netidx_amd.lib()
    for sym in ("nxg_oneshot_pack_pathmap", "nxg_oneshot_pack_deltas", "nxg_oneshot_shard_layout",
                "nxg_oneshot_reply_head", "nxg_oneshot_assemble_shard"):
        assert hasattr(lib, sym), sym
    for m in ("oneshot_pack_pathmap", "oneshot_pack_deltas", "oneshot_pack_deltas_into",
              "oneshot_shard_layout", "oneshot_reply_head", "oneshot_assemble_shard"):
        assert hasattr(codec.Codec, m), m


# ---- refusals that need no device ---------------------------------------------------------------------------
def _raw(fn, *args):
    import netidx_amd
    from netidx_amd.codec import NetidxError
    err = NetidxError()
    ok = getattr(netidx_amd.lib(), fn)(*args, C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    netidx_amd.lib().nxg_error_free(C.byref(err))
    return ok, msg


@pytest.mark.parametrize("null", ["paths", "out", "paths->path_off", "paths->path_bytes", "keep",
                                  "out->sel", "ctx"])
def test_pathmap_null_argument_is_refused_by_name(null):
    from netidx_amd.codec import NxgOneshotPathmap, NxgOneshotPaths
    a = np.zeros(64, np.uint64)
    p = a.ctypes.data
    paths = NxgOneshotPaths(4, None if null == "paths->path_off" else p,
                            None if null == "paths->path_bytes" else p)
    out = NxgOneshotPathmap(0, None, None if null == "out->sel" else p, 0, 0)
    ok, msg = _raw("nxg_oneshot_pack_pathmap", None, None if null == "paths" else C.byref(paths),
                   None if null == "keep" else p, None if null == "out" else C.byref(out))
    assert not ok and msg == f"null argument ({null})", msg


DELTA_NULLS = ["window", "info", "ts_secs", "ts_nanos", "sel", "out", "out->rec_off",
               "out->rec_items", "ctx"]


def raw_pack_deltas(ctx, null, cols=None, ptrs=None, n_ids=8):
    """nxg_oneshot_pack_deltas through ctypes with the argument named `null` a null pointer."""
    from netidx_amd.codec import NxgArchiveBatchInfo, NxgColumns, NxgOneshotDeltas
    a = np.zeros(64, np.uint64)
    p = ptrs or {k: a.ctypes.data for k in ("sel", "rec_off", "rec_items", "out")}
    if cols is None:
        from netidx_amd import codec
        cols = NxgColumns()
        cols.layout, cols.mem = codec.LAYOUT_MIXED, codec.MEM_DEVICE
    info = (NxgArchiveBatchInfo * 2)()
    secs, nanos = np.zeros(2, np.int64), np.zeros(2, np.uint32)
    o = NxgOneshotDeltas(0, None, None if null == "out->rec_off" else p["rec_off"],
                         None if null == "out->rec_items" else p["rec_items"], 0, 0, 0, 0)
    return _raw("nxg_oneshot_pack_deltas", ctx, None if null == "window" else C.byref(cols), None,
                None if null == "info" else info, 2,
                None if null == "ts_secs" else secs.ctypes.data,
                None if null == "ts_nanos" else nanos.ctypes.data,
                None if null == "sel" else p["sel"], n_ids, None if null == "out" else C.byref(o))


@pytest.mark.parametrize("null", DELTA_NULLS)
def test_deltas_null_argument_is_refused_by_name(null):
    ok, msg = raw_pack_deltas(None, null)
    assert not ok and msg == f"null argument ({null})", msg


def test_assemble_refusals_before_the_ctx():
    from netidx_amd.codec import Codec, NxgOneshotFrag
    a = np.zeros(64, np.uint8)
    p = a.ctypes.data
    lay = Codec.oneshot_shard_layout(3, 2, 10, 1)
    fr = (NxgOneshotFrag * 2)(NxgOneshotFrag(p, 4), NxgOneshotFrag(p, 5))
    n = C.c_uint64(0)

    def call(layout=lay, pm=p, im=p, frags=fr, nf=2, out=p, cap=64):
        return _raw("nxg_oneshot_assemble_shard", None, C.byref(layout) if layout else None, pm,
                    im, frags, nf, out, cap, C.byref(n))

    for kw, word in ((dict(layout=None), "null argument (layout)"),
                     (dict(pm=None), "null argument (pathmap)"),
                     (dict(im=None), "null argument (image)"),
                     (dict(frags=None), "null argument (frags)"),
                     (dict(out=None), "null argument (out)"),
                     (dict(), "do not sum to the layout's deltas_len (10)")):
        ok, msg = call(**kw)
        assert not ok and word in msg, msg
    fr[1].len = 6
    ok, msg = call(cap=lay.shard_len - 1)
    assert not ok and "output buffer too small" in msg
    ok, msg = call()
    assert not ok and msg == "null argument (ctx)"
    bad = Codec.oneshot_shard_layout(3, 2, 10, 1)
    bad.deltas_off += 1
    ok, msg = call(layout=bad)
    assert not ok and "not what nxg_oneshot_shard_layout made" in msg
    assert (a == 0).all()


def test_deltas_equal_record_entries_with_timestamps():
    """The deltas elements are nxg_record_entries' records of the same filter, a timestamp in
    front of each (the model's second restatement leans on that; restatement 1 does not)."""
    win = DELTAS["values_all"][0]
    recs = rm.records_python(win.as_record_case())
    els = om.deltas_python(win)
    assert [e[12:] for e in els] == recs and all(len(e) > 12 for e in els)
