"""CPU checks for the archive window (nxg_archive_decode_window / nxg_archive_build_image,
include/nxg_codec.h): the sequential model of tests/archive_window_model.py on a hand-written
window with known answers, its fold against a direct restatement of build_image's
(netidx-archive/src/logfile/reader.rs:519-552), the two exported symbols, and the misuse cases
that return false before any device work. No GPU compute is called here."""
import ctypes as C
import json
import os
import random

import numpy as np

import archive_window_model as awm
import netidx_amd
from netidx_amd import codec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = {b["name"]: b for b in json.load(open(os.path.join(GOLD, "manifest.json")))["archive"]}


def fixture(name):
    return open(os.path.join(GOLD, MANIFEST[name]["file"]), "rb").read()


# one Array row: count 1 | Id 9 | Array of 2 | U32 7 | U32 8
ARRAY_REC = bytes.fromhex("01" "09" "13" "02" "0000000007" "0000000008")


def three_record_window():
    """pad(3) | ref_basic | junk(5) | long | ARRAY_REC + 2 trailing bytes; slots in that order."""
    a, b = fixture("ref_basic"), fixture("long")
    buf = b"\xee" * 3 + a + b"\xff" * 5 + b + ARRAY_REC + b"\x05\x05"
    o1 = 3
    o2 = o1 + len(a) + 5
    o3 = o2 + len(b)
    return np.frombuffer(buf, np.uint8), [(o1, len(a)), (o2, len(b)), (o3, len(ARRAY_REC) + 2)], o2


def test_model_on_a_hand_written_window():
    buf, recs, o2 = three_record_window()
    cols, infos = awm.window(buf, recs)
    lg = MANIFEST["long"]
    assert lg["consumed"] == 23961 and len(lg["expect"]["children"]) == 300
    rows = [list(map(int, r)) for r in zip(cols["id"], cols["tag"], cols["fixed"], cols["aux"])]
    assert rows == [
        [0, 4, 42, 0], [1, 4, 42, 0],                      # ref_basic
        [3, 12, 5 + o2, 5000], [4, 13, 5009 + o2, 10240],  # long: text offsets in the buffer
        [5, 64, 0, 0], [6, 19, 0, 300], [7, 12, 17959 + o2, 6000], [8, 16, 0, 0],
        [9, 19, 300, 2],                                   # the array after long's 300 children
    ]
    ch = [list(map(int, r)) for r in zip(cols["ctag"], cols["cfixed"], cols["caux"])]
    assert ch == lg["expect"]["children"] + [[0, 7, 0], [0, 8, 0]]
    want = [(0, 2, 0, 0, 21), (2, 6, 0, 300, 23961), (8, 1, 300, 2, len(ARRAY_REC))]
    for f, w in zip(infos, want):
        assert (f["row_off"], f["n_rows"], f["child_off"], f["n_children"], f["consumed"]) == w
        assert f["err_kind"] == 0 and f["err_offset"] == 0


def test_model_failing_and_skipped_records_stand_alone():
    good = fixture("unsub_only")
    bad = bytes.fromhex("020504000000000000002a061c")  # bad_tag: UnknownTag at 11
    buf = np.frombuffer(good + bad + good, np.uint8)
    recs = [(0, len(good)), (len(good), len(bad)), (len(good) + len(bad), len(good), 2),
            (len(good) + len(bad), len(good))]
    cols, infos = awm.window(buf, recs)
    assert cols["id"].tolist() == [7, 4294967295, 7, 4294967295]
    assert [(f["n_rows"], f["err_kind"], f["err_offset"], f["consumed"]) for f in infos] == \
        [(2, 0, 0, 9), (0, 1, 11, 0), (0, 0, 0, 0), (2, 0, 0, 9)]
    assert [f["row_off"] for f in infos] == [0, 2, 2, 2]


def test_model_fold_is_the_reference_fold():
    rng = random.Random(5)
    for keep_mode in ("none", "all", "some", "nothing"):
        n_ids = 40
        batches = [[(rng.randrange(n_ids), (rng.choice([4, 9, 64]), rng.randrange(1000)))
                    for _ in range(rng.randrange(0, 30))] for _ in range(12)]
        flat = [it for b in batches for it in b]
        cols = {"id": np.array([i for i, _ in flat], np.uint64),
                "tag": np.array([e[0] for _, e in flat], np.uint8),
                "fixed": np.array([e[1] for _, e in flat], np.uint64),
                "aux": np.zeros(len(flat), np.uint32)}
        keep = {"none": None, "all": set(range(n_ids)), "nothing": set(),
                "some": {i for i in range(n_ids) if rng.random() < 0.5}}[keep_mode]
        mask = None if keep is None else np.array([i in keep for i in range(n_ids)], np.uint8)
        img, dropped = awm.image(cols, n_ids, mask)
        ref = awm.reference_fold(batches, keep)
        assert img["id"].tolist() == sorted(ref)
        got = {int(i): (int(t), int(f)) for i, t, f in zip(img["id"], img["tag"], img["fixed"])}
        assert got == ref
        assert dropped == sum(1 for i, _ in flat if keep is not None and i not in keep)
        for i, s in zip(img["id"], img["src_row"]):
            assert flat[int(s)][0] == int(i)


def test_model_fold_names_an_id_out_of_range():
    cols = {"id": np.array([1, 5, 2], np.uint64), "tag": np.zeros(3, np.uint8),
            "fixed": np.zeros(3, np.uint64), "aux": np.zeros(3, np.uint32)}
    try:
        awm.image(cols, 5)
    except ValueError as e:
        assert "Id 5" in str(e) and "row 1" in str(e)
    else:
        raise AssertionError("an Id equal to n_ids must fail")


def test_library_exports_the_window_symbols():
    L = netidx_amd.lib()
    for f in ("nxg_archive_decode_window", "nxg_archive_build_image"):
        assert hasattr(L, f), f
        assert f in codec.SIGNATURES


def _host_cols(n=4, mem=codec.MEM_DEVICE, layout=netidx_amd.LAYOUT_MIXED):
    """An NxgColumns over host arrays (never dereferenced: the calls below fail first)."""
    keep = [np.zeros(n, np.uint64) for _ in range(11)]
    s = codec.NxgColumns()
    s.layout, s.mem = layout, mem
    s.cap_rows = s.cap_children = s.cap_ctl = n
    for a, (name, _, _) in zip(keep, codec.Columns.FIELDS):
        setattr(s, name, a.ctypes.data)
    return s, keep


def _window(ctx, buf_len, recs, cols, with_out=True):
    L = netidx_amd.lib()
    n = len(recs)
    r = (codec.NxgArchiveRecord * max(n, 1))()
    for i, (o, ln) in enumerate(recs):
        r[i].out_off, r[i].out_len = o, ln
    info = (codec.NxgArchiveBatchInfo * max(n, 1))()
    buf = np.zeros(max(buf_len, 1), np.uint8)
    nr, nc, err = C.c_uint64(0), C.c_uint64(0), codec.NetidxError()
    ok = L.nxg_archive_decode_window(ctx, C.c_void_p(buf.ctypes.data), buf_len, r, n, None,
                                     C.byref(cols) if with_out else None, info, C.byref(nr),
                                     C.byref(nc), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    L.nxg_error_free(C.byref(err))
    return ok, msg


def test_window_misuse_fails_before_any_device_work():
    cols, keep = _host_cols()
    ok, msg = _window(None, 16, [(0, 8)], cols, with_out=False)
    assert not ok and "null argument" in msg
    host, keep2 = _host_cols(mem=codec.MEM_HOST)
    ok, msg = _window(None, 16, [(0, 8)], host)
    assert not ok and "device MIXED" in msg
    f64, keep3 = _host_cols()
    f64.tag = None
    ok, msg = _window(None, 16, [(0, 8)], f64)
    assert not ok and "device MIXED" in msg
    for rec in [(9, 8), (17, 0), (0, 17), (2**63, 2**63)]:
        ok, msg = _window(None, 16, [(0, 8), rec], cols)
        assert not ok and "record 1" in msg and "outside" in msg, (rec, msg)
    ok, msg = _window(None, 16, [(0, 8), (8, 8)], cols)  # well-formed, but no ctx
    assert not ok and "null argument" in msg


def test_image_misuse_fails_before_any_device_work():
    L = netidx_amd.lib()

    def call(cols, img, n_ids=4):
        err = codec.NetidxError()
        ok = L.nxg_archive_build_image(None, C.byref(cols) if cols is not None else None, n_ids,
                                       None, C.byref(img) if img is not None else None,
                                       C.byref(err))
        msg = err.msg.decode() if err.msg else ""
        L.nxg_error_free(C.byref(err))
        return ok, msg

    cols, keep = _host_cols()
    cols.n_rows = 3
    arrs = [np.zeros(4, np.uint64) for _ in range(5)]
    img = codec.NxgArchiveImage()
    img.cap_rows = 3
    img.id, img.tag, img.fixed, img.aux, img.src_row = (a.ctypes.data for a in arrs)
    ok, msg = call(None, img)
    assert not ok and "null argument" in msg
    ok, msg = call(cols, None)
    assert not ok and "null argument" in msg
    host, keep2 = _host_cols(mem=codec.MEM_HOST)
    ok, msg = call(host, img)
    assert not ok and "device MIXED" in msg
    img.cap_rows = 2  # < min(n_ids = 4, 3 rows)
    ok, msg = call(cols, img)
    assert not ok and "capacity" in msg
    img.cap_rows = 3
    img.src_row = None
    ok, msg = call(cols, img)
    assert not ok and "null output array" in msg
    img.src_row = arrs[4].ctypes.data
    ok, msg = call(cols, img)  # well-formed, but no ctx
    assert not ok and "null argument" in msg
