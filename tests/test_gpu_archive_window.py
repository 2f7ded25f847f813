"""GPU checks of nxg_archive_decode_window and nxg_archive_build_image (include/nxg_codec.h)
against the sequential model of tests/archive_window_model.py: the oracle's archive decoder per
record, concatenated; the image a dict fold. Every window runs three times -- big_record_bytes
default, 1 (every record through the single-batch decoder) and UINT64_MAX (every record the wave
kernels do not decline through them) -- and each run must equal the model in every row, child and
info field. Bit-exact: no tolerance is involved."""
import importlib.util
import json
import os
import random
import re

import numpy as np
import pytest

import archive_window_model as awm
import nxo

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
COLS = ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux")
U64_MAX = 2**64 - 1
ROUTES = (0, 1, U64_MAX)
PATH_WINDOW = 7
HEADER = os.path.join(os.path.dirname(GOLD), os.pardir, "include", "nxg_codec.h")
BIG_DEFAULT = int(re.search(r"#define NXG_ARCHIVE_WINDOW_BIG_DEFAULT (\d+)", open(HEADER).read()).group(1))


def _mg():
    spec = importlib.util.spec_from_file_location("mg", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


mg = _mg()


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def vi(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def item(i, v):
    return vi(i) + (b"\x40" if v is None else mg.enc_value(v))


def batch(items, count=None):
    return vi(len(items) if count is None else count) + b"".join(items)


F64 = (9, 0x400921FB54442D18)
GOOD = batch([item(3, F64), item(4, (12, b"ok")), item(5, None)])


def layout(records, gap=0, pad=0):
    """The buffer and slots of `records` (bytes each) laid back to back with `gap` junk bytes
    between them, after `pad` bytes."""
    parts, recs, off = [b"\xa5" * pad], [], pad
    for r in records:
        parts.append(r)
        recs.append((off, len(r)))
        off += len(r)
        if gap:
            parts.append(b"\x5a" * gap)
            off += gap
    return np.frombuffer(b"".join(parts), np.uint8), recs


def run_window(codec, buf, recs, big, cap_rows=None, cap_children=None):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    dbuf = torch.from_numpy(buf.copy()).cuda() if len(buf) else torch.zeros(1, dtype=torch.uint8).cuda()
    total = sum(r[1] for r in recs)
    cols = Columns(total // 2 + 1 if cap_rows is None else cap_rows,
                   total + 1 if cap_children is None else cap_children, 1,
                   netidx_amd.LAYOUT_MIXED, "cuda")
    infos = codec.archive_decode_window(dbuf[:len(buf)], recs, cols, big)
    return cols, infos, dbuf


def check_window(codec, buf, recs, wave=None):
    """The three routes against the model. wave: the records (indices) that the wave kernels
    must take on the UINT64_MAX route and, when shorter than the default big_record_bytes, on
    the default route (None: not checked)."""
    mcols, minfos = awm.window(buf, recs)
    for big in ROUTES:
        cols, infos, _ = run_window(codec, buf, recs, big)
        g = cols.numpy()
        assert cols.s.n_rows == len(mcols["id"]) and cols.s.n_children == len(mcols["ctag"])
        for k in COLS:
            assert np.array_equal(g[k], mcols[k]), (big, k)
        assert len(infos) == len(minfos)
        for i, (f, m) in enumerate(zip(infos, minfos)):
            for k in awm.INFO:
                assert getattr(f, k) == m[k], (big, i, k, getattr(f, k), m[k])
            skipped = len(recs[i]) > 2 and recs[i][2]
            if skipped:
                assert f.path == 0
            elif big == 1:
                assert f.path in (3, 5), (i, f.path)
            elif wave is not None:
                small = big == U64_MAX or recs[i][1] < BIG_DEFAULT
                assert (f.path == PATH_WINDOW) == (i in wave and small), (big, i, f.path)
    return mcols, minfos


def test_empty_window(codec):
    buf = np.zeros(0, np.uint8)
    for big in ROUTES:
        cols, infos, _ = run_window(codec, buf, [], big)
        assert infos == [] and cols.s.n_rows == 0 and cols.s.n_children == 0


def test_one_record(codec):
    buf, recs = layout([GOOD])
    m, _ = check_window(codec, buf, recs, wave={0})
    assert m["id"].tolist() == [3, 4, 5]


def test_item_counts(codec):
    """Records of 0, 1, 63, 64, 65 and 129 items: the rounds of 64 items per wave."""
    rng = random.Random(1)
    records = []
    for n in (0, 1, 63, 64, 65, 129):
        its = []
        for j in range(n):
            v = rng.choice([F64, (12, b"text-%d" % j), None, (19, [(0, j), (9, j)]), (1, j * 997)])
            its.append(item(rng.getrandbits(rng.choice([7, 14, 32])), v))
        records.append(batch(its))
    buf, recs = layout(records)
    check_window(codec, buf, recs, wave=set(range(6)))


def sized(n):
    """A record of exactly n bytes: f64 items and one Bytes item that takes up the slack."""
    k = (n - 300) // 10
    body = vi(k + 1) + b"".join(item(j & 0x7F, F64) for j in range(k))
    slack = n - len(body) - 4  # Id, tag 13, a two-byte length
    assert 128 <= slack < 16384
    r = body + b"\x01\x0d" + vi(slack) + b"\x7f" * slack
    assert len(r) == n
    return r


def test_record_lengths_around_the_stage(codec):
    records = [sized(n) for n in (4095, 4096, 4097, 4343, 4344, 4345, 8192, 8193)]
    buf, recs = layout(records)
    check_window(codec, buf, recs)
    buf, recs = layout(records, gap=3, pad=1)  # other alignments of the same records
    check_window(codec, buf, recs)


def test_items_across_the_stage_edge(codec):
    """An f64 item, a text and an array that start at every position from before the 4 KiB mark
    to past the stage image's end, behind small items and behind one long Bytes item; the
    records lie back to back, so their starts take every alignment."""
    probes = [item(300, F64), item(301, (12, ("straddle-é-" * 5).encode())),
              item(302, (19, [(9, 1), (12, b"el"), (0, 2), (10, (5, 6)), (4, 3)]))]
    records = []
    for start in range(4070, 4400):
        for p in probes:
            k = (start - 2) // 10 - 2
            small = [item(j & 0x7F, F64) for j in range(k)]
            rest = start - 2 - 10 * k - 3  # a Bytes item: Id, tag, one-byte length
            assert 0 <= rest < 128
            its = small + [b"\x02\x0d" + vi(rest) + b"\x80" * rest, p, item(1, None)]
            r = batch(its)
            assert len(vi(len(its))) == 2 and r.index(p) == start
            records.append(r)
            fill = start - 1 - 4  # count, Id, tag, two-byte length
            records.append(batch([b"\x02\x0d" + vi(fill) + b"\x09" * fill, p, item(1, None)]))
            assert records[-1].index(p) == start
    buf, recs = layout(records)
    check_window(codec, buf, recs, wave=set(range(len(records))))


def test_trailing_bytes_and_scattered_slots(codec):
    """Bytes after a batch inside its slot (items, garbage, zeros) are not read; slots with gaps,
    out of order and overlapping."""
    a = GOOD + batch([item(9, F64)]) + b"\xff" * 7
    b = batch([item(1, (12, b"x" * 300))]) + bytes(40)
    c = batch([], count=0) + b"\x09" * 5
    buf, recs = layout([a, b, c], gap=11, pad=5)
    check_window(codec, buf, recs, wave={0, 1, 2})
    back = [recs[2], recs[0], recs[1], recs[0]]
    check_window(codec, buf, back, wave={0, 1, 2, 3})


def test_more_records_than_waves(codec):
    """20,000 records of 1-3 items: more records than the chip holds waves (the stride loop)."""
    rng = random.Random(2)
    records = []
    for i in range(20_000):
        its = [item(rng.getrandbits(20), rng.choice([F64, (0, i), None, (12, b"r%d" % i)]))
               for _ in range(rng.randrange(1, 4))]
        records.append(batch(its))
    buf, recs = layout(records)
    m, infos = check_window(codec, buf, recs, wave=set(range(20_000)))
    assert len(m["id"]) == sum(f["n_rows"] for f in infos) >= 20_000


def test_every_leaf_tag_and_text_sizes(codec):
    rng = random.Random(3)
    leaves = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 23, 24, 25, 26, 27]
    its = []
    for t in leaves * 4:
        v = mg.rand_value(rng)
        while v[0] != t:
            v = mg.rand_value(rng)
        its.append(item(rng.getrandbits(28), v))
    # (an Abstract that ends with its record is left to the single-batch decoder: its length wrap
    # is clamped to the buffer)
    its.append(item(1, F64))
    texts = [b"", b"a", ("é" * 2500).encode(), b"z" * 5000]
    records = [batch(its), batch([item(i, (12, s)) for i, s in enumerate(texts)]),
               batch([item(1, (19, [(12, b""), (12, b"a"), (18, "€uro".encode()), (13, b"\xff")]))]),
               batch([b"\x01\x11"])]  # Null's second tag, normalised to 16
    buf, recs = layout(records)
    check_window(codec, buf, recs, wave={0, 1, 2, 3})


def declined_cases():
    cases = {
        "map": batch([item(1, (21, [((12, b"k"), (9, 1))]))]),
        "nested_array": batch([item(1, (19, [(19, [(9, 1)]), (9, 2)]))]),
        "array_128": batch([item(1, (19, [(0, j) for j in range(128)]))]),
        "id_6_bytes": batch([vi(1 << 35) + mg.enc_value(F64)]),
        "error_value": batch([item(1, (22, (9, 7)))]),
        "bad_utf8_long": batch([item(1, (12, b"a" * 5000 + b"\xc3\x28"))]),
        "bad_utf8_in_array": batch([item(1, (19, [(12, b"\xe2\x82")]))]),
        "bad_datetime": batch([item(1, (10, (2**62, 0)))]),
        "count_larger": batch([item(1, F64), item(2, F64)], count=3),
        "count_smaller": batch([item(1, F64), item(2, F64), item(3, F64)], count=2),
        "array_over_the_image": batch([item(1, (19, [(13, b"\x01" * 60) for _ in range(100)]))]),
        "empty_slot": b"",
    }
    for c in MANIFEST["archive_errors"]:
        cases["golden_" + c["name"]] = bytes.fromhex(c["hex"])
    # an item cut short, and an unknown tag
    cases["cut_short"] = batch([item(1, F64)])[:-3]
    cases["unknown_tag"] = batch([b"\x01\x1c\x00"])
    return cases


DECLINED = declined_cases()
# the cases that decode (through the single-batch decoder): no error
DECODES = {"map", "nested_array", "array_128", "id_6_bytes", "error_value", "count_smaller",
           "array_over_the_image"}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_and_failing_records(codec, name):
    """A record the wave kernels decline, or that fails, between two good records: its info is
    nxg_decode_archive_batch's status on the same bytes, its neighbours are unaffected."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    bad = DECLINED[name]
    buf, recs = layout([GOOD, bad, GOOD], gap=2)
    wave = {0, 2} | ({1} if name == "count_smaller" else set())
    m, minfos = check_window(codec, buf, recs, wave=wave)
    assert (minfos[1]["err_kind"] == 0) == (name in DECODES), minfos[1]
    # the single-batch decoder's status on the same bytes
    d = torch.from_numpy(np.frombuffer(bad + b"\0", np.uint8).copy()).cuda()
    one = Columns(len(bad) // 2 + 1, len(bad) + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    st, used = codec.decode_archive(d, len(bad), one, check=False)
    for big in ROUTES:
        _, infos, _ = run_window(codec, buf, recs, big)
        f = infos[1]
        assert (f.err_kind, f.err_offset) == (st.err_kind, st.err_offset)
        if not st.err_kind:
            assert (f.n_rows, f.n_children, f.consumed) == (st.n_rows, st.n_children, used)
        else:
            assert (f.n_rows, f.n_children, f.consumed) == (0, 0, 0)
        for k in (0, 2):
            assert (infos[k].n_rows, infos[k].err_kind, infos[k].consumed) == (3, 0, len(GOOD))


def test_capacity_one_short(codec):
    from netidx_amd.codec import WindowCapacity
    records = [GOOD, batch([item(1, (19, [(9, j) for j in range(7)]))]), GOOD,
               batch([item(1, (21, [((12, b"k"), (9, 1))]))])]
    buf, recs = layout(records)
    m, _ = awm.window(buf, recs)
    nr, nc = len(m["id"]), len(m["ctag"])
    assert nr == 8 and nc == 9
    for big in ROUTES:
        for cr, cc in ((nr - 1, nc), (nr, nc - 1)):
            with pytest.raises(WindowCapacity) as e:
                run_window(codec, buf, recs, big, cap_rows=cr, cap_children=cc)
            assert (e.value.need_rows, e.value.need_children) == (nr, nc)
        cols, infos, _ = run_window(codec, buf, recs, big, cap_rows=nr, cap_children=nc)
        g = cols.numpy()
        for k in COLS:
            assert np.array_equal(g[k], m[k]), k


def test_records_outside_the_buffer_and_pending_async(codec):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    buf, recs = layout([GOOD])
    with pytest.raises(netidx_amd.CodecError, match="outside"):
        run_window(codec, buf, [(0, len(buf) + 1)], 0)
    with pytest.raises(netidx_amd.CodecError, match="outside"):
        run_window(codec, buf, recs + [(len(buf) + 1, 0)], 0)
    # an async decode pending on the ctx
    from netidx_amd import synth
    ids, vals = synth.f64_columns(100)
    wire = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    out = Columns(100, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
    codec.decode_async(wire.data_ptr(), wire.numel(), out)
    try:
        with pytest.raises(netidx_amd.CodecError, match="pending"):
            run_window(codec, buf, recs, 0)
    finally:
        codec.sync()
    check_window(codec, buf, recs, wave={0})


@pytest.mark.parametrize("indexed", [False, True])
def test_with_the_decompressor(codec, indexed):
    """The batch + dict records of the zstd fixtures through archive_decompress; its records go
    straight into the window call, a corrupt record's err included."""
    ents = json.load(open(os.path.join(GOLD, "zstd_manifest.json")))["records"]
    rec = np.frombuffer(open(os.path.join(GOLD, "zstd_records.bin"), "rb").read(), np.uint8)
    zd = codec.zstd_dict(open(os.path.join(GOLD, "zstd_dict.bin"), "rb").read())
    es = [e for e in ents if e["batch"] and e["dict"] and e["indexed"] == indexed]
    assert len(es) >= 3
    src = rec.copy()
    e1 = es[1]
    src[e1["rec_off"] + 4 + e1["index_len"]] ^= 0xFF  # record 1: not a zstd frame (its magic)
    out, res = codec.archive_decompress(src, [(e["rec_off"], e["rec_len"]) for e in es], indexed, zd)
    assert res[1][2] != 0 and all(r[2] == 0 for i, r in enumerate(res) if i != 1)
    host = out.cpu().numpy()
    m, minfos = awm.window(host, res)
    assert minfos[1]["n_rows"] == 0 and sum(f["n_rows"] for f in minfos) > 0
    import netidx_amd
    from netidx_amd.codec import Columns
    total = sum(r[1] for r in res)
    for big in ROUTES:
        cols = Columns(total // 2 + 1, total + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
        infos = codec.archive_decode_window(out, res, cols, big)
        g = cols.numpy()
        for k in COLS:
            assert np.array_equal(g[k], m[k]), (big, k)
        for f, mi in zip(infos, minfos):
            for k in awm.INFO:
                assert getattr(f, k) == mi[k], (big, k)
        # the per-record decode of the same bytes
        for (oo, ol, er), f in zip(res, infos):
            if er:
                continue
            one = Columns(ol // 2 + 1, ol + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
            st, used = codec.decode_archive(out[oo:], ol, one, check=False)
            assert (st.err_kind, st.n_rows, st.n_children, used) == \
                (f.err_kind, f.n_rows, f.n_children, f.consumed)
            o = one.numpy()
            assert np.array_equal(o["id"], g["id"][f.row_off:f.row_off + f.n_rows])
            assert np.array_equal(o["tag"], g["tag"][f.row_off:f.row_off + f.n_rows])


# ---- the image ----------------------------------------------------------------------------------

def image_window(n_ids, n_records, seed, values=None):
    rng = random.Random(seed)
    values = values or [F64, (0, 5), None, (12, b"abc"), (1, 300)]
    records = []
    for r in range(n_records):
        its = [item(rng.randrange(n_ids), rng.choice(values)) for _ in range(rng.randrange(0, 12))]
        records.append(batch(its))
    return layout(records)


def check_image(codec, buf, recs, n_ids, keep=None):
    import torch
    cols, infos, dbuf = run_window(codec, buf, recs, 0)
    g = cols.numpy()
    want, dropped = awm.image(g, n_ids, keep)
    dkeep = None if keep is None else torch.from_numpy(np.asarray(keep, np.uint8).copy()).cuda()
    img = codec.archive_build_image(cols, n_ids, dkeep)
    got = img.numpy()
    assert img.n_rows == len(want["id"]) and img.n_filtered == dropped
    for k in ("id", "tag", "fixed", "aux", "src_row"):
        assert np.array_equal(got[k], want[k]), k
    return cols, img, dbuf, want


@pytest.mark.parametrize("n_ids", [1, 64, 65, 1025, 4096, 4097, 9000])
def test_image_table_sizes(codec, n_ids):
    """Ids on the scan's block edges (4096 flags per block) and the table's last entry."""
    buf, recs = image_window(n_ids, 60, n_ids)
    edge = [i for i in (0, 63, 64, 255, 256, 1023, 1024, 4095, 4096, n_ids - 1) if i < n_ids]
    extra = batch([item(i, (0, i)) for i in edge] + [item(edge[-1], None)])
    buf2, recs2 = layout([bytes(buf[o:o + n]) for o, n in recs] + [extra])
    cols, img, _, want = check_image(codec, buf2, recs2, n_ids)
    assert want["tag"][-1] == 0x40 and want["id"][-1] == n_ids - 1  # Unsubscribed stays, last event


def test_image_repeats_and_unsubscribed(codec):
    """An Id repeated across records and within one record; Unsubscribed as an Id's last event;
    every row carrying the same Id."""
    r1 = batch([item(5, (0, 1)), item(5, (0, 2)), item(6, (0, 3)), item(5, (0, 4))])
    r2 = batch([item(6, None), item(7, (12, b"seven")), item(5, (0, 9))])
    r3 = batch([item(7, None)])
    buf, recs = layout([r1, r2, r3])
    cols, img, _, want = check_image(codec, buf, recs, 8)
    assert want["id"].tolist() == [5, 6, 7] and want["tag"].tolist() == [0, 0x40, 0x40]
    assert want["fixed"].tolist() == [9, 0, 0] and want["src_row"].tolist() == [6, 4, 7]
    same = batch([item(3, (0, j)) for j in range(200)])
    buf, recs = layout([same, same])
    cols, img, _, want = check_image(codec, buf, recs, 4)
    assert want["id"].tolist() == [3] and want["src_row"].tolist() == [399]


def test_image_keep(codec):
    n_ids = 300
    buf, recs = image_window(n_ids, 80, 11)
    rng = np.random.default_rng(12)
    for keep in (np.ones(n_ids, np.uint8), np.zeros(n_ids, np.uint8),
                 (rng.random(n_ids) < 0.5).astype(np.uint8)):
        cols, img, _, want = check_image(codec, buf, recs, n_ids, keep)
        assert all(keep[int(i)] for i in want["id"])
    cols, img, _, want = check_image(codec, buf, recs, n_ids, np.zeros(n_ids, np.uint8))
    assert img.n_rows == 0 and img.n_filtered == cols.s.n_rows


def test_image_id_out_of_range_and_empty_window(codec):
    import netidx_amd
    buf, recs = layout([batch([item(1, F64), item(9, F64), item(12, F64)])])
    cols, _, _ = run_window(codec, buf, recs, 0)
    with pytest.raises(netidx_amd.CodecError, match=r"Id 9 at row 1\b"):
        codec.archive_build_image(cols, 9)
    assert codec.archive_build_image(cols, 13).n_rows == 3
    cols, _, _ = run_window(codec, np.zeros(0, np.uint8), [], 0)
    for n_ids in (0, 1, 100):
        img = codec.archive_build_image(cols, n_ids)
        assert img.n_rows == 0 and img.n_filtered == 0


RICH = [F64, (12, b"text"), (12, ("é€" * 40).encode()), None, (19, [(9, 1), (12, b"el"), (0, 2)]),
        (21, [((12, b"k"), (19, [(0, 1), (0, 2)]))]), (22, (9, 7)), (13, b"\x00\xff"), (19, []),
        (20, bytes(range(16))), (10, (5, 6)), (27, bytes(range(20)))]


def encode_image(codec, cols, img, dbuf):
    return codec.encode_archive(img.columns(cols), dbuf).cpu().numpy()


def image_values(bytes_):
    d, used = nxo.decode_archive(bytes_)
    o = d.trim()
    assert o["err_kind"] == 0 and used == len(bytes_)
    return awm.values(o, o, bytes_)


def test_image_encodes_as_the_image_record(codec):
    """encode_archive of the image view (the image's rows over the window's children, heap = the
    window's buffer), decoded by the oracle, is the model's image -- containers and text among
    the winners, so the encoder reaches children through `fixed` alone."""
    buf, recs = image_window(50, 40, 21, RICH)
    cols, img, dbuf, want = check_image(codec, buf, recs, 50)
    assert {19, 21, 22, 12} <= set(want["tag"].tolist())
    enc = encode_image(codec, cols, img, dbuf)
    g = cols.numpy()
    assert image_values(enc) == awm.values(want, g, buf)


def test_image_chains_over_windows(codec):
    """image(W1) encoded and made record 0 of W2 gives image(W1 + W2)."""
    n_ids = 70
    b1, r1 = image_window(n_ids, 30, 31, RICH)
    b2, r2 = image_window(n_ids, 30, 32, RICH)
    cols1, img1, d1, _ = check_image(codec, b1, r1, n_ids)
    enc = encode_image(codec, cols1, img1, d1)
    w2 = [enc.tobytes()] + [bytes(b2[o:o + n]) for o, n in r2]
    bc, rc = layout(w2)
    colsc, imgc, dc, wantc = check_image(codec, bc, rc, n_ids)
    # the whole history in one window
    ball, rall = layout([bytes(b1[o:o + n]) for o, n in r1] + [bytes(b2[o:o + n]) for o, n in r2])
    colsa, imga, da, wanta = check_image(codec, ball, rall, n_ids)
    assert awm.values(wantc, colsc.numpy(), bc) == awm.values(wanta, colsa.numpy(), ball)
    assert image_values(encode_image(codec, colsc, imgc, dc)) == \
        image_values(encode_image(codec, colsa, imga, da))
