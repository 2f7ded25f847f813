"""GPU tests of the write-batch direction (publisher::To): nxg_decode_writes and
nxg_encode_writes against the Python twin (tests/to_twin.py), which is written from the
reference's rules and shares no code with the library.

Bar: bit-exact columns (id, tag, fixed, aux, children, control spans, wflags, wid), the counts,
path 6, the twin's (PackError kind, offset of the first failing message) with all counts zero,
and byte-identical encoding. Every test takes a fresh Codec.
"""
import random
import struct

import numpy as np
import pytest

import to_twin as tw

pytestmark = pytest.mark.gpu


@pytest.fixture
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def dev(wire):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(wire), np.uint8).copy()).cuda()


def u64(xs):
    return np.array(list(xs), dtype=np.uint64)


def decode(codec, wire, host_frame=False, host_out=False):
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    n = len(wire)
    where = "cpu" if host_out else "cuda"
    cols = Columns(n // 5 + 1, n + 1, n // 3 + 1, LAYOUT_MIXED, where)
    wcols = WriteCols(n // 5 + 1, where)
    frame = bytes(wire) if host_frame or not n else dev(wire)
    codec.decode_writes(frame, cols, wcols, check=False)
    return cols, wcols, codec.writes_status


def assert_expected(codec, cols, wcols, st, e):
    assert (st.err_kind, st.path) == (0, 6)
    assert codec.last_status()[2] == 6
    assert (st.n_rows, st.n_children, st.n_ctl, st.n_heartbeat) == \
        (len(e.rows), len(e.children), len(e.ctl), 0)
    g = cols.numpy()
    w = wcols.numpy(st.n_rows)
    for k, name in enumerate(("id", "tag", "fixed", "aux")):
        assert np.array_equal(g[name].astype(np.uint64), u64(r[k] for r in e.rows)), name
    for k, name in enumerate(("ctag", "cfixed", "caux")):
        assert np.array_equal(g[name].astype(np.uint64), u64(r[k] for r in e.children)), name
    for k, name in enumerate(("ctl_row", "ctl_off", "ctl_len", "ctl_variant")):
        assert np.array_equal(g[name].astype(np.uint64), u64(r[k] for r in e.ctl)), name
    assert np.array_equal(w["wflags"].astype(np.uint64), u64(e.wflags))
    assert np.array_equal(w["wid"], u64(e.wid))


def check(codec, wire, e=None, **kw):
    """Decode `wire` and compare with the twin's decode of it (and with `e`, the columns the
    twin expects from the messages themselves, when given)."""
    d, err = tw.decode(wire)
    assert err is None
    if e is not None:
        for k in ("rows", "children", "ctl", "wflags", "wid"):
            assert getattr(d, k) == getattr(e, k), k
    cols, wcols, st = decode(codec, wire, **kw)
    assert_expected(codec, cols, wcols, st, d)
    return cols, wcols, d


def check_error(codec, wire, want=None):
    err = tw.first_error(wire)
    assert err is not None
    if want is not None:
        assert err == want
    cols, wcols, st = decode(codec, wire)
    assert (st.err_kind, st.err_offset) == err
    assert (st.n_rows, st.n_children, st.n_ctl) == (0, 0, 0)
    assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == (0, 0, 0)


def rand_wid(rng):
    k = rng.randrange(1, 11)  # varint bytes
    if k == 10:
        return rng.getrandbits(64) | (1 << 63)
    return rng.getrandbits(7 * k) | (1 << (7 * k - 1)) if k > 1 else rng.getrandbits(7)


def rand_id(rng):
    b = rng.choice([7, 14, 21, 28, 35, 36, 50, 64])
    return rng.getrandbits(b) | (1 << (b - 1))


def rand_writes(n, seed, wid=rand_wid):
    mg = tw.mg()
    rng = random.Random(seed)
    return [("w", rand_id(rng), rng.random() < 0.5, mg.rand_value(rng), wid(rng))
            for _ in range(n)]


def encode_from(codec, e, wire):
    """Columns from the twin's expected decode (heap = the frame) -> encode_writes."""
    import netidx_amd
    from netidx_amd.codec import WriteCols
    import torch
    r, c, k = e.rows, e.children, e.ctl
    cols = netidx_amd.columns_from_arrays(
        u64(x[0] for x in r), u64(x[2] for x in r), u64(x[1] for x in r).astype(np.uint8),
        u64(x[3] for x in r).astype(np.uint32), u64(x[0] for x in c).astype(np.uint8),
        u64(x[1] for x in c), u64(x[2] for x in c).astype(np.uint32),
        u64(x[0] for x in k), u64(x[1] for x in k), u64(x[2] for x in k).astype(np.uint32),
        u64(x[3] for x in k).astype(np.uint8))
    wc = WriteCols(len(r), "cuda")
    if r:
        wc.wflags[: len(r)].copy_(torch.from_numpy(np.array(e.wflags, np.uint8)))
        wc.wid[: len(r)].copy_(torch.from_numpy(u64(e.wid).view(np.int64)))
    torch.cuda.synchronize()
    return cols, wc, dev(wire) if wire else None


# ---- decode = twin ------------------------------------------------------------------------------
# 1-3: below one 64-byte lane chunk; 63/64/65: a wave of messages; 4096: across 4 KiB tiles;
# 30 000: several runs and workgroups
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 500, 4096, 30_000])
def test_random_writes_every_tag(codec, n):
    wire, e = tw.batch(rand_writes(n, 1000 + n))
    check(codec, wire, e)


def test_f64_writes_take_the_bucketed_emit(codec):
    rng = random.Random(5)
    msgs = [("w", rand_id(rng), rng.random() < 0.5, (9, rng.getrandbits(64)), rand_wid(rng))
            for _ in range(5000)]
    wire, e = tw.batch(msgs)
    check(codec, wire, e)
    assert codec.last_diag()[7] == 0  # no tile went to the per-lane work list


def test_short_flat_writes_take_the_bucketed_emit(codec):
    """Fixed-size, varint, text, time and flat-array values: the common write. (Ids of two or
    more bytes keep a 4 KiB tile at 512 messages or fewer, the bucketed path's table size.)"""
    mg = tw.mg()
    rng = random.Random(6)
    flat = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 23, 24, 25, 26]
    msgs = []
    while len(msgs) < 6000:
        v = mg.rand_value(rng, 3) if rng.random() < 0.2 else mg.rand_value(rng)
        if v[0] == 19:
            v = (19, [(9, rng.getrandbits(64)), (6, -rng.getrandbits(40)), (16, None)][: rng.randrange(4)])
        elif v[0] not in flat:
            continue
        msgs.append(("w", rng.getrandbits(20) | (1 << 13), rng.random() < 0.5, v, rand_wid(rng)))
    wire, e = tw.batch(msgs)
    check(codec, wire, e)
    assert codec.last_diag()[7] == 0


@pytest.mark.parametrize("size", [65, 200, 5200, 9000, 40_000],
                         ids=["over_a_lane", "200B", "past_the_image", "two_tiles", "ten_tiles"])
def test_long_values(codec, size):
    """A text value longer than 64 B leaves a lane without a message start; one above 5 KiB lies
    past the LDS image's look-ahead (the global-memory source); one above two tiles spans runs."""
    rng = random.Random(size)
    msgs = []
    for i in range(max(4, min(40, 400_000 // size))):  # about half a MiB at the most
        msgs.append(("w", i, True, (12, bytes(rng.choice(b"abcxyz") for _ in range(size))), i))
        msgs.append(("w", i, False, (9, rng.getrandbits(64)), rand_wid(rng)))
        if i % 7 == 0:
            msgs.append(("w", i, False, (13, bytes(rng.getrandbits(8) for _ in range(size))), 3))
    wire, e = tw.batch(msgs)
    check(codec, wire, e)


def test_unsubscribes_interleaved(codec):
    rng = random.Random(11)
    msgs = rand_writes(3000, 12)
    for _ in range(700):
        msgs.insert(rng.randrange(len(msgs) + 1), ("unsub", rand_id(rng)))
    wire, e = tw.batch(msgs)
    check(codec, wire, e)


@pytest.mark.parametrize("n", [1, 64, 5000])
def test_unsubscribes_only(codec, n):
    rng = random.Random(n)
    wire, e = tw.batch([("unsub", rand_id(rng)) for _ in range(n)])
    check(codec, wire, e)


def test_subscribes_between_writes(codec):
    rng = random.Random(13)
    msgs = rand_writes(1500, 14)
    for i in range(300):
        v6 = ("v6", [rng.getrandbits(16) for _ in range(8)], rng.getrandbits(16),
              rng.getrandbits(32), rng.getrandbits(32))
        v4 = ("v4", rng.getrandbits(32), rng.getrandbits(16))
        sub = dict(path="/app/é/%d" % i, resolver=rng.choice([v4, v6]),
                   timestamp=rng.getrandbits(64), permissions=rng.getrandbits(32),
                   token=bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 90))))
        msgs.insert(rng.randrange(len(msgs) + 1), ("sub", sub))
    wire, e = tw.batch(msgs)
    check(codec, wire, e)


def test_trailing_bytes_and_nonminimal_ids(codec):
    """Bytes inside L after the last field are skipped (pack.rs:551-553); id varints need not be
    minimal (pack.rs:504-520)."""
    rng = random.Random(15)
    parts = []
    for i in range(2000):
        k = rng.randrange(5)
        v = (9, rng.getrandbits(64)) if k < 3 else tw.mg().rand_value(rng)
        if k == 0:
            parts.append(tw.write(i, True, v, 7, trailing=b"junk"[: rng.randrange(1, 5)]))
        elif k == 1:
            parts.append(tw.write(5, False, v, 9, id_bytes=rng.choice([b"\x85\x00", b"\x85\x80\x80\x00"])))
        elif k == 2:
            parts.append(tw.unsubscribe(i, trailing=b"\x02\x02"))
        elif k == 3:
            parts.append(tw.subscribe("/t", token=b"x", trailing=b"\x00\x01"))
        else:
            parts.append(tw.write(i, False, v, rand_wid(rng)))
    check(codec, b"".join(parts))


def test_old_peers_without_write_id(codec):
    wire, e = tw.batch(rand_writes(3000, 16, wid=lambda rng: None))
    check(codec, wire, e)
    wire, e = tw.batch(rand_writes(3000, 17, wid=lambda rng: None if rng.random() < 0.5 else rand_wid(rng)))
    cols, wcols, d = check(codec, wire, e)
    assert 0 < sum(1 for f in d.wflags if f & tw.WRITE_NO_WID) < 3000


def test_write_id_truncated_by_the_length_prefix(codec):
    """BufferShort inside the WriteId varint means "absent" (netidx-derive lib.rs:392-401)."""
    mg = tw.mg()
    rng = random.Random(18)
    parts = []
    for i in range(1500):
        v = mg.enc_value((9, rng.getrandbits(64)) if i % 3 else mg.rand_value(rng))
        cut = b"\x80" * rng.randrange(1, 4) if i % 2 else mg.enc_varint(rand_wid(rng))
        parts.append(mg.enc_msg(2, mg.enc_varint(i) + b"\x01" + v + cut))
    wire = b"".join(parts)
    cols, wcols, d = check(codec, wire)
    assert sum(1 for f in d.wflags if f & tw.WRITE_NO_WID) == 750


def test_adversarial_payloads_look_like_write_headers(codec):
    """Text and Bytes payloads full of byte patterns that look like Write starts; the exact
    repair must still give the twin's answer."""
    rng = random.Random(19)
    fake1 = bytes.fromhex("060200001000")
    fake2 = bytes.fromhex("8f0602ac0201093ff000000000000005")
    msgs = []
    for i in range(600):
        L = rng.choice([30, 64, 100, 700, 6000])
        pat = rng.choice([fake1, fake2, b"\x90\x02", b"\xff\x05\x02\x01\x00\x0e"])
        msgs.append(("w", i, False, (13, (pat * (L // len(pat) + 1))[:L]), rand_wid(rng)))
        msgs.append(("w", i, True, (12, (fake1 * (L // 6 + 1))[:L]), 0))
        msgs.append(("w", i, True, (9, rng.getrandbits(64)), rand_wid(rng)))
        if i % 5 == 0:
            msgs.append(("unsub", 2))
    wire, e = tw.batch(msgs)
    check(codec, wire, e)


def test_cross_pin_with_the_c_oracle(codec):
    """Frames of fixed-width values: the To decode's id/tag/fixed/aux equal the C oracle's
    decode of the Update frame built from the same (id, value) list."""
    import nxo
    mg = tw.mg()
    rng = random.Random(20)
    fixed_tags = [0, 2, 4, 6, 8, 9, 10, 11, 14, 15, 16, 23, 24, 25, 26]
    pairs = []
    while len(pairs) < 5000:
        v = mg.rand_value(rng, 3) if rng.random() < 0.3 else mg.rand_value(rng)
        if v[0] in fixed_tags:
            pairs.append((rand_id(rng), v))
    wire, e = tw.batch([("w", i, False, v, n) for n, (i, v) in enumerate(pairs)])
    cols, wcols, d = check(codec, wire, e)
    o = nxo.decode(tw.update_frame(pairs)).trim()
    g = cols.numpy()
    for k in ("id", "tag", "fixed", "aux"):
        assert np.array_equal(g[k], o[k]), k


def test_host_frame_and_pinned_host_columns(codec):
    msgs = rand_writes(2500, 21)
    msgs[100:100] = [("unsub", 9), ("sub", dict(path="/h", token=b"tt"))]
    wire, e = tw.batch(msgs)
    check(codec, wire, e, host_frame=True)
    check(codec, wire, e, host_frame=True, host_out=True)
    check(codec, wire, e, host_out=True)


def test_empty_frame(codec):
    cols, wcols, st = decode(codec, b"")
    assert (st.err_kind, st.path, st.n_rows, st.n_children, st.n_ctl) == (0, 6, 0, 0, 0)


# ---- errors = the twin's (kind, offset); counts zero --------------------------------------------
def _w(body):
    return tw.mg().enc_msg(2, body)


GOOD = None


def good():
    global GOOD
    if GOOD is None:
        GOOD = [tw.write(i, i % 2 == 0, (9, i * 77), i) if i % 9 else tw.unsubscribe(i)
                for i in range(5000)]
    return GOOD


V6_SHORT = b"\x01" + b"\x00" * 20
BAD = {
    "bool_2": (lambda: _w(b"\x01\x02\x10\x00"), tw.UNKNOWN_TAG),
    "bool_missing": (lambda: _w(b"\x01"), tw.SHORT),
    "variant_3": (lambda: tw.mg().enc_msg(3, b"\x01"), tw.UNKNOWN_TAG),
    "variant_255": (lambda: tw.mg().enc_msg(255, b""), tw.UNKNOWN_TAG),
    "sub_sockaddr_tag_2": (lambda: tw.mg().enc_msg(0, b"\x02/a\x02" + b"\x00" * 30), tw.UNKNOWN_TAG),
    "sub_short_v6": (lambda: tw.mg().enc_msg(0, b"\x02/a" + V6_SHORT), tw.SHORT),
    "sub_token_too_big": (lambda: tw.mg().enc_msg(
        0, b"\x02/a" + tw.sockaddr(("v4", 1, 2)) + struct.pack(">QI", 1, 2) + b"\x09abc"), tw.TOO_BIG),
    "sub_bad_utf8_path": (lambda: tw.mg().enc_msg(
        0, b"\x02\xc3\x28" + tw.sockaddr(("v4", 1, 2)) + struct.pack(">QI", 1, 2) + b"\x00"), tw.INVALID),
    "len_zero": (lambda: b"\x00", tw.SHORT),
    "wid_varint_too_long": (lambda: _w(b"\x01\x00\x10" + b"\xff" * 10 + b"\x01"), tw.INVALID),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_error_alone_and_after_good_messages(codec, name):
    make, kind = BAD[name]
    bad = make()
    check_error(codec, bad, (kind, 0))
    pre = b"".join(good()[:50])
    check_error(codec, pre + bad + b"".join(good()[:10]), (kind, len(pre)))


def value_error_bodies():
    """The failing Update of each make_golden.errors() case whose error lies in the value,
    as (name, value bytes, kind)."""
    out = []
    for name, wire, kind, off in tw.mg().errors():
        m = wire[off:]
        if len(m) < 4 or m[0] >= 0x80 or m[1] != 4 or m[2] != 1 or m[0] != len(m):
            continue
        out.append((name, m[3:], kind))
    return out


def test_bad_values_inside_writes(codec):
    bodies = value_error_bodies()
    assert len(bodies) >= 6
    for name, v, kind in bodies:
        bad = _w(b"\x01\x00" + v)
        assert tw.first_error(bad) == (kind, 0), name
        pre = b"".join(good()[:30])
        check_error(codec, pre + bad + good()[0], (kind, len(pre)))


def test_length_prefix_past_the_frame(codec):
    """A prefix that runs past the frame limits the fields to the frame (pack.rs:537-555): the
    value is cut short."""
    pre = b"".join(good()[:100])
    bad = b"\x7f\x02\x01\x00\x09\x00\x00"
    check_error(codec, pre + bad, (tw.SHORT, len(pre)))
    check_error(codec, pre + b"\x85", (tw.SHORT, len(pre)))  # the prefix itself is cut


@pytest.mark.parametrize("at", [0, 2500, 4999], ids=["first", "middle", "last"])
def test_error_position_in_a_long_frame(codec, at):
    msgs = list(good())
    msgs[at] = _w(b"\x01\x02\x10\x00")
    off = sum(len(m) for m in msgs[:at])
    check_error(codec, b"".join(msgs), (tw.UNKNOWN_TAG, off))


def test_two_errors_the_earlier_wins(codec):
    msgs = list(good())
    msgs[1200] = _w(b"\x01\x00\x0c\x02\xc3\x28")   # bad UTF-8 in the value
    msgs[3100] = tw.mg().enc_msg(9, b"")            # unknown variant
    off = sum(len(m) for m in msgs[:1200])
    check_error(codec, b"".join(msgs), (tw.INVALID, off))
    msgs[1200], msgs[3100] = b"\x00", msgs[1200]    # a broken length prefix first
    check_error(codec, b"".join(msgs), (tw.SHORT, off))


# ---- capacity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["rows", "children", "ctl"])
def test_capacity_one_short(codec, short):
    import torch
    from netidx_amd import CodecError
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    rng = random.Random(23)
    msgs = [("w", i, True, (19, [(9, i), (6, -i)]) if i % 3 == 0 else (9, i), i)
            for i in range(2000)]
    for _ in range(200):
        msgs.insert(rng.randrange(len(msgs)), ("unsub", 4))
    wire, e = tw.batch(msgs)
    caps = {"rows": len(e.rows), "children": len(e.children), "ctl": len(e.ctl)}
    caps[short] -= 1
    # one spare element behind each capacity holds a sentinel
    cols = Columns(caps["rows"] + 1, caps["children"] + 1, caps["ctl"] + 1, LAYOUT_MIXED, "cuda")
    wcols = WriteCols(caps["rows"] + 1, "cuda")
    cols.s.cap_rows, cols.s.cap_children, cols.s.cap_ctl = caps["rows"], caps["children"], caps["ctl"]
    wcols.s.cap_rows = caps["rows"]
    tensors = [(cols.t[name], caps[kind]) for (name, _, kind) in Columns.FIELDS]
    tensors += [(wcols.wflags, caps["rows"]), (wcols.wid, caps["rows"])]
    for t, _ in tensors:
        t.fill_(0x5A)
    torch.cuda.synchronize()
    with pytest.raises(CodecError, match="NXG_CAPACITY"):
        codec.decode_writes(dev(wire), cols, wcols)
    for t, cap in tensors:
        assert int(t[cap]) == 0x5A
    # with exactly enough room it decodes
    cols.s.cap_rows, cols.s.cap_children, cols.s.cap_ctl = len(e.rows), len(e.children), len(e.ctl)
    wcols.s.cap_rows = len(e.rows)
    codec.decode_writes(dev(wire), cols, wcols)
    assert_expected(codec, cols, wcols, codec.writes_status, e)


# ---- encode = twin bytes --------------------------------------------------------------------------
# an encoder tile is 1024 rows
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 5000])
def test_encode_random_writes(codec, n):
    wire, e = tw.batch(rand_writes(n, 3000 + n))
    cols, wc, heap = encode_from(codec, e, wire)
    assert codec.encoded_writes_len(cols, wc, heap) == len(wire)
    assert codec.encode_writes(cols, wc, heap).cpu().numpy().tobytes() == wire


def test_encode_long_strings_overflow_the_staging(codec):
    rng = random.Random(31)
    msgs = []
    for i in range(3000):
        if i % 700 == 5:
            msgs.append(("w", i, True, (13, bytes(rng.getrandbits(8) for _ in range(40000))), i))
        elif i % 3 == 0:
            msgs.append(("w", i, False, (12, b"x" * rng.randrange(0, 60)), rand_wid(rng)))
        else:
            msgs.append(("w", i, True, (9, rng.getrandbits(64)), rand_wid(rng)))
    wire, e = tw.batch(msgs)
    cols, wc, heap = encode_from(codec, e, wire)
    assert codec.encode_writes(cols, wc, heap).cpu().numpy().tobytes() == wire


def test_encode_with_control_spans(codec):
    """Control spans (pre-encoded Subscribe / Unsubscribe messages): the direct-write path."""
    rng = random.Random(32)
    msgs = rand_writes(2600, 33)
    for i in range(400):
        m = ("unsub", rand_id(rng)) if i % 2 else ("sub", dict(path="/c/%d" % i, token=b"k" * (i % 40)))
        msgs.insert(rng.randrange(len(msgs) + 1), m)
    msgs.append(("unsub", 1))  # after the last row
    wire, e = tw.batch(msgs)
    cols, wc, heap = encode_from(codec, e, wire)
    assert codec.encoded_writes_len(cols, wc, heap) == len(wire)
    assert codec.encode_writes(cols, wc, heap).cpu().numpy().tobytes() == wire


def test_encode_ignores_no_wid_and_other_flag_bits(codec):
    wire, e = tw.batch([("w", 3, True, (9, 1), 0), ("w", 4, False, (16, None), 0)])
    e.wflags = [1 | 2, 2]
    cols, wc, heap = encode_from(codec, e, wire)
    assert codec.encode_writes(cols, wc, heap).cpu().numpy().tobytes() == wire


def test_encode_buffer_one_byte_short_and_empty_batch(codec):
    import torch
    from netidx_amd import CodecError
    wire, e = tw.batch(rand_writes(1500, 34))
    cols, wc, heap = encode_from(codec, e, wire)
    out = torch.zeros(len(wire) + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(CodecError, match="too small"):
        codec.encode_writes_into(cols, wc, heap, out.data_ptr(), len(wire) - 1)
    assert codec.encode_writes_into(cols, wc, heap, out.data_ptr(), len(wire)) == len(wire)
    assert out[: len(wire)].cpu().numpy().tobytes() == wire
    cols0, wc0, _ = encode_from(codec, tw.Expect(), b"")
    assert codec.encoded_writes_len(cols0, wc0) == 0
    assert codec.encode_writes(cols0, wc0).numel() == 0


def test_encode_from_host_columns(codec):
    """in / win / heap / out all host memory."""
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    wire, e = tw.batch(rand_writes(1200, 35))
    dcols, dwc, _ = encode_from(codec, e, wire)
    n, nc = len(e.rows), len(e.children)
    cols = Columns(n, nc, 1, LAYOUT_MIXED, "cpu")
    wc = WriteCols(n, "cpu")
    for name, _, _ in Columns.FIELDS:
        cols.t[name].copy_(dcols.t[name].cpu())
    cols.s.n_rows, cols.s.n_children, cols.s.n_ctl = n, nc, 0
    wc.wflags[:n].copy_(dwc.wflags[:n].cpu())
    wc.wid[:n].copy_(dwc.wid[:n].cpu())
    heap = np.frombuffer(wire, np.uint8).copy()
    out = np.zeros(len(wire), np.uint8)
    assert codec.encode_writes_into(cols, wc, heap, out.ctypes.data, len(out)) == len(wire)
    assert out.tobytes() == wire


# ---- round trip -----------------------------------------------------------------------------------
def test_round_trip_canonical_frames(codec):
    msgs = rand_writes(4000, 36)
    rng = random.Random(37)
    for i in range(300):
        msgs.insert(rng.randrange(len(msgs) + 1), ("unsub", rand_id(rng)))
        msgs.insert(rng.randrange(len(msgs) + 1), ("sub", dict(path="/r/%d" % i, token=b"z")))
    for wire in (tw.batch(msgs)[0], tw.batch(rand_writes(2000, 38))[0]):
        frame = dev(wire)
        cols, wcols = codec.decode_writes(frame)
        assert codec.encode_writes(cols, wcols, frame).cpu().numpy().tobytes() == wire


# ---- unchanged ground -----------------------------------------------------------------------------
def test_from_and_to_frames_alternate_on_one_context(codec):
    """A From frame through decode_batch and a To frame through decode_writes, alternately,
    twice, on one context: they share the scratch buffers and the status ring."""
    import netidx_amd
    import nxo
    mg = tw.mg()
    rng = random.Random(39)
    upd = [("u", rand_id(rng), mg.rand_value(rng)) if i % 11 else ("hb",) for i in range(3000)]
    fwire, _ = mg.batch(upd)
    twire, e = tw.batch(rand_writes(3000, 40))
    o = nxo.decode(fwire).trim()
    for _ in range(2):
        cols, st = codec.decode_batch(dev(fwire), flags=netidx_amd.HINT_MIXED)
        g = cols.numpy()
        assert st.err_kind == 0 and st.n_heartbeat == o["n_heartbeat"] and st.path in (2, 4)
        for k in ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off",
                  "ctl_len", "ctl_variant"):
            assert np.array_equal(g[k], o[k]), k
        check(codec, twire, e)
