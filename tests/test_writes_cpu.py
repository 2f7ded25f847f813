"""CPU-only checks of the write-batch (publisher::To) ground: the Python twin against the
hand-derived known answers and against the host parser, the new C ABI symbols, and the argument
checks of the new calls (which come before any use of the context, so no GPU is needed)."""
import ctypes as C
import random
import struct

import pytest

import netidx_amd
from netidx_amd import codec
import to_twin as tw

F64_1 = struct.unpack(">Q", struct.pack(">d", 1.0))[0]

KNOWN = [
    ("write_null", lambda: tw.write(0, False, (16, None), 0), "06 02 00 00 10 00"),
    ("write_f64", lambda: tw.write(300, True, (9, F64_1), 5),
     "0f 02 ac 02 01 09 3f f0 00 00 00 00 00 00 05"),
    ("write_old_peer", lambda: tw.write(1, False, (14, None)), "05 02 01 00 0e"),
    ("unsubscribe", lambda: tw.unsubscribe(7), "03 01 07"),
    ("subscribe", lambda: tw.subscribe("/a", ("v4", 0, 0), 1, 2, b"t"),
     "1a 00 02 2f 61 00 00 00 00 00 00 00 00 00 00 00 00 00 00 01 00 00 00 02 01 74"),
]


@pytest.mark.parametrize("name,make,hexes", KNOWN, ids=[k[0] for k in KNOWN])
def test_twin_known_answers(name, make, hexes):
    assert make().hex() == hexes.replace(" ", "")


def test_twin_decodes_what_it_encodes():
    """batch()'s expected columns (from the messages) equal decode()'s (from the wire)."""
    mg = tw.mg()
    rng = random.Random(7)
    msgs = []
    for i in range(600):
        k = rng.random()
        if k < 0.1:
            msgs.append(("unsub", rng.getrandbits(30)))
        elif k < 0.15:
            msgs.append(("sub", dict(path="/p/%d" % i, resolver=("v6", list(range(8)), 9, 1, 2),
                                     timestamp=i, permissions=3, token=b"tok")))
        else:
            msgs.append(("w", rng.getrandbits(rng.choice([7, 20, 40])), rng.random() < 0.5,
                         mg.rand_value(rng), rng.choice([None, 0, 5, 2**40, 2**64 - 1])))
    wire, e = tw.batch(msgs)
    d, err = tw.decode(wire)
    assert err is None
    for k in ("rows", "children", "ctl", "wflags", "wid"):
        assert getattr(d, k) == getattr(e, k), k


def test_twin_first_error_rules():
    good = tw.write(1, False, (16, None), 0)
    bad_bool = tw.mg().enc_msg(2, b"\x01\x02\x10\x00")
    assert tw.first_error(good + bad_bool) == (tw.UNKNOWN_TAG, len(good))
    assert tw.first_error(good + tw.mg().enc_msg(3, b"")) == (tw.UNKNOWN_TAG, len(good))
    assert tw.first_error(good + b"\x00") == (tw.SHORT, len(good))
    # a WriteId cut mid-varint by the length prefix is "absent", not an error
    cut = tw.mg().enc_msg(2, b"\x01\x00\x10\x80")
    d, err = tw.decode(cut)
    assert err is None and d.wflags == [tw.WRITE_NO_WID] and d.wid == [0]
    # an over-long WriteId varint is InvalidFormat
    assert tw.first_error(tw.mg().enc_msg(2, b"\x01\x00\x10" + b"\xff" * 10 + b"\x01")) == \
        (tw.INVALID, 0)


def test_host_parser_agrees_with_twin():
    """nxg_msg_parse(to=1), the host parser already in the tree, on variant, id and value tag."""
    cases = [(tw.write(0, False, (16, None), 0), 2, 0, 16),
             (tw.write(300, True, (9, F64_1), 5), 2, 300, 9),
             (tw.write(1, False, (14, None)), 2, 1, 14),
             (tw.write(2**35 + 3, True, (6, -5), 2**63), 2, 2**35 + 3, 6),
             (tw.unsubscribe(7), 1, 7, None),
             (tw.subscribe("/a", ("v4", 0, 0), 1, 2, b"t"), 0, None, None)]
    for m, variant, id_, tag in cases:
        p = netidx_amd.msg_parse(m, to=True)
        d, err = tw.decode(m)
        assert err is None
        assert p.variant == variant and p.msg_len == len(m)
        if variant == 2:
            assert (p.id, p.value_tag) == (id_, tag) == (d.rows[0][0], d.rows[0][1])
        elif variant == 1:
            assert p.id == id_ and d.ctl == [(0, 0, len(m), 1)]
        else:
            assert d.ctl == [(0, 0, len(m), 0)]


def test_new_symbols_and_constants():
    L = netidx_amd.lib()
    for f in ("nxg_write_cols_alloc", "nxg_write_cols_free", "nxg_decode_writes",
              "nxg_encoded_writes_len", "nxg_encode_writes"):
        assert hasattr(L, f) and f in codec.SIGNATURES
    assert (netidx_amd.WRITE_REPLY, netidx_amd.WRITE_NO_WID, netidx_amd.PATH_WRITES) == (1, 2, 6)
    assert C.sizeof(codec.NxgWriteCols) == 32
    for m in ("decode_writes", "encoded_writes_len", "encode_writes"):
        assert hasattr(netidx_amd.Codec, m)


def _cols(layout, cap_rows):
    """An NxgColumns that only the argument checks look at (its arrays are never touched)."""
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    c = codec.NxgColumns()
    c.layout, c.mem, c.cap_rows, c.cap_children, c.cap_ctl = layout, codec.MEM_HOST, cap_rows, 1, 1
    c.id = c.fixed = p
    if layout == codec.LAYOUT_MIXED:
        for f in ("tag", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off", "ctl_len",
                  "ctl_variant"):
            setattr(c, f, p)
    return c, buf


def _wcols(cap_rows, mem=codec.MEM_HOST):
    buf = C.create_string_buffer(64)
    w = codec.NxgWriteCols()
    w.mem, w.cap_rows = mem, cap_rows
    w.wflags = w.wid = C.addressof(buf)
    return w, buf


def _fails(call, needle):
    err = codec.NetidxError()
    assert call(err) is False
    msg = err.msg.decode()
    netidx_amd.lib().nxg_error_free(C.byref(err))
    assert needle in msg, msg


def test_misuse_is_refused_with_a_message():
    L = netidx_amd.lib()
    ctx = C.create_string_buffer(8)  # never used: the argument checks come first
    st = codec.NxgStatus()
    frame = C.create_string_buffer(b"\x03\x01\x07")
    mixed, k1 = _cols(codec.LAYOUT_MIXED, 4)
    f64, k2 = _cols(codec.LAYOUT_F64, 4)
    w4, k3 = _wcols(4)
    w3, k4 = _wcols(3)
    wdev, k5 = _wcols(4, codec.MEM_DEVICE)
    dec = L.nxg_decode_writes
    # null arguments
    _fails(lambda e: dec(None, frame, 3, C.byref(mixed), C.byref(w4), C.byref(st), C.byref(e)),
           "null")
    _fails(lambda e: dec(ctx, frame, 3, None, C.byref(w4), C.byref(st), C.byref(e)), "null")
    _fails(lambda e: dec(ctx, frame, 3, C.byref(mixed), None, C.byref(st), C.byref(e)), "null")
    _fails(lambda e: dec(ctx, None, 3, C.byref(mixed), C.byref(w4), C.byref(st), C.byref(e)),
           "null")
    # F64-layout columns
    _fails(lambda e: dec(ctx, frame, 3, C.byref(f64), C.byref(w4), C.byref(st), C.byref(e)),
           "MIXED")
    # write columns smaller than the columns
    _fails(lambda e: dec(ctx, frame, 3, C.byref(mixed), C.byref(w3), C.byref(st), C.byref(e)),
           "write columns hold 3 rows")
    # mismatched memory kinds
    _fails(lambda e: dec(ctx, frame, 3, C.byref(mixed), C.byref(wdev), C.byref(st), C.byref(e)),
           "both")
    # the encode side
    n = C.c_uint64(0)
    _fails(lambda e: L.nxg_encode_writes(None, C.byref(mixed), C.byref(w4), None, None, 0,
                                         C.byref(n), C.byref(e)), "null")
    _fails(lambda e: L.nxg_encoded_writes_len(ctx, C.byref(mixed), None, None, C.byref(n),
                                              C.byref(e)), "null")
    _fails(lambda e: L.nxg_encoded_writes_len(ctx, C.byref(f64), C.byref(w4), None, C.byref(n),
                                              C.byref(e)), "MIXED")
    mixed.n_rows = 4
    _fails(lambda e: L.nxg_encoded_writes_len(ctx, C.byref(mixed), C.byref(w3), None, C.byref(n),
                                              C.byref(e)), "write columns hold 3 rows")
