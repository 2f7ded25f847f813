"""CPU-only checks of Subscribe routing: the Python model (tests/subscribe_route_model.py) against
answers written out by hand and against the library's host encoder, nxg_path_is_plain against the
model's rule, the exported symbols, and the argument checks of nxg_route_subscribes that come
before any use of the context (so no GPU is needed)."""
import ctypes as C
import struct

import netidx_amd
from netidx_amd import codec
import subscribe_route_model as sm
import to_twin as tw
import write_route_model as wm

F64_1 = (9, struct.unpack(">Q", struct.pack(">d", 1.0))[0])


def test_known_answers():
    assert sm.subscribed(b"/a", 5, F64_1).hex() == (
        "0f 03 02 2f 61 05 09 3f f0 00 00 00 00 00 00").replace(" ", "")
    assert sm.no_such_value(b"/a").hex() == "0500022f61"
    assert sm.denied(b"/a").hex() == "0501022f61"


def test_length_prefix_width_changes_at_a_125_byte_path():
    # body = variant + varint(|p|) + p = |p| + 2 (|p| < 128); L = lw(body)
    p124, p125 = b"/" + b"x" * 123, b"/" + b"x" * 124
    m = sm.no_such_value(p124)
    assert m[0] == 127 and len(m) == 1 + 126 and m[1:3] == bytes([0, 124])
    m = sm.no_such_value(p125)
    assert m[:2] == bytes([0x81, 0x01]) and len(m) == 2 + 127 and m[2:4] == bytes([0, 125])
    # a 128-byte path: varint(|p|) takes two bytes; body = 1 + 2 + 128 = 131, L = 133 = 85 01
    p128 = b"/" + b"y" * 127
    m = sm.denied(p128)
    assert m[:2] == bytes([0x85, 0x01]) and m[2:5] == bytes([1, 0x80, 0x01]) and m[5:] == p128


def test_subscribed_matches_the_host_encoder_for_scalars():
    cases = [(b"/a", 5, (9, F64_1[1]), (9, F64_1[1], 0, b"")),
             (b"/some/longer/path", 2**35, (4, 2**63 + 9), (4, 2**63 + 9, 0, b"")),
             (b"/t", 127, (12, b"text"), (12, 0, 4, b"text")),
             (b"/e", 128, (12, b""), (12, 0, 0, b"")),
             (b"/n", 0, (16, None), (16, 0, 0, b"")),
             (b"/v", 300, (1, 300), (1, 300, 0, b"")),
             (b"/z", 1, (7, -5), (7, (-5) & tw.M64, 0, b""))]
    for path, id, value, (tag, fixed, aux, text) in cases:
        assert sm.subscribed(path, id, value) == codec.msg_subscribed(path, id, tag, fixed, aux, text)


def run(st, paths, perm=None):
    res, n = sm.route(st, paths, perm)
    return res, n


def test_every_outcome_and_its_reply():
    st = sm.State({b"/a": 1, b"/b": 2, b"/gone": 9}, {1: F64_1, 2: (12, b"x")},
                  default=[b"/dflt"], denied_ids={2})
    paths = [b"/a", b"/b", b"/gone", b"/dflt/x", b"/nope", b"/a"]
    res, n = run(st, paths)
    assert n == 6 and res.outcome == [0, 2, 4, 3, 1, 0]
    assert res.span_id == [1, 2, 9, None, None, 1]
    assert res.sub == [(1, sm.ALL), (1, sm.ALL)] and res.deferred == [3]
    assert bytes(res.reply) == sm.subscribed(b"/a", 1, F64_1) + sm.denied(b"/b") + \
        sm.no_such_value(b"/nope") + sm.subscribed(b"/a", 1, F64_1)
    assert res.n_replies == 4 and st.subscribed == {1: sm.ALL} and st.deferred_len == 1


def test_token_results():
    st = sm.State({b"/a": 1}, {1: F64_1})
    res, n = run(st, [b"/a", b"/a", b"/zz"], [0x03, sm.DENY, sm.DENY])
    assert res.outcome == [0, 2, 2] and res.sub == [(1, 0x03)] and res.span_id == [1, None, None]
    assert bytes(res.reply) == sm.subscribed(b"/a", 1, F64_1) + sm.denied(b"/a") + sm.denied(b"/zz")


def test_only_the_greatest_base_is_examined():
    # bases /a and /a/b: /a/c finds /a/b, which is no prefix -> NoSuchValue although /a is one
    st = sm.State({}, {}, default=[b"/a", b"/a/b"])
    res, _ = run(st, [b"/a/c", b"/a/b/c", b"/a/b", b"/a", b"/0"])
    assert res.outcome == [1, 3, 3, 3, 1]
    # base /d: /dx is deferred, starts_with is a string prefix
    st = sm.State({}, {}, default=[b"/d"])
    res, _ = run(st, [b"/dx", b"/d", b"/c", b"/e"])
    assert res.outcome == [3, 3, 1, 1]


def test_deferred_room():
    st = sm.State({}, {}, default=[b"/d"], deferred_len=sm.MAX_DEFERRED)       # room 0
    res, _ = run(st, [b"/d/1", b"/d/2"])
    assert res.outcome == [1, 1] and res.deferred == []
    st = sm.State({}, {}, default=[b"/d"], deferred_len=sm.MAX_DEFERRED - 1)   # room 1
    res, _ = run(st, [b"/x", b"/d/1", b"/d/2", b"/d/3"])
    assert res.outcome == [1, 3, 1, 1] and res.deferred == [1]
    assert bytes(res.reply) == sm.no_such_value(b"/x") + sm.no_such_value(b"/d/2") + \
        sm.no_such_value(b"/d/3")


def test_a_path_that_is_not_plain_stops_the_run():
    st = sm.State({b"/a": 1}, {1: F64_1})
    res, n = run(st, [b"/a", b"/a//b", b"/a"])
    assert n == 1 and res.outcome == [0]


PLAIN_CASES = [(b"", False), (b"/", True), (b"//", False), (b"/a/", False), (b"a/b", True),
               (b"/a//b", False), (b"/a\\/b", False), ("/ä/€\U0001f600".encode(), True),
               (b"/a", True), (b"a", True), (b"\\", False), (b"/abcdefg/", False),
               (b"/abcdefg//h", False), (b"/abcdef//", False), (b"/abcdefgh/i", True),
               (b"/abcdefg/h/", False), (b"a/", False)]


def test_path_is_plain():
    for p, want in PLAIN_CASES:
        assert sm.is_plain(p) is want, p
        assert netidx_amd.path_is_plain(p) is want, p
    # every two-slash placement around the 8-byte words the device reads
    for n in range(1, 20):
        for i in range(n):
            for c in (b"/", b"\\"):
                p = bytearray(b"/" + b"x" * n)
                p[1 + i:2 + i] = c
                assert netidx_amd.path_is_plain(bytes(p)) is sm.is_plain(bytes(p)), bytes(p)


def test_mixed_frame_through_the_write_model():
    sst = sm.State({b"/p": 3}, {3: F64_1})
    res = sm.Result()
    st = wm.State({}, {3: [0]})
    msgs = [("sub", b"/p", 0, None), ("w", 3, True, 1), ("unsub", 3), ("w", 3, True, 2),
            ("sub", b"/p", 2, 0x03), ("w", 3, True, 3)]
    w = wm.handle_batch(st, msgs, 0, sm.on_subscribe(sst, res))
    assert w.outcome == [wm.ROUTED, wm.UNSUBSCRIBED, wm.DENIED]
    assert res.outcome == [0, 0] and res.sub == [(3, sm.ALL), (3, 0x03)]


def test_symbols_and_structs():
    L = netidx_amd.lib()
    for f in ("nxg_path_table_new", "nxg_path_table_free", "nxg_path_table_len",
              "nxg_path_table_insert", "nxg_path_table_remove", "nxg_path_table_lookup",
              "nxg_path_is_plain", "nxg_route_subscribes"):
        assert hasattr(L, f) and f in codec.SIGNATURES, f
    assert C.sizeof(codec.NxgSubscribeTable) == 56
    assert C.sizeof(codec.NxgSubscribeRoute) == 10 * 8 + 5 * 8 + 5 * 8 + 8 + 8
    assert (netidx_amd.SUB_SUBSCRIBED, netidx_amd.SUB_NO_SUCH_VALUE, netidx_amd.SUB_DENIED,
            netidx_amd.SUB_DEFERRED, netidx_amd.SUB_IGNORED) == (0, 1, 2, 3, 4)
    assert netidx_amd.NO_ID == 2**64 - 1 and netidx_amd.SUB_PERM_DENY == 0xFFFFFFFF
    assert netidx_amd.PERM_ALL == 0x3F and netidx_amd.MAX_DEFERRED == 1000000
    for m in ("route_subscribes",):
        assert hasattr(netidx_amd.Codec, m)
    assert L.nxg_path_table_len(None) == 0


def _cols(layout=codec.LAYOUT_MIXED, mem=codec.MEM_DEVICE, n_rows=4, n_ctl=2):
    """An NxgColumns that only the argument checks look at (its arrays are never touched)."""
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    c = codec.NxgColumns()
    c.layout, c.mem, c.cap_rows, c.cap_children, c.cap_ctl = layout, mem, 8, 1, 8
    c.n_rows, c.n_ctl = n_rows, n_ctl
    c.id = c.fixed = p
    if layout == codec.LAYOUT_MIXED:
        for f in ("tag", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off", "ctl_len",
                  "ctl_variant"):
            setattr(c, f, p)
    return c, buf


def test_misuse_is_refused_with_a_message():
    L = netidx_amd.lib()
    ctx = C.create_string_buffer(8)  # never used: these argument checks come first
    frame = C.create_string_buffer(16)
    keep = C.create_string_buffer(64)
    p = C.addressof(keep)
    pub = codec.NxgPubTable()
    tab = codec.NxgSubscribeTable()
    tab.paths, tab.pub = p, C.addressof(pub)  # (a path table nothing below looks into)
    out = codec.NxgSubscribeRoute()
    out.cap_spans, out.outcome, out.span_id = 8, p, p
    good, k1 = _cols()

    def fails(needle, ctx=ctx, tab=tab, cols=good, row_begin=0, ctl_begin=0, out=out):
        err = codec.NetidxError()
        ok = L.nxg_route_subscribes(ctx, C.byref(tab) if tab is not None else None, frame,
                                    C.byref(cols) if cols is not None else None, row_begin,
                                    ctl_begin, None, C.byref(out) if out is not None else None,
                                    C.byref(err))
        msg = err.msg.decode() if err.msg else ""
        L.nxg_error_free(C.byref(err))
        assert ok is False and needle in msg, (needle, msg)

    fails("null", ctx=None)
    fails("null", cols=None)
    fails("null", out=None)
    fails("tab", tab=None)
    nopaths = codec.NxgSubscribeTable()
    nopaths.pub = C.addressof(pub)
    fails("tab->paths", tab=nopaths)
    nopub = codec.NxgSubscribeTable()
    nopub.paths = p
    fails("tab->pub", tab=nopub)
    host, k2 = _cols(mem=codec.MEM_HOST)
    fails("cols->mem", cols=host)
    f64, k3 = _cols(layout=codec.LAYOUT_F64)
    fails("cols->layout", cols=f64)
    fails("ctl_begin 3", ctl_begin=3)
    fails("row_begin 5", row_begin=5)
    small = codec.NxgSubscribeRoute()
    small.cap_spans, small.outcome, small.span_id = 1, p, p
    fails("out->cap_spans", out=small)
    noarr = codec.NxgSubscribeRoute()
    noarr.cap_spans, noarr.outcome, noarr.span_id, noarr.cap_reply = 8, p, p, 4
    fails("null output array", out=noarr)
