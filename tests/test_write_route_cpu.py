"""CPU-only checks of write routing: the Python model (tests/write_route_model.py) against known
answers written out by hand, the exported symbol, and the argument checks of nxg_route_writes
(which come before any use of the context, so no GPU is needed)."""
import ctypes as C

import netidx_amd
from netidx_amd import codec
import write_route_model as wm

M1 = b"cannot write to unsubscribed value"
M2 = b"write permission denied"
M3 = b"writes not accepted"


def test_known_answers():
    assert wm.unsubscribed(3).hex() == "030203"
    assert wm.write_result(3, M3, 7).hex() == (
        "19 06 03 12 13 77 72 69 74 65 73 20 6e 6f 74 20 61 63 63 65 70 74 65 64 07"
    ).replace(" ", "")
    assert wm.write_result(300, M2, 128).hex() == (
        "1f 06 ac 02 12 17 77 72 69 74 65 20 70 65 72 6d 69 73 73 69 6f 6e 20 64 65 6e 69 65 64 "
        "80 01").replace(" ", "")
    # the fourth message by the same rule: body = 06 03 12 22 + 34 bytes + 07 = 39, L = 40
    assert wm.write_result(3, M1, 7).hex() == (
        "28 06 03 12 22 63 61 6e 6e 6f 74 20 77 72 69 74 65 20 74 6f 20 75 6e 73 75 62 73 63 72 "
        "69 62 65 64 20 76 61 6c 75 65 07").replace(" ", "")
    assert (len(M1), len(M2), len(M3)) == (34, 23, 19)
    # the longest reply: 10-byte Id and WriteId; its body is 57 bytes, L = 58 in one byte
    big = wm.write_result(2**64 - 1, M1, 2**64 - 1)
    assert len(big) == 58 and big[0] == 58


def test_hand_built_batch():
    """Write, Unsubscribe, Write to the same id, Write to another id."""
    st = wm.State({5: 0x05, 6: 0x01}, {5: [2, 0]})
    msgs = [("w", 5, True, 9), ("unsub", 5), ("w", 5, True, 10), ("w", 6, True, None)]
    r = wm.handle_batch(st, msgs, fresh_wid=100)
    assert r.outcome == [0, 1, 2]
    assert bytes(r.reply) == (
        bytes.fromhex("030205")
        + bytes.fromhex("2806051222") + M1 + b"\x0a"
        + bytes.fromhex("1d06061217") + M2 + b"\x64")
    assert r.n_replies == 3
    assert r.wait == [(0, 5, 9)]
    assert r.unsub == [5]
    assert r.batches == {2: [(5, 0)], 0: [(5, 0)]}
    assert r.n_fresh == 1
    assert st.subscribed == {6: 0x01}


def test_model_rules():
    st = wm.State({1: 0x04, 2: 0x04, 3: 0x03}, {1: [0], 2: []})
    r = wm.handle_batch(st, [("w", 1, False, 1), ("w", 2, True, 2), ("w", 3, False, 3),
                             ("w", 4, True, 4), ("w", 9, False, 5), ("unsub", 77)], 0)
    assert r.outcome == [0, 3, 2, 1, 1]
    # without r nothing is queued; Unsubscribe of an unknown id still replies
    assert bytes(r.reply) == wm.write_result(2, M3, 2) + wm.write_result(4, M1, 4) + \
        wm.unsubscribed(77)
    assert r.wait == [] and r.unsub == [77]
    # a client the publisher does not know
    r = wm.handle_batch(wm.State(None, {1: [0]}), [("w", 1, True, 8), ("unsub", 1)], 0)
    assert r.outcome == [1] and bytes(r.reply) == wm.write_result(1, M1, 8) + wm.unsubscribed(1)


def test_symbol_and_structs():
    L = netidx_amd.lib()
    assert hasattr(L, "nxg_route_writes") and "nxg_route_writes" in codec.SIGNATURES
    assert C.sizeof(codec.NxgWriteTable) == 56
    assert C.sizeof(codec.NxgWriteRoute) == 16 + 56 + 64 + 12 * 8 + 8
    assert hasattr(netidx_amd.Codec, "route_writes")
    assert (netidx_amd.WRITE_ROUTED, netidx_amd.WRITE_UNSUBSCRIBED, netidx_amd.WRITE_DENIED,
            netidx_amd.WRITE_NOT_ACCEPTED) == (0, 1, 2, 3)
    assert netidx_amd.NOT_SUBSCRIBED == 0xFFFFFFFF


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
    ctx = C.create_string_buffer(8)  # never used: the argument checks come first
    frame = C.create_string_buffer(16)
    keep = C.create_string_buffer(64)
    p = C.addressof(keep)
    tab = codec.NxgWriteTable()
    w = codec.NxgWriteCols()
    w.mem, w.cap_rows, w.wflags, w.wid = codec.MEM_DEVICE, 8, p, p
    out = codec.NxgWriteRoute()
    out.cap_rows, out.outcome = 8, p
    out.disp.chan_off = p
    good, k1 = _cols()

    def fails(needle, ctx=ctx, tab=tab, cols=good, wcols=w, row_begin=0, ctl_begin=0, out=out):
        err = codec.NetidxError()
        ok = L.nxg_route_writes(ctx, C.byref(tab) if tab is not None else None, frame,
                                C.byref(cols) if cols is not None else None,
                                C.byref(wcols) if wcols is not None else None, row_begin,
                                ctl_begin, 0, C.byref(out) if out is not None else None,
                                C.byref(err))
        msg = err.msg.decode() if err.msg else ""
        L.nxg_error_free(C.byref(err))
        assert ok is False and needle in msg, (needle, msg)

    fails("null", ctx=None)
    fails("null", tab=None)
    fails("null", cols=None)
    fails("null", out=None)
    fails("wcols", wcols=None)
    host, k2 = _cols(mem=codec.MEM_HOST)
    fails("cols->mem", cols=host)
    f64, k3 = _cols(layout=codec.LAYOUT_F64)
    fails("cols->layout", cols=f64)
    fails("row_begin 5", row_begin=5)
    fails("ctl_begin 3", ctl_begin=3)
    small = codec.NxgWriteRoute()
    small.cap_rows, small.outcome = 3, p
    small.disp.chan_off = p
    fails("out->cap_rows", out=small)
    w3 = codec.NxgWriteCols()
    w3.mem, w3.cap_rows, w3.wflags, w3.wid = codec.MEM_DEVICE, 3, p, p
    fails("wcols holds 3 rows", wcols=w3)
