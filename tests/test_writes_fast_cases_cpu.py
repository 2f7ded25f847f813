"""The case table of the fast To decoder against the twin, and the ABI of nxg_decode_writes_opts
(no GPU): tests/writes_fast_cases.py is what tests/test_gpu_writes_fast.py runs on the device, so
its classes must mean what they say."""
import ctypes as C

import pytest

import netidx_amd
from netidx_amd import codec

import to_twin as tw
import writes_fast_cases as wf


def test_every_must_case_is_in_the_must_take_set_and_decodes_cleanly():
    must = wf.by_class("must")
    assert len(must) > 200
    for k in must:
        assert wf.fast_must_take(k.wire), k
        d, err = tw.decode(k.wire)
        assert err is None and not d.children, k


def test_every_decline_case_is_outside_the_must_take_set():
    for k in wf.by_class("decline"):
        assert not wf.fast_must_take(k.wire), k


def test_every_error_case_records_the_twins_error():
    errors = [k for k in wf.by_class("decline") if k.err is not None]
    valid = [k for k in wf.by_class("decline") if k.err is None]
    assert len(errors) >= 3 * 9 and len(valid) >= 3 * 6
    for k in errors:
        assert tw.first_error(k.wire) == k.err and k.err[0] in (1, 2, 3, 4), k
    for k in valid:
        assert tw.first_error(k.wire) is None, k
    # the same bad message first, in the middle and last: three different offsets, the first 0
    for name in wf._bad_messages():
        offs = [k.err[1] for k in errors if k.name.startswith(name + "_")]
        assert len(offs) == 3 and offs[0] == 0 and offs[0] < offs[1] < offs[2], (name, offs)
    # "may" cases are valid frames too
    for k in wf.by_class("may"):
        assert tw.first_error(k.wire) is None, k


def test_the_predicate_on_crafted_messages():
    m = tw.mg()
    ok = [wf.U(7), wf.S(), wf.W(1, True, (9, 1), 5), wf.W(2**35 - 1, False, (16, None), None),
          wf.sub_of_len(256)]
    for w in ok:
        assert wf.fast_must_take(w), w
    no = [b"", wf.W(2**35, True, (9, 1), 5), wf.sub_of_len(257),
          wf.W(1, True, (19, []), 5), wf.W(1, True, (27, bytes(20)), 5),
          tw.write(1, True, (9, 1), 5, id_bytes=b"\x81\x00"),   # a non-canonical id
          m.enc_msg(2, b"\x01\x00\x10\x80"),                    # a wid cut short
          tw.unsubscribe(7, trailing=b"\x00"), wf.U(7)[:-1], m.enc_msg(3, b"\x01")]
    for w in no:
        assert not wf.fast_must_take(w), w


def test_the_table_covers_the_geometry_it_claims():
    names = {k.name: k for k in wf.cases()}
    for off in range(-70, 3):
        for kind in ("sub", "write"):
            k = names[f"{kind}_at_edge{off:+d}"]
            # the shifted message starts at the stated offset from the tile edge
            pos, starts = 0, []
            while pos < len(k.wire):
                starts.append(pos)
                pos += tw._varint(k.wire, pos, len(k.wire))[0]
            assert wf.TILE + off in starts, k
    for nt in (1, 4, 5, 9, 256, 257):
        assert len(names[f"exactly_{nt}_tiles"].wire) == nt * wf.TILE
    assert len(names["tile_of_1366_unsubscribes"].wire) == 3 * 1366
    assert len(names["last_tile_of_1_byte"].wire) == wf.TILE + 1


def test_abi_is_exported():
    L = netidx_amd.lib()
    assert hasattr(L, "nxg_decode_writes_opts") and "nxg_decode_writes_opts" in codec.SIGNATURES
    assert netidx_amd.PATH_WRITES_FAST == 8 and netidx_amd.PATH_WRITES == 6
    assert C.sizeof(codec.NxgWriteDecodeOpts) == 8
    assert "fast" in codec.Codec.decode_writes.__code__.co_varnames


def _args():
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    cols = codec.NxgColumns()
    cols.layout, cols.mem, cols.cap_rows, cols.cap_children, cols.cap_ctl = (
        codec.LAYOUT_MIXED, codec.MEM_DEVICE, 8, 8, 8)
    for name in ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off",
                 "ctl_len", "ctl_variant"):
        setattr(cols, name, p)
    w = codec.NxgWriteCols(codec.MEM_DEVICE, 0, 8, p, p)
    return buf, cols, w


@pytest.mark.parametrize("fast,reserved", [(2, 0), (0, 1), (1, 1), (0xFFFFFFFF, 0)])
def test_bad_options_are_refused_before_any_use_of_the_context(fast, reserved):
    L = netidx_amd.lib()
    ctx = C.create_string_buffer(8)  # never used: the argument checks come first
    frame = C.create_string_buffer(16)
    keep, cols, w = _args()
    st, err = codec.NxgStatus(), codec.NetidxError()
    opts = codec.NxgWriteDecodeOpts(fast, reserved)
    ok = L.nxg_decode_writes_opts(C.addressof(ctx), C.addressof(frame), 3, C.byref(cols),
                                  C.byref(w), C.byref(opts), C.byref(st), C.byref(err))
    assert not ok
    assert b"NxgWriteDecodeOpts" in bytes(err.msg)


def test_a_null_argument_is_refused():
    L = netidx_amd.lib()
    ctx = C.create_string_buffer(8)
    frame = C.create_string_buffer(16)
    keep, cols, w = _args()
    opts = codec.NxgWriteDecodeOpts(1, 0)
    full = [C.addressof(ctx), C.addressof(frame), 3, C.byref(cols), C.byref(w), C.byref(opts),
            C.byref(codec.NxgStatus())]
    for k in (0, 1, 3, 4, 6):
        st, err = codec.NxgStatus(), codec.NetidxError()
        a = list(full)
        a[k] = None
        assert not L.nxg_decode_writes_opts(*a, C.byref(err)), k
        assert b"null argument" in bytes(err.msg), k
