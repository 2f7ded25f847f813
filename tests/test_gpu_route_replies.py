"""GPU tests of nxg_route_replies: the cases and the host loop of tests/reply_route_cases.py and
tests/reply_route_model.py run over the library. Bar: every call's outputs bit-exact with the
contract's statement (contract_call), and the chained result equal to the sequential restatement
of process_batch (connection.rs:409-541), which shares no code with the library."""
import ctypes as C

import numpy as np
import pytest

import reply_route_cases as rc
import reply_route_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def dev(wire):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(wire) or b"\x00", np.uint8).copy()).cuda()


def decode(codec, msgs, quirks=None):
    from netidx_amd.codec import Columns, HINT_MIXED, LAYOUT_MIXED
    w = rc.wire_of(msgs, quirks)
    frame = dev(w)
    cols = Columns(len(w) // 3 + 1, 1, len(w) // 2 + 1, LAYOUT_MIXED, "cuda")
    if w:  # (an all-f64 frame of Updates alone would come back in the F64 layout: not this call's)
        codec.decode_into(frame, len(w), cols, flags=HINT_MIXED)
    assert cols.s.n_rows == sum(1 for m in msgs if m[0] == "upd")
    assert cols.s.n_ctl == len(msgs) - cols.s.n_rows
    return frame, cols


def device_table(codec, tab):
    from netidx_amd.codec import PathTable, ReplyTable, SubTable
    off, chans = [0], []
    for _, cs, _ in tab["slots"]:
        chans += cs
        off.append(len(chans))
    subs = SubTable(tab["slot_of_id"], [s[0] for s in tab["slots"]], off, chans,
                    [s[2] for s in tab["slots"]], tab["n_chans"])
    paths = sorted(tab["pending"], key=tab["pending"].get)
    pt = PathTable(codec, len(paths), sum(len(p) for p in paths))
    if paths:
        assert pt.insert(paths, list(range(len(paths)))) == 0
    return ReplyTable(subs, pt, tab["pend_slot"], tab["pend_alive"])


def as_contract(r, n_chans):
    h = r.numpy()
    b = r.batches()
    return {"outcome": h["outcome"], "span_q": h["span_q"], "span_id": h["span_id"],
            "chan": [b.get(c, []) for c in range(n_chans)], "last_row": h["last_row"],
            "sub": h["sub"], "unsub": h["unsub"], "reply": h["reply"], "n_replies": r.n_replies,
            "n_unmatched": r.n_unmatched, "next_row": r.next_row, "next_ctl": r.next_ctl,
            "stopped": r.stopped}


def library_call(codec, frame, cols):
    """call() for rm.run_chained: one nxg_route_replies, checked against the contract."""
    def call(tab, ids, spans, row_begin, ctl_begin):
        want = rm.contract_call(tab, ids, spans, row_begin, ctl_begin)
        t = device_table(codec, tab)
        r = codec.route_replies(t, frame, cols, row_begin, ctl_begin)
        got = as_contract(r, tab["n_chans"])
        got["last_row"] = got["last_row"][:len(tab["slots"])]
        for f in want:
            assert got[f] == want[f], f
        assert r.n_entries == sum(len(c) for c in want["chan"])
        assert r.n_sub == len(want["sub"]) and r.n_unsub == len(want["unsub"])
        assert r.reply_len == len(want["reply"])
        assert r.n_outcome == [want["outcome"].count(o) for o in range(7)]
        t.pending.close()
        return got
    return call


def run_case(codec, case):
    name, st, msgs, n_ids, n_chans, quirks = case
    frame, cols = decode(codec, msgs, quirks)
    want = rm.process_batch(st.copy(), msgs)
    log = []
    got = rm.run_chained(st.copy(), msgs, library_call(codec, frame, cols), n_ids, n_chans, log)
    assert rm.same(want, got) == []
    return log


@pytest.mark.parametrize("case", rc.hand_cases(), ids=lambda c: c[0])
def test_one_message_of_each_kind_by_hand(codec, case):
    name, st, msgs, n_ids, n_chans, want = case
    frame, cols = decode(codec, msgs)
    tab, _, _ = rm.tables_of(st, n_ids, n_chans)
    ids, spans = rm.split(msgs)
    out = library_call(codec, frame, cols)(tab, ids, spans, 0, 0)
    for field, v in want.items():
        assert out[field] == v, field


@pytest.mark.parametrize("case", rc.crafted_cases(), ids=lambda c: c[0])
def test_crafted_sequences(codec, case):
    run_case(codec, case)


@pytest.mark.parametrize("case", rc.sized_cases(), ids=lambda c: c[0])
def test_every_block_and_segment_edge_in_one_call(codec, case):
    assert len(run_case(codec, case)) == 1


def test_random_batches_chained(codec):
    stops = set()
    for case in rc.random_cases():
        stops |= {s for s, _ in run_case(codec, case)}
    assert stops == {0, 1, 2}


def test_resuming_in_the_middle_and_at_the_end(codec):
    name, st, msgs, n_ids, n_chans, _ = rc.sized_cases()[4]
    frame, cols = decode(codec, msgs)
    tab, _, _ = rm.tables_of(st, n_ids, n_chans)
    ids, spans = rm.split(msgs)
    call = library_call(codec, frame, cols)
    k = len(spans) // 2
    call(tab, ids, spans, spans[k][0], k)                  # from the middle, two epochs in a row
    call(tab, ids, spans, spans[k][0], k)
    out = call(tab, ids, spans, len(ids), len(spans))      # the empty run
    assert out["stopped"] == 0 and out["outcome"] == [] and out["reply"] == b""


# ---- capacities -------------------------------------------------------------------------------------
def capacity_case():
    st = rc.base_state()
    msgs = [("upd", 1), ("upd", 5), ("unsub", 1), ("sub", b"/p/a", 6), ("upd", 6), ("sub", b"/p/none", 4),
            ("unsub", 2), ("sub", b"/p/stop", 7), ("upd", 1)]
    return st, msgs


def raw_call(codec, tab, frame, cols, caps):
    """The call with arrays longer than the capacities it is told, the rest filled with 0x5A."""
    import torch
    from netidx_amd.codec import NetidxError, NxgDispatch, NxgReplyRoute, lib
    t = device_table(codec, tab)
    n_ctl = int(cols.s.n_ctl)
    arrs = {}

    def arr(name, n, dt=torch.int64):
        a = torch.full((n + 8,), 0x5A5A5A5A5A5A5A5A if dt == torch.int64 else 0x5A5A5A5A if
                       dt == torch.int32 else 0x5A, dtype=dt, device="cuda")
        arrs[name] = (a, n)
        return a.data_ptr()

    s = NxgReplyRoute()
    s.cap_spans = n_ctl
    s.outcome, s.span_q, s.span_id = arr("outcome", n_ctl, torch.uint8), arr("span_q", n_ctl), arr("span_id", n_ctl)
    s.disp = NxgDispatch(caps["entries"], arr("chan_off", tab["n_chans"] + 1), arr("ent_sub", caps["entries"]),
                         arr("ent_row", caps["entries"]), arr("last_row", len(tab["slots"])), 0, 0)
    s.cap_sub = caps["sub"]
    s.sub_span, s.sub_q, s.sub_id = arr("sub_span", caps["sub"]), arr("sub_q", caps["sub"]), arr("sub_id", caps["sub"])
    s.cap_unsub = caps["unsub"]
    s.unsub_id, s.unsub_slot = arr("unsub_id", caps["unsub"]), arr("unsub_slot", caps["unsub"], torch.int32)
    s.cap_reply, s.reply = caps["reply"], arr("reply", caps["reply"], torch.uint8)
    torch.cuda.synchronize()
    tb, err = t.c_struct(), NetidxError()
    ok = lib().nxg_route_replies(codec.ctx, C.byref(tb), C.c_void_p(frame.data_ptr()), C.byref(cols.s),
                                 0, 0, C.byref(s), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    if err.msg:
        lib().nxg_error_free(C.byref(err))
    for name, (a, n) in arrs.items():
        tail = a[n:].cpu().numpy().view(np.uint8)
        assert (tail == 0x5A).all(), name
    t.pending.close()
    return ok, s, msg, {k: v[0][:v[1]].cpu().numpy() for k, v in arrs.items()}


def test_capacities_exact_and_one_short(codec):
    st, msgs = capacity_case()
    frame, cols = decode(codec, msgs)
    tab, _, _ = rm.tables_of(st, rc.N_IDS, rc.N_CHANS)
    ids, spans = rm.split(msgs)
    want = rm.contract_call(tab, ids, spans, 0, 0)
    need = {"entries": sum(len(c) for c in want["chan"]), "sub": len(want["sub"]),
            "unsub": len(want["unsub"]), "reply": len(want["reply"])}
    assert all(v >= 2 for v in need.values()) and want["stopped"] == 0
    ok, s, msg, h = raw_call(codec, tab, frame, cols, need)
    assert ok, msg
    assert h["reply"].tobytes() == want["reply"]
    assert h["sub_id"].view(np.uint64).tolist() == [x[2] for x in want["sub"]]
    assert h["unsub_slot"].view(np.uint32).tolist() == [x[1] for x in want["unsub"]]
    for short in need:
        caps = dict(need)
        caps[short] -= 1
        ok, s, msg, h = raw_call(codec, tab, frame, cols, caps)
        assert not ok and "NXG_CAPACITY" in msg, short
        assert (s.n_entries, s.n_sub, s.n_unsub, s.reply_len) == (
            need["entries"], need["sub"], need["unsub"], need["reply"])
        assert h["reply"].tobytes() == want["reply"][:caps["reply"]]          # what fitted
        assert h["unsub_id"].view(np.uint64).tolist() == [x[0] for x in want["unsub"]][:caps["unsub"]]


# ---- misuse: refused before any launch, the message names the field -------------------------------
def test_misuse(codec):
    from netidx_amd.codec import CodecError, Columns, LAYOUT_F64, LAYOUT_MIXED, MEM_HOST
    st, msgs = capacity_case()
    frame, cols = decode(codec, msgs)
    tab, _, _ = rm.tables_of(st, rc.N_IDS, rc.N_CHANS)
    t = device_table(codec, tab)

    def refused(word, cols=cols, frame=frame, table=t, **kw):
        with pytest.raises(CodecError) as e:
            codec.route_replies(table, frame, cols, **kw)
        assert word in str(e.value), str(e.value)

    refused("ctl_begin", ctl_begin=cols.s.n_ctl + 1)
    refused("row_begin", row_begin=cols.s.n_rows + 1)
    f64 = Columns(8, 0, 0, LAYOUT_F64, "cuda")
    refused("cols->layout", cols=f64)
    host = Columns(8, 1, 8, LAYOUT_MIXED, "cuda")
    host.s.mem = MEM_HOST  # columns that say they are host memory
    refused("cols->mem", cols=host)
    hostptr = np.zeros(64, np.uint8)

    class HostFrame:  # a frame that claims to be on the device
        device = frame.device

        def data_ptr(self):
            return hostptr.ctypes.data
    refused("frame", frame=HostFrame())
    saved = cols.s.id
    cols.s.id = None
    refused("cols->id: null")
    cols.s.id = saved
    # a request whose slot the table does not have: found on the device, the span named
    bad = dict(tab, pend_slot=[len(tab["slots"])] * len(tab["pend_slot"]))
    tb = device_table(codec, bad)
    refused("tab->pend_slot", table=tb)
    tb.pending.close()
    # async work pending on the ctx
    w = rc.wire_of(msgs)
    other = Columns.for_frame(len(w), LAYOUT_MIXED, "cuda")
    codec.decode_async(frame.data_ptr(), len(w), other)
    refused("async")
    codec.sync()
    codec.route_replies(t, frame, cols)  # and the ctx still works
    t.pending.close()
