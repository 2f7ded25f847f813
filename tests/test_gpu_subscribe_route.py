"""GPU tests of nxg_route_subscribes against the Python model (tests/subscribe_route_model.py),
which restates handle_batch_inner's Subscribe arm and subscribe() (publisher/server.rs:60-137,
506-549) and shares no code with the library.

Frames are built with to_twin and decoded with codec.decode_writes. Bar: every output equal to the
model's -- the outcome and Id per span, sub_id / sub_perm in order, the deferred spans, the reply
bytes, every count, and next_ctl / stopped at every stop."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import subscribe_route_model as sm
import to_twin as tw
import write_route_model as wm

pytestmark = pytest.mark.gpu

BLOCK = 256  # spans per workgroup of the routing scans (nxg_internal.h kRwBlock)
F64_1 = (9, struct.unpack(">Q", struct.pack(">d", 1.0))[0])


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
    return torch.from_numpy(np.frombuffer(bytes(wire) or b"\x00", np.uint8).copy()).cuda()


_values = None


def values():
    """A pool of Values of every kind: the random pool of the write tests, plus a nested
    Array-in-Map, an empty string, an Error(Value) and empty containers."""
    global _values
    if _values is None:
        rng = random.Random(99)
        _values = [tw.mg().rand_value(rng) for _ in range(64)]
        _values += [(12, b"text"), (19, [(12, b"a"), (9, 7)]), (16, None), (12, b""),
                    (21, [((12, b"k"), (19, [(4, 1), (19, [(12, b"deep")])]))]),
                    (22, (21, [((4, 5), (16, None))])), (19, []), (21, []), (18, b"err"),
                    (19, [(9, i) for i in range(70)]),
                    # the tags the seeded pool has only inside containers
                    (7, -2**40 - 5), (11, (2**63 + 1, 999999999)), (20, bytes(range(16))),
                    (27, bytes(range(40, 62)))]
    return _values


def wire_of(items):
    """items: ("sub", path, perm | None) | ("w", id, r, wid | None) | ("unsub", id)."""
    out = bytearray()
    for n, m in enumerate(items):
        if m[0] == "sub":
            out += tw.subscribe(m[1], timestamp=n, permissions=n & 0xFF, token=b"tok")
        elif m[0] == "w":
            out += tw.write(m[1], m[2], (9, n), m[3])
        else:
            out += tw.unsubscribe(m[1])
    return bytes(out)


def decode(codec, items):
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    w = wire_of(items)
    frame = dev(w)
    cols = Columns(len(w) // 5 + 1, len(w) + 1, len(w) // 3 + 1, LAYOUT_MIXED, "cuda")
    wcols = WriteCols(len(w) // 5 + 1, "cuda")
    codec.decode_writes(frame if w else b"", cols, wcols)
    assert cols.s.n_ctl == sum(1 for m in items if m[0] != "w")
    return frame, cols, wcols


def table_of(codec, st, n_ids=None):
    from netidx_amd.codec import SubscribeTable
    return SubscribeTable.from_state(codec, st.by_path, st.by_id, n_ids=n_ids,
                                     denied_ids=st.denied_ids, defaults=st.default,
                                     deferred_room=sm.MAX_DEFERRED - st.deferred_len)


def perms_of(items):
    """span_perm[] of the frame's control spans (None: Anonymous, when no Subscribe has one)."""
    spans = [m for m in items if m[0] != "w"]
    if all(m[0] != "sub" or m[2] is None for m in spans):
        return None
    return [m[2] if m[0] == "sub" and m[2] is not None else sm.ALL for m in spans]


def check_run(codec, st0, items, ctl_begin=0, row_begin=0, n_ids=None, want_stop=None, tab=None,
              decoded=None):
    """One call over the run that starts at span ctl_begin, against the model. tab: a
    SubscribeTable that holds st0 (default: one built fresh from it); decoded: what decode()
    returned for these items (default: decoded here)."""
    frame, cols, _ = decoded if decoded is not None else decode(codec, items)
    spans, rows = [], 0  # (message, rows in front of it) per control span
    for m in items:
        if m[0] == "w":
            rows += 1
        else:
            spans.append((m, rows))
    perm = perms_of(items)
    run = []
    for m, row in spans[ctl_begin:]:
        if m[0] != "sub" or row != row_begin:
            break
        run.append(m[1])
    st = st0.copy()
    want, n = sm.route(st, run, perm, ctl_begin)
    r = codec.route_subscribes(tab if tab is not None else table_of(codec, st0, n_ids), frame, cols,
                               row_begin, ctl_begin, perm)
    h = r.numpy()
    assert r.next_ctl == ctl_begin + n and r.n_spans == n
    assert h["outcome"] == want.outcome
    assert h["span_id"] == [sm_id if sm_id is not None else 2**64 - 1 for sm_id in want.span_id]
    assert h["sub"] == want.sub and r.n_sub == len(want.sub)
    assert h["deferred"] == want.deferred and r.n_deferred == len(want.deferred)
    assert h["reply"] == bytes(want.reply) and r.reply_len == len(want.reply)
    assert r.n_replies == want.n_replies
    assert r.n_outcome == [want.outcome.count(o) for o in range(5)]
    if want_stop is not None:
        assert r.stopped == want_stop
    return want, r


# ---- the rules ----------------------------------------------------------------------------------
def base_state(**kw):
    return sm.State({b"/a": 1, b"/b": 2, b"/gone": 9, b"/far": 40}, {1: F64_1, 2: (12, b"x")},
                    default=[b"/dflt"], denied_ids={2}, **kw)


@pytest.mark.parametrize("path,outcome", [(b"/a", 0), (b"/nope", 1), (b"/b", 2), (b"/dflt/x", 3),
                                          (b"/gone", 4), (b"/far", 4)])
def test_one_subscribe_of_each_outcome(codec, path, outcome):
    # /gone: an Id in by_path whose slot is NXG_NO_SLOT; /far: an Id >= n_ids
    want, r = check_run(codec, base_state(), [("sub", path, None)], n_ids=12, want_stop=0)
    assert want.outcome == [outcome]


def mixed_run(rng, n, st):
    paths = list(st.by_path) + [b"/dflt/%d" % i for i in range(5)] + [b"/none/%d" % i for i in range(5)]
    return [("sub", rng.choice(paths), rng.choice([None, 0x3F, 0x03, sm.DENY, 0x04])) for _ in range(n)]


@pytest.mark.parametrize("n", [BLOCK + 1, 2 * BLOCK + 1])
def test_runs_with_every_outcome_mixed(codec, n):
    rng = random.Random(n)
    # Ids 30 .. 39 are past n_ids, the odd ones below have no slot: by_id has neither
    st = sm.State({b"/p/%d" % i: i for i in range(40)}, {i: values()[i] for i in range(0, 30, 2)},
                  default=[b"/dflt"], denied_ids={4, 8, 12})
    want, r = check_run(codec, st, mixed_run(rng, n, st), n_ids=30, want_stop=0)
    assert all(want.outcome.count(o) > 5 for o in range(5))


def test_the_same_path_twice(codec):
    want, r = check_run(codec, base_state(), [("sub", b"/a", None), ("sub", b"/a", None)])
    assert want.outcome == [0, 0] and want.sub == [(1, sm.ALL)] * 2


def test_current_values_of_every_tag(codec):
    vs = values()
    st = sm.State({b"/v/%d" % i: i for i in range(len(vs))}, dict(enumerate(vs)))
    want, r = check_run(codec, st, [("sub", b"/v/%d" % i, None) for i in range(len(vs))])
    assert want.outcome == [0] * len(vs)
    assert {v[0] for v in vs} >= set(range(17)) | {18, 19, 20, 21, 22, 23, 24, 25, 26, 27}


def test_widths_of_the_length_prefixes_and_ids(codec):
    # Subscribed body = 1 + vl(|p|) + |p| + vl(id) + 9 (F64): |p| = 114 / 115 with a one-byte id
    # gives bodies of 126 / 127 bytes (L 127 in one byte, 129 in two); |p| = 128: varint(|p|) two
    p114, p115, p128 = b"/" + b"a" * 113, b"/" + b"b" * 114, b"/" + b"c" * 127
    ids = {p114: 3, p115: 4, p128: 5, b"/i127": 127, b"/i128": 128, b"/i14": 2**14,
           b"/i21": 2**21, b"/i35": 2**35}
    st = sm.State(ids, {i: F64_1 for i in ids.values() if i < 2**35})
    want, r = check_run(codec, st, [("sub", p, None) for p in ids] + [("sub", p128 + b"x", None)])
    assert want.outcome == [0] * 7 + [4, 1]  # 2^35 is past n_ids: by_id has no such Id
    assert len(sm.subscribed(p114, 3, F64_1)) == 127 and len(sm.subscribed(p115, 4, F64_1)) == 129


def test_long_paths_past_the_staging_window(codec):
    # a workgroup stages 24 KiB of its spans' bytes; 256 spans with paths of 150-400 bytes are
    # about 70 KiB, so the later spans of each block are read from global memory
    rng = random.Random(8)
    paths = [b"/long/%03d/" % i + bytes(rng.choice(b"abcdefghij") for _ in range(rng.randrange(140, 390)))
             for i in range(BLOCK + 44)]
    st = sm.State({p: i for i, p in enumerate(paths) if i % 3}, {i: (9, i) for i in range(0, 300, 2)},
                  default=[b"/long/1"])
    want, r = check_run(codec, st, [("sub", p, None) for p in paths], want_stop=0)
    assert all(want.outcome.count(o) > 10 for o in (0, 1, 3, 4))


def test_span_perm_null_against_an_explicit_array(codec):
    st = base_state()
    items = [("sub", b"/a", None), ("sub", b"/nope", None), ("sub", b"/a", None)]
    anon, _ = check_run(codec, st, items)
    same, _ = check_run(codec, st, [(m[0], m[1], sm.ALL) for m in items])
    assert bytes(anon.reply) == bytes(same.reply) and anon.sub == same.sub
    want, _ = check_run(codec, st, [("sub", b"/a", sm.DENY), ("sub", b"/nope", sm.DENY),
                                    ("sub", b"/a", 0x03), ("sub", b"/dflt/q", sm.DENY),
                                    ("sub", b"/a", 0)])
    assert want.outcome == [2, 2, 0, 2, 0] and want.sub == [(1, 0x03), (1, 0)]


def test_extended_auth_denies(codec):
    want, _ = check_run(codec, base_state(), [("sub", b"/b", None), ("sub", b"/a", None)])
    assert want.outcome == [2, 0]
    st = base_state()
    st.denied_ids = None  # no extended_auth: allow_of_id NULL
    want, _ = check_run(codec, st, [("sub", b"/b", None)])
    assert want.outcome == [0]


# ---- default publishers -------------------------------------------------------------------------
def test_defaults(codec):
    none = sm.State({b"/a": 1}, {1: F64_1})
    want, _ = check_run(codec, none, [("sub", b"/x", None), ("sub", b"/a", None)])
    assert want.outcome == [1, 0]
    two = sm.State({}, {}, default=[b"/a", b"/a/b"])
    want, _ = check_run(codec, two, [("sub", p, None) for p in
                                     (b"/a/c", b"/a/b/c", b"/a/b", b"/a", b"/0", b"/a/bb", b"/b")])
    assert want.outcome == [1, 3, 3, 3, 1, 3, 1]
    one = sm.State({}, {}, default=[b"/d"])
    want, _ = check_run(codec, one, [("sub", p, None) for p in (b"/dx", b"/d", b"/c", b"/e")])
    assert want.outcome == [3, 3, 1, 1]
    # many bases, long ones, and bases that differ past the first 8-byte word
    rng = random.Random(3)
    bases = [b"/base/%05d/%s" % (rng.randrange(10**5), b"z" * rng.randrange(1, 12)) for _ in range(50)]
    many = sm.State({}, {}, default=bases)
    paths = [rng.choice(bases) + rng.choice([b"", b"/leaf", b"0"]) for _ in range(100)]
    paths += [b[:-1] + b"y" for b in bases[:20]]  # just below a base: another one is found
    want, _ = check_run(codec, many, [("sub", p, None) for p in paths])
    assert len(want.outcome) == 120 and want.outcome.count(3) > 50 and want.outcome.count(1) > 5


@pytest.mark.parametrize("room", [0, 1, 2])
def test_deferred_room_runs_out_mid_run(codec, room):
    # candidates at spans 0 and 300 (another block), and two more inside the first block
    items = [("sub", b"/none/%d" % i, None) for i in range(2 * BLOCK)]
    for k in (0, 7, 9, 300):
        items[k] = ("sub", b"/d/%d" % k, None)
    st = sm.State({}, {}, default=[b"/d"], deferred_len=sm.MAX_DEFERRED - room)
    want, r = check_run(codec, st, items)
    assert want.deferred == [0, 7, 9, 300][:room]
    st = sm.State({}, {}, default=[b"/d"], deferred_len=sm.MAX_DEFERRED - 1)
    want, _ = check_run(codec, st, [items[0]] + items[10:])  # room 1, candidates at 0 and 291
    assert want.deferred == [0] and want.outcome[291] == 1


# ---- stops --------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 5, BLOCK - 1, BLOCK, BLOCK + 1])
@pytest.mark.parametrize("bad", [b"/a//b", b"/a\\/b", b"/a/", b""])
def test_a_path_that_is_not_plain_stops_the_run(codec, where, bad):
    items = [("sub", b"/a", None) for _ in range(BLOCK + 40)]
    items[where] = ("sub", bad, None)
    items[where + 3] = ("sub", b"//", None)  # a later one does not matter
    want, r = check_run(codec, base_state(), items, want_stop=2)
    assert r.next_ctl == where
    # the host handles span `where`; the next call resumes behind it
    want, r = check_run(codec, base_state(), items, ctl_begin=where + 1, want_stop=2)
    assert r.next_ctl == where + 3


def test_an_unsubscribe_or_a_write_row_ends_the_run(codec):
    st = base_state()
    items = [("sub", b"/a", None), ("sub", b"/b", None), ("unsub", 1), ("sub", b"/a", None)]
    want, r = check_run(codec, st, items, want_stop=1)
    assert r.next_ctl == 2
    items = [("sub", b"/a", None), ("w", 1, True, 5), ("sub", b"/a", None)]
    want, r = check_run(codec, st, items, want_stop=1)
    assert r.next_ctl == 1
    want, r = check_run(codec, st, items, ctl_begin=1, row_begin=1, want_stop=0)  # behind the row
    assert r.next_ctl == 2 and want.outcome == [0]


def test_a_frame_with_no_subscribe(codec):
    st = base_state()
    for items, stop in (([("unsub", 1), ("unsub", 2)], 1), ([("w", 1, True, 1)], 0), ([], 0),
                        ([("w", 1, True, 1), ("sub", b"/a", None)], 1)):
        want, r = check_run(codec, st, items, want_stop=stop)
        assert r.next_ctl == 0 and r.n_replies == 0 and r.reply_len == 0 and want.outcome == []
    # at the end of the spans: nothing to do
    want, r = check_run(codec, st, [("sub", b"/a", None)], ctl_begin=1, want_stop=0)
    assert r.next_ctl == 1 and r.n_spans == 0


# ---- a mixed frame: the alternation with nxg_route_writes -----------------------------------------
def drive(codec, sst0, wst0, items, n_ids):
    """The host loop of INTEGRATION.md: subscribe runs and write runs in turn."""
    from netidx_amd.codec import WriteTable
    frame, cols, wcols = decode(codec, items)
    n_rows, n_ctl = int(cols.s.n_rows), int(cols.s.n_ctl)
    perm = perms_of(items)
    sst, wst = sst0.copy(), wst0.copy()
    got_s, got_w, handled = sm.Result(), wm.Result(), []
    row = ctl = calls = 0
    while True:
        r = codec.route_subscribes(table_of(codec, sst, n_ids), frame, cols, row, ctl, perm)
        calls += 1
        h = r.numpy()
        got_s.outcome += h["outcome"]
        got_s.sub += h["sub"]
        got_s.deferred += h["deferred"]
        got_s.reply += h["reply"]
        for i, p in h["sub"]:        # the host: cl.subscribed.insert(id, permissions)
            wst.subscribed[i] = p
        sst.deferred_len += r.n_deferred
        ctl = r.next_ctl
        if r.stopped == 2:           # the host handles this Subscribe itself
            handled.append(ctl)
            ctl += 1
            continue
        if ctl == n_ctl and row == n_rows:
            break
        w = codec.route_writes(WriteTable.from_state(wst.subscribed, wst.on_write, 1, n_ids=n_ids),
                               frame, cols, wcols, row, ctl, 0)
        hw = w.numpy()
        got_w.outcome += hw["outcome"].tolist()
        got_w.reply += hw["reply"]
        got_w.unsub += hw["unsub_id"]
        for i in hw["unsub_id"]:     # the host's own unsubscribe() bookkeeping
            wst.subscribed.pop(i, None)
        row, ctl = w.next_row, w.next_ctl - (1 if w.stopped_at_subscribe else 0)
        if not w.stopped_at_subscribe:
            break
    return got_s, got_w, handled, calls


def test_mixed_frame_alternates_with_route_writes(codec):
    sst = sm.State({b"/p": 3, b"/q": 4}, {3: F64_1, 4: (12, b"s")})
    wst = wm.State({}, {3: [0], 4: [0]})
    items = [("sub", b"/p", None), ("w", 3, True, 1), ("unsub", 3), ("w", 3, True, 2),
             ("sub", b"/p", 0x03), ("w", 3, True, 3), ("sub", b"/q", None), ("sub", b"/p", 0x04),
             ("w", 3, True, 4), ("w", 4, True, 5), ("w", 5, True, 6)]
    res = sm.Result()
    msgs, k = [], 0
    for m in items:
        if m[0] == "sub":
            msgs.append(("sub", m[1], k, m[2] if perms_of(items) else None))
        else:
            msgs.append(m)
        k += m[0] != "w"
    want_w = wm.handle_batch(wst.copy(), msgs, 0, sm.on_subscribe(sst.copy(), res))
    got_s, got_w, handled, calls = drive(codec, sst, wst, items, 8)
    # the second write sees the Unsubscribe, the third the permissions without WRITE, the fourth
    # the subscription renewed with WRITE
    assert want_w.outcome == [wm.ROUTED, wm.UNSUBSCRIBED, wm.DENIED, wm.ROUTED, wm.ROUTED,
                              wm.UNSUBSCRIBED]
    assert got_w.outcome == want_w.outcome and bytes(got_w.reply) == bytes(want_w.reply)
    assert got_w.unsub == want_w.unsub
    assert got_s.outcome == res.outcome == [0, 0, 0, 0] and got_s.sub == res.sub
    assert bytes(got_s.reply) == bytes(res.reply) and handled == []


def test_mixed_frame_with_a_path_for_the_host(codec):
    sst = sm.State({b"/p": 3}, {3: F64_1})
    wst = wm.State({}, {3: [0]})
    items = [("sub", b"/p", None), ("sub", b"/p//x", None), ("sub", b"/p", None), ("w", 3, True, 1)]
    got_s, got_w, handled, calls = drive(codec, sst, wst, items, 4)
    assert handled == [1] and got_s.outcome == [0, 0] and got_w.outcome == [wm.ROUTED]


# ---- capacity and misuse ------------------------------------------------------------------------
def raw_call(codec, tab, frame, cols_s, row_begin, ctl_begin, perm_ptr, out):
    from netidx_amd import codec as cm
    err = cm.NetidxError()
    ok = cm.lib().nxg_route_subscribes(codec.ctx, C.byref(tab) if tab is not None else None,
                                       C.c_void_p(frame.data_ptr()), C.byref(cols_s), row_begin,
                                       ctl_begin, C.c_void_p(perm_ptr), C.byref(out), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    cm.lib().nxg_error_free(C.byref(err))
    return ok, msg


def out_struct(n_ctl, caps, keep):
    """An NxgSubscribeRoute whose arrays hold 8 sentinel entries past each capacity."""
    import torch
    from netidx_amd import codec as cm
    o = cm.NxgSubscribeRoute()

    def buf(n, dt):
        t = torch.full((n + 8,), 0x5A, dtype=dt, device="cuda")
        keep.append(t)
        return t

    keep.clear()
    o.cap_spans = n_ctl
    o.outcome, o.span_id = buf(n_ctl, torch.uint8).data_ptr(), buf(n_ctl, torch.int64).data_ptr()
    o.cap_sub, o.cap_deferred, o.cap_reply = caps
    o.sub_id, o.sub_perm = buf(caps[0], torch.int64).data_ptr(), buf(caps[0], torch.int32).data_ptr()
    o.deferred = buf(caps[1], torch.int64).data_ptr()
    o.reply = buf(caps[2], torch.uint8).data_ptr()
    torch.cuda.synchronize()
    return o


def test_capacities_one_short_and_exact(codec):
    rng = random.Random(11)
    st = sm.State({b"/p/%d" % i: i for i in range(20)}, {i: values()[i] for i in range(20)},
                  default=[b"/dflt"])
    items = mixed_run(rng, 300, st)
    items = [(m[0], m[1], None) for m in items]
    frame, cols, _ = decode(codec, items)
    want, _ = sm.route(st.copy(), [m[1] for m in items])
    need = (len(want.sub), len(want.deferred), len(want.reply))
    assert all(v > 1 for v in need)
    tab_keep = table_of(codec, st)
    tab = tab_keep.c_struct()
    keep = []
    for short in range(3):
        caps = tuple(v - (1 if j == short else 0) for j, v in enumerate(need))
        o = out_struct(300, caps, keep)
        ok, msg = raw_call(codec, tab, frame, cols.s, 0, 0, 0, o)
        assert not ok and "NXG_CAPACITY" in msg
        assert (o.n_sub, o.n_deferred, o.reply_len) == need and o.next_ctl == 300
        for t, cap in zip(keep[2:], (caps[0], caps[0], caps[1], caps[2])):
            assert (t[cap:].cpu().numpy() == 0x5A).all()  # nothing past a capacity
    o = out_struct(300, need, keep)
    ok, msg = raw_call(codec, tab, frame, cols.s, 0, 0, 0, o)
    assert ok, msg
    assert keep[5][:need[2]].cpu().numpy().tobytes() == bytes(want.reply)
    assert keep[2][:need[0]].cpu().numpy().tolist() == [i for i, _ in want.sub]
    assert keep[4][:need[1]].cpu().numpy().tolist() == want.deferred
    for t, cap in zip(keep, (300, 300, need[0], need[0], need[1], need[2])):
        assert (t[cap:].cpu().numpy() == 0x5A).all()


def test_misuse_is_refused_before_any_launch(codec):
    from netidx_amd import codec as cm
    st = base_state()
    items = [("sub", b"/a", None), ("sub", b"/b", None)]
    frame, cols, _ = decode(codec, items)
    tab_keep = table_of(codec, st)
    tab = tab_keep.c_struct()
    keep = []
    o = out_struct(2, (2, 2, 64), keep)

    def fails(needle, tab=tab, cols_s=cols.s, ctl_begin=0, perm_ptr=0, out=o):
        ok, msg = raw_call(codec, tab, frame, cols_s, 0, ctl_begin, perm_ptr, out)
        assert not ok and needle in msg, (needle, msg)

    host = cm.NxgColumns.from_buffer_copy(cols.s)
    host.mem = cm.MEM_HOST
    fails("cols->mem", cols_s=host)
    f64 = cm.NxgColumns.from_buffer_copy(cols.s)
    f64.layout = cm.LAYOUT_F64
    fails("cols->layout", cols_s=f64)
    hperm = np.full(2, 0x3F, np.uint32)
    fails("span_perm: not device memory", perm_ptr=hperm.ctypes.data)
    fails("ctl_begin 3", ctl_begin=3)
    fails("tab", tab=None)
    hostout = cm.NxgSubscribeRoute.from_buffer_copy(o)
    hreply = np.zeros(64, np.uint8)
    hostout.reply = hreply.ctypes.data
    fails("out->reply: not device memory", out=hostout)
    ok, msg = raw_call(codec, tab, frame, cols.s, 0, 0, 0, o)  # and the same arguments, valid
    assert ok and o.n_replies == 2, msg
