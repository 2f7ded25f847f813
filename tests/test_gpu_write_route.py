"""GPU tests of nxg_route_writes against the Python model (tests/write_route_model.py), which
restates handle_batch_inner's Write / Unsubscribe arms and write() (publisher/server.rs:171-245,
497-576) and shares no code with the library.

Frames are built with to_twin and decoded with codec.decode_writes. Bar: every output equal to the
model's -- the outcome per row, each channel's requests and their order, the reply bytes, the wait
triples, unsub_id, every count, and next_row / next_ctl at every stop. Every check goes through
the resume loop around Subscribe (one call when the batch has none)."""
import random

import numpy as np
import pytest

import to_twin as tw
import write_route_model as wm

pytestmark = pytest.mark.gpu

BLOCK = 256  # rows (and spans) per workgroup of the routing scans (nxg_internal.h kRwBlock)


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
    """A pool of Values of every kind (text, arrays, maps included: rows of every decode bucket)."""
    global _values
    if _values is None:
        rng = random.Random(99)
        _values = [tw.mg().rand_value(rng) for _ in range(64)]
        _values += [(12, b"text"), (19, [(12, b"a"), (9, 7)]), (16, None)]
    return _values


def wire_of(items):
    """items: ("w", id, r, wid | None) | ("unsub", id) | ("unsub", id, raw message bytes) |
    ("sub", k). Returns the frame; the Write values cycle through the pool."""
    vs = values()
    out = bytearray()
    for n, m in enumerate(items):
        if m[0] == "w":
            out += tw.write(m[1], m[2], vs[n % len(vs)], m[3])
        elif m[0] == "unsub":
            out += m[2] if len(m) > 2 else tw.unsubscribe(m[1])
        else:
            out += tw.subscribe("/p/%d" % m[1], timestamp=m[1], token=b"t")
    return bytes(out)


def table_of(st, n_ids, n_chans):
    from netidx_amd.codec import WriteTable
    if st.subscribed is None:  # a client the publisher does not know: n_ids = 0
        return WriteTable.from_state({}, {}, n_chans, n_ids=0)
    return WriteTable.from_state(st.subscribed, st.on_write, n_chans, n_ids=n_ids)


def decode(codec, items):
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    w = wire_of(items)
    frame = dev(w)  # (an empty frame: one unused byte, so that there is a device pointer)
    cols = Columns(len(w) // 5 + 1, len(w) + 1, len(w) // 3 + 1, LAYOUT_MIXED, "cuda")
    wcols = WriteCols(len(w) // 5 + 1, "cuda")
    codec.decode_writes(frame if w else b"", cols, wcols)
    return frame, cols, wcols


def route_all(codec, st0, items, n_ids, n_chans, fresh=0, on_subscribe=None):
    """The host loop around Subscribe: returns the calls' outputs joined, and the stops."""
    frame, cols, wcols = decode(codec, items)
    assert cols.s.n_rows == sum(1 for m in items if m[0] == "w")
    assert cols.s.n_ctl == len(items) - cols.s.n_rows
    st = st0.copy()
    got = wm.Result()
    got.n_outcome = [0, 0, 0, 0]
    stops = []
    row = ctl = 0
    calls = 0
    while True:
        r = codec.route_writes(table_of(st, n_ids, n_chans), frame, cols, wcols, row, ctl,
                               (fresh + got.n_fresh) & tw.M64)
        calls += 1
        h = r.numpy()
        got.outcome += h["outcome"].tolist()
        for c, ents in r.batches().items():
            got.batches.setdefault(c, []).extend(ents)
        got.reply += h["reply"]
        got.n_replies += r.n_replies
        got.wait += h["wait"]
        got.unsub += h["unsub_id"]
        got.n_fresh += r.n_fresh
        assert r.n_entries == sum(len(e) for e in r.batches().values())
        assert r.n_outcome == [int((h["outcome"] == o).sum()) for o in range(4)]
        got.n_outcome = [a + b for a, b in zip(got.n_outcome, r.n_outcome)]
        for i in h["unsub_id"]:  # the host's own unsubscribe() bookkeeping
            if st.subscribed is not None:
                st.subscribed.pop(i, None)
        row, ctl = r.next_row, r.next_ctl
        if not r.stopped_at_subscribe:
            assert (row, ctl) == (cols.s.n_rows, cols.s.n_ctl)
            break
        stops.append((row, ctl))
        if on_subscribe is not None:
            on_subscribe(st, ("sub", len(stops) - 1))
    got.calls = calls
    return got, stops


def check(codec, st0, items, n_ids, n_chans, fresh=0, on_subscribe=None):
    want = wm.handle_batch(st0.copy(), [m[:4] if m[0] == "w" else m[:2] for m in items], fresh,
                           on_subscribe)
    got, stops = route_all(codec, st0, items, n_ids, n_chans, fresh, on_subscribe)
    assert got.outcome == want.outcome
    assert bytes(got.reply) == bytes(want.reply)
    assert got.n_replies == want.n_replies
    assert got.wait == want.wait
    assert got.unsub == want.unsub
    assert got.n_fresh == want.n_fresh
    assert got.n_outcome == [want.outcome.count(o) for o in range(4)]
    assert {c: [tuple(e) for e in v] for c, v in got.batches.items()} == want.batches
    # the stops: each Subscribe's place among the rows and the control spans
    exp, rows, ctl = [], 0, 0
    for m in items:
        if m[0] == "w":
            rows += 1
        else:
            ctl += 1
            if m[0] == "sub":
                exp.append((rows, ctl))
    assert stops == exp
    return want, got


def rand_wid(rng):
    k = rng.randrange(1, 11)  # varint bytes
    if k == 10:
        return rng.getrandbits(64) | (1 << 63)
    return rng.getrandbits(7 * k) | (1 << (7 * k - 1)) if k > 1 else rng.getrandbits(7)


def rand_state(rng, n_ids, n_chans, max_list=3):
    sub = {i: rng.choice([0x04, 0x05, 0x07, 0x01, 0x03, 0x00, 0xFFFFFFFE])
           for i in range(n_ids) if rng.random() < 0.8}
    ow = {i: [rng.randrange(n_chans) for _ in range(rng.randrange(max_list + 1))]
          for i in range(n_ids) if rng.random() < 0.7}
    ow = {i: list(dict.fromkeys(c)) for i, c in ow.items()}  # a list names a channel once
    return wm.State(sub, ow)


def rand_id(rng, n_ids):
    k = rng.random()
    if k < 0.8 and n_ids:
        return rng.randrange(n_ids)
    if k < 0.9:
        return n_ids + rng.randrange(3)
    b = rng.choice([14, 21, 28, 35, 36, 50, 64])
    return rng.getrandbits(b) | (1 << (b - 1))


def rand_items(rng, n_rows, n_spans, n_ids, n_subs=0):
    kinds = ["w"] * n_rows + ["unsub"] * n_spans + ["sub"] * n_subs
    rng.shuffle(kinds)
    items, k = [], 0
    for kind in kinds:
        if kind == "w":
            items.append(("w", rand_id(rng, n_ids), rng.random() < 0.5,
                          None if rng.random() < 0.2 else rand_wid(rng)))
        elif kind == "unsub":
            items.append(("unsub", rand_id(rng, n_ids)))
        else:
            items.append(("sub", k))
            k += 1
    return items


# ---- row counts ---------------------------------------------------------------------------------
# 0: nothing at all; 63/64/65, 128/129: a wave, two waves; BLOCK +- 1: the scans' block size
@pytest.mark.parametrize("n_rows,n_spans", [(0, 0), (0, 5), (0, BLOCK + 1), (1, 0), (1, 1), (63, 3),
                                            (64, 3), (65, 3), (128, 9), (129, 9), (BLOCK - 1, 20),
                                            (BLOCK, 20), (BLOCK + 1, 20), (3 * BLOCK + 7, 2 * BLOCK + 3)])
def test_random_batches(codec, n_rows, n_spans):
    rng = random.Random(1000 * n_rows + n_spans)
    st = rand_state(rng, 48, 5)
    check(codec, st, rand_items(rng, n_rows, n_spans, 48), 48, 5, fresh=rng.getrandbits(40))


def test_large_batch(codec):
    rng = random.Random(7)
    n_ids = 5000
    st = rand_state(rng, n_ids, 16)
    want, got = check(codec, st, rand_items(rng, 200_000, 2000, n_ids), n_ids, 16, fresh=2**63)
    assert got.calls == 1 and all(n > 1000 for n in got.n_outcome)


# ---- the rules, with the expected outcomes written out ---------------------------------------------
def test_every_outcome_with_and_without_reply(codec):
    n_ids = 8
    st = wm.State({0: 0x04, 1: 0x04, 2: 0x03, 3: 0x07, 4: 0x04, 7: 0xFFFFFFFE},
                  {0: [1], 1: [], 2: [0], 4: [0, 1], 5: [1], 7: [1, 0]})
    items = []
    for r in (True, False):
        items += [("w", 0, r, 1), ("w", 4, r, 2),      # routed
                  ("w", 5, r, 3), ("w", 6, r, 4),      # not subscribed (5 has on_write only)
                  ("w", 2, r, 5),                      # no WRITE bit
                  ("w", 1, r, 6), ("w", 3, r, 7),      # empty channel list; no on_write entry
                  ("w", 7, r, 8),                      # id == n_ids - 1, every bit but NOT_SUBSCRIBED
                  ("w", 8, r, 9),                      # id == n_ids
                  ("w", 2**35 + 11, r, 10), ("w", 2**64 - 1, r, 11)]
    want, got = check(codec, st, items, n_ids, 2)
    assert got.outcome == [0, 0, 1, 1, 2, 3, 3, 0, 1, 1, 1] * 2
    assert got.n_replies == 8 and len(got.wait) == 3
    assert got.batches == {1: [(0, 0), (4, 1), (7, 7), (0, 11), (4, 12), (7, 18)],
                           0: [(4, 1), (7, 7), (4, 12), (7, 18)]}


def test_unknown_client_is_unsubscribed(codec):
    st = wm.State(None, {1: [0]})
    want, got = check(codec, st, [("w", 1, True, 5), ("w", 0, False, 6), ("unsub", 1),
                                  ("w", 2**40, True, None)], 0, 1, fresh=77)
    assert got.outcome == [1, 1, 1] and got.n_replies == 3 and got.n_fresh == 1


def test_unsubscribe_and_write_to_the_same_id(codec):
    st = wm.State({i: 0x04 for i in range(6)}, {i: [0] for i in range(6)})
    noncanon = bytes([0x83, 0x00, 0x01, 0x03])        # varint(L = 3) in two bytes
    trailing = tw.unsubscribe(4, trailing=b"\xff\x00\x80")
    items = [("w", 0, True, 1), ("unsub", 0), ("w", 0, True, 2),   # directly before / after
             ("w", 1, True, 3), ("w", 1, True, 4), ("unsub", 1),
             ("unsub", 2), ("unsub", 5), ("unsub", 2),              # one ctl_row; an id twice
             ("w", 2, True, 5), ("w", 5, False, 6),
             ("w", 3, True, 7), ("unsub", 3, noncanon), ("w", 3, True, 8),
             ("w", 4, False, 9), ("unsub", 4, trailing), ("w", 4, True, 10),
             ("unsub", 2**50), ("unsub", 1)]                        # last messages
    want, got = check(codec, st, items, 6, 1)
    assert got.outcome == [0, 1, 0, 0, 1, 1, 0, 1, 0, 1]
    assert got.unsub == [0, 1, 2, 5, 2, 3, 4, 2**50, 1]


@pytest.mark.parametrize("r", [True, False])
def test_varint_widths_in_replies(codec, r):
    ids = [0, 0x7F, 0x80, 0x3FFF, 0x4000, 2**21 - 1, 2**21, 2**28 - 1, 2**28, 2**35 - 1, 2**63,
           2**64 - 1]
    wids = [0] + [2**(7 * k) - 1 for k in range(1, 10)] + [2**(7 * k) for k in range(1, 10)] + \
        [2**64 - 1]
    items = [("w", ids[n % len(ids)], r, w) for n, w in enumerate(wids)]
    items += [("unsub", i) for i in ids]
    items += [("w", 2**35 + n, r, None) for n in range(4)]
    # fresh WriteIds whose width changes inside the block: 2^14 - 2 .. 2^14 + 1
    check(codec, wm.State({}, {}), items, 0, 1, fresh=2**14 - 2)


def test_fresh_wids_near_the_top(codec):
    items = [("w", 3, True, None), ("w", 3, True, 5), ("w", 3, True, None), ("w", 3, False, None),
             ("w", 3, True, None)]
    want, got = check(codec, wm.State({}, {}), items, 4, 1, fresh=2**64 - 2)
    assert got.n_fresh == 4


# ---- channels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chans", [1, 1025])
def test_channel_counts(codec, n_chans):
    rng = random.Random(n_chans)
    st = rand_state(rng, 40, n_chans)
    if n_chans > 1:
        st.on_write[0] = [1024, 0, 512]
        st.subscribed[0] = 0x04
    check(codec, st, rand_items(rng, 300, 10, 40), 40, n_chans)


def test_a_list_naming_one_channel_twice(codec):
    st = wm.State({0: 0x04, 1: 0x04, 2: 0x04}, {0: [1, 1], 1: [0, 1, 0], 2: [1]})
    items = [("w", n % 3, n % 2 == 0, n) for n in range(200)]
    want, got = check(codec, st, items, 3, 2)
    assert len(got.batches[1]) == 67 * 2 + 67 + 66


# ---- Subscribe: the resume loop ---------------------------------------------------------------------
def _on_subscribe(st, m):
    k = m[1]
    st.subscribed[k % 48] = 0x04           # the host's subscribe(): a new subscription
    st.on_write.setdefault(k % 48, [k % 5])


@pytest.mark.parametrize("where", ["first", "middle", "last", "pair", "only", "many"])
def test_subscribes(codec, where):
    rng = random.Random(len(where) * 31)
    st = rand_state(rng, 48, 5)
    body = rand_items(rng, 300, 12, 48)
    if where == "first":
        items = [("sub", 0)] + body
    elif where == "middle":
        items = body[:150] + [("sub", 0)] + body[150:]
    elif where == "last":
        items = body + [("sub", 0)]
    elif where == "pair":
        items = body[:100] + [("sub", 0), ("sub", 1)] + body[100:]
    elif where == "only":
        items = [("sub", 0)]
    else:
        items = rand_items(rng, 600, 30, 48, n_subs=7)
    want, got = check(codec, st, items, 48, 5, fresh=500, on_subscribe=_on_subscribe)
    assert got.calls == sum(1 for m in items if m[0] == "sub") + 1


def test_subscribe_resubscribes_an_id_unsubscribed_earlier(codec):
    st = wm.State({1: 0x04}, {1: [0]})
    items = [("w", 1, True, 1), ("unsub", 1), ("w", 1, True, 2), ("sub", 0), ("w", 1, True, 3)]

    def on_sub(s, m):
        s.subscribed[1] = 0x04

    want, got = check(codec, st, items, 2, 1, on_subscribe=on_sub)
    assert got.outcome == [0, 1, 0]


# ---- capacity ---------------------------------------------------------------------------------------
def test_capacities_one_short_and_exact(codec):
    from netidx_amd.codec import RouteCapacity
    rng = random.Random(5)
    st = rand_state(rng, 48, 5)
    items = rand_items(rng, 500, 25, 48)
    want = wm.handle_batch(st.copy(), items, 0)
    need = {"cap_entries": sum(len(v) for v in want.batches.values()), "cap_wait": len(want.wait),
            "cap_unsub": len(want.unsub), "cap_reply": len(want.reply)}
    assert all(v > 1 for v in need.values())
    frame, cols, wcols = decode(codec, items)
    tab = table_of(st, 48, 5)
    for k, v in need.items():
        caps = dict(need)
        caps[k] = v - 1
        with pytest.raises(RouteCapacity) as e:
            codec.route_writes(tab, frame, cols, wcols, **caps)
        r = e.value.route
        assert (r.n_entries, r.n_wait, r.n_unsub, r.reply_len) == (
            need["cap_entries"], need["cap_wait"], need["cap_unsub"], need["cap_reply"])
        assert "NXG_CAPACITY" in str(e.value)
    r = codec.route_writes(tab, frame, cols, wcols, **need)  # the exact capacities
    h = r.numpy()
    assert h["reply"] == bytes(want.reply) and h["wait"] == want.wait
    assert h["unsub_id"] == want.unsub and h["outcome"].tolist() == want.outcome
    assert {c: [tuple(x) for x in v] for c, v in r.batches().items()} == want.batches


# ---- state between calls ----------------------------------------------------------------------------
def test_second_call_sees_no_earlier_unsubscribe(codec):
    n_ids = 600
    st = wm.State({i: 0x04 for i in range(n_ids)}, {i: [i % 3] for i in range(n_ids)})
    first = [("unsub", i) for i in range(n_ids)] + [("w", i, True, i) for i in range(n_ids)]
    want, got = check(codec, st, first, n_ids, 3)
    assert got.outcome == [1] * n_ids
    second = [("w", i, True, i) for i in range(n_ids)] + [("unsub", 5)]
    want, got = check(codec, st, second, n_ids, 3)  # the same table: every Id still subscribed
    assert got.outcome == [0] * n_ids and len(got.wait) == n_ids
