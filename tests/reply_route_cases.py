"""Cases for nxg_route_replies: one hand-written message per row of the contract's table, crafted
Id-state sequences, and seeded random batches of chosen sizes. Pure Python, deterministic, no GPU.
Every case is (name, State, messages, n_ids, n_chans); messages and State are those of
tests/reply_route_model.py. `wire_of` builds the From frame of a case with the primitives of
tests/golden/make_golden.py.
"""
import random

import path_table_cases as pc
import reply_route_model as rm
import to_twin as tw

S = rm.ENT_SPAN
N_IDS, N_CHANS = 8, 4
# Ids of every varint width, 1-10 bytes (all outside a table of a few Ids)
WIDE_IDS = [2**7 - 1] + [2**(7 * w) for w in range(1, 9)] + [2**63, 2**64 - 1]
PATH_LENGTHS = (1, 7, 8, 9, 127, 128)  # the hash's 8-byte words, a two-byte |p| and L


def path_of_length(n):
    return b"/" if n == 1 else pc.clean_path(n)


# ---- wire --------------------------------------------------------------------------------------------
def message(m, quirk=None):
    """The From message of m. quirk "noncanon": varint(L) with a padding byte; "trailing": bytes
    after the last field inside the wrap (Unsubscribed and Subscribed only)."""
    g = tw.mg()
    path = lambda p: g.enc_varint(len(p)) + p
    if m[0] == "upd":
        return g.update(m[1], (9, m[1] & 0xFFFF))
    if m[0] == "hb":
        return g.HEARTBEAT
    if m[0] == "wr":
        return g.enc_msg(6, g.enc_varint(m[1]) + g.enc_value((16, None)) + g.enc_varint(m[2]))
    if m[0] in ("nsv", "den"):
        return g.enc_msg(0 if m[0] == "nsv" else 1, path(m[1]))
    if m[0] == "unsub":
        variant, body = 2, g.enc_varint(m[1])
    else:
        variant, body = 3, path(m[1]) + g.enc_varint(m[2]) + g.enc_value((12, b"v"))
    if quirk == "trailing":
        body += b"\xff\x00\x80"
    out = g.enc_msg(variant, body)
    if quirk == "noncanon":
        L = g.lw(1 + len(body))
        n = len(g.enc_varint(L))
        pad = bytearray(g.enc_varint(L))
        pad[-1] |= 0x80
        out = bytes(pad) + b"\x00" + out[n:]
    return out


def wire_of(msgs, quirks=None):
    return b"".join(message(m, (quirks or {}).get(i)) for i, m in enumerate(msgs))


# ---- one message of each row of the table ------------------------------------------------------------
def base_state():
    """Ids 1 (two streams, keeps last), 2 (one stream, no last), 3 (no streams, keeps last); requests
    /p/a (alive, channels 0 and 3), /p/dead (receiver gone), /p/stop (STOP_COLLECTING_LAST)."""
    return rm.State(
        {1: rm.Sub(101, [0, 1], ("u", 0)), 2: rm.Sub(102, [2], None), 3: rm.Sub(103, [], ("u", 0))},
        {b"/p/a": rm.Req(201, [(0, 0), (0, 3), (0, 0)]), b"/p/dead": rm.Req(202, [(0, 1)], alive=False),
         b"/p/stop": rm.Req(203, [(rm.STOP_COLLECTING_LAST, 2)])})


# slots of base_state, as tables_of numbers them: 0-2 the subscriptions of Ids 1-3, then the
# requests by path: 3 /p/a (q 0), 4 /p/dead (q 1), 5 /p/stop (q 2)
# (name, messages, expected fields of the one call, by hand)
HAND = [
    ("update_subscribed", [("upd", 1)],
     dict(outcome=[], chan=[[(101, 0)], [(101, 0)], [], []], last_row=[1, 0, 0, 0, 0, 0], reply=b"",
          n_unmatched=0, stopped=0)),
    ("update_no_last", [("upd", 2)],
     dict(chan=[[], [], [(102, 0)], []], last_row=[0, 0, 0, 0, 0, 0], reply=b"")),
    ("update_not_subscribed", [("upd", 5), ("upd", 300)],
     dict(chan=[[], [], [], []], reply=bytes([3, 1, 5, 4, 1, 0xAC, 2]), n_replies=2, n_unmatched=2)),
    ("heartbeat", [("hb",)], dict(outcome=[rm.NONE], span_q=[rm.NO_ID], span_id=[rm.NO_ID], reply=b"")),
    ("write_result", [("wr", 1, 77)], dict(outcome=[rm.WRITE_RESULT], span_id=[rm.NO_ID])),
    ("no_such_value_pending", [("nsv", b"/p/a")], dict(outcome=[rm.FAILED], span_q=[0])),
    ("denied_pending", [("den", b"/p/dead")], dict(outcome=[rm.FAILED], span_q=[1])),
    ("no_such_value_otherwise", [("nsv", b"/p/none")], dict(outcome=[rm.NONE], span_q=[rm.NO_ID])),
    ("unsubscribed_subscribed", [("unsub", 1)],
     dict(outcome=[rm.UNSUBSCRIBED], span_id=[1], chan=[[(101, S | 0)], [(101, S | 0)], [], []],
          unsub=[(1, 0)], last_row=[0] * 6)),
    ("unsubscribed_otherwise", [("unsub", 5)], dict(outcome=[rm.NONE], span_id=[5], unsub=[])),
    ("subscribed_orphan", [("sub", b"/p/none", 6)],
     dict(outcome=[rm.ORPHAN], span_q=[rm.NO_ID], span_id=[6], reply=bytes([3, 1, 6]), sub=[])),
    ("subscribed_dropped", [("sub", b"/p/dead", 6)],
     dict(outcome=[rm.DROPPED], span_q=[1], span_id=[6], reply=bytes([3, 1, 6]), sub=[])),
    ("subscribed", [("sub", b"/p/a", 6), ("upd", 6)],
     dict(outcome=[rm.SUBSCRIBED], span_q=[0], span_id=[6], reply=b"", sub=[(0, 0, 6)],
          chan=[[(201, 0)], [], [], [(201, 0)]], last_row=[0, 0, 0, 1, 0, 0])),
    ("subscribed_stop_collecting", [("sub", b"/p/stop", 7), ("upd", 7)],
     dict(outcome=[rm.SUBSCRIBED], chan=[[], [], [(203, 0)], []], last_row=[0] * 6)),
    ("alias_is_the_hosts", [("hb",), ("sub", b"/p/a", 1), ("upd", 1)],
     dict(outcome=[rm.NONE], stopped=2, next_ctl=1, next_row=0, chan=[[], [], [], []])),
    ("id_outside_the_table_is_the_hosts", [("sub", b"/p/a", 12)],
     dict(outcome=[], stopped=2, next_ctl=0)),
    ("orphan_outside_the_table", [("sub", b"/p/none", 12)], dict(outcome=[rm.ORPHAN], stopped=0)),
    ("path_not_plain_is_the_hosts", [("upd", 1), ("den", b"/p//a"), ("upd", 1)],
     dict(outcome=[], stopped=2, next_ctl=0, next_row=1, chan=[[(101, 0)], [(101, 0)], [], []])),
    ("id_named_twice", [("unsub", 1), ("upd", 1), ("unsub", 1)],
     dict(outcome=[rm.UNSUBSCRIBED], stopped=1, next_ctl=1, next_row=1,
          reply=bytes([3, 1, 1]), n_unmatched=1)),
]


def hand_cases():
    return [(name, base_state(), msgs, N_IDS, N_CHANS, want) for name, msgs, want in HAND]


# ---- crafted sequences -------------------------------------------------------------------------------
def crafted_cases():
    """(name, State, messages, n_ids, n_chans, quirks)."""
    out = []
    add = lambda name, st, msgs, quirks=None, n_ids=N_IDS, n_chans=N_CHANS: out.append(
        (name, st, msgs, n_ids, n_chans, quirks or {}))
    add("update_around_its_unsubscribed", base_state(),
        [("upd", 1), ("unsub", 1), ("upd", 1), ("upd", 2), ("unsub", 2), ("unsub", 3), ("upd", 2)])
    add("update_after_its_subscribed", base_state(),
        [("upd", 6), ("sub", b"/p/a", 6), ("upd", 6), ("upd", 6)])
    add("unsubscribed_then_subscribed", base_state(),
        [("unsub", 1), ("upd", 1), ("sub", b"/p/a", 1), ("upd", 1), ("unsub", 1), ("upd", 1)])
    add("dropped_then_updates", base_state(), [("sub", b"/p/dead", 6), ("upd", 6), ("upd", 6)])
    add("alias_and_not_plain", base_state(),
        [("upd", 1), ("sub", b"/p/a", 1), ("upd", 1), ("nsv", b"/p/dead\\"), ("sub", b"/p//x", 4),
         ("upd", 4), ("sub", b"/p/stop", 12), ("upd", 12)])
    add("failed_then_orphan", base_state(),
        [("nsv", b"/p/a"), ("sub", b"/p/a", 6), ("upd", 6), ("den", b"/p/a")])
    add("subscribed_then_subscribed", base_state(),
        [("sub", b"/p/a", 6), ("sub", b"/p/a", 7), ("upd", 6), ("upd", 7)])
    add("wide_ids", base_state(),
        [m for i in WIDE_IDS for m in (("upd", i), ("unsub", i), ("sub", b"/p/none", i))])
    add("quirks", base_state(),
        [("unsub", 1), ("upd", 1), ("sub", b"/p/a", 6), ("upd", 6), ("unsub", 2), ("sub", b"/p/dead", 5)],
        {0: "noncanon", 2: "trailing", 4: "trailing", 5: "noncanon"})
    # paths of every length the hash and the prefixes care about; two pending paths with one hash
    (a, b), (c, d) = pc.plain_collision_pairs()[:2]
    paths = [path_of_length(n) for n in PATH_LENGTHS] + [a, b, c]
    st = rm.State({}, {p: rm.Req(300 + i, [(0, i % N_CHANS)]) for i, p in enumerate(paths)})
    msgs = []
    for i, p in enumerate(paths):
        msgs += [("sub", p, i), ("upd", i)] if i % 3 else [("den", p), ("sub", p, i), ("upd", i)]
    msgs += [("sub", d, 20), ("nsv", d)]  # the colliding path that is not pending
    add("path_lengths_and_collisions", st, msgs, n_ids=32)
    add("wide_streams", rm.State(
        {0: rm.Sub(100, [], ("u", 0)), 1: rm.Sub(101, [0], None), 2: rm.Sub(102, [3, 1, 0, 2, 3], ("u", 0)),
         3: rm.Sub(103, [1, 1], ("u", 0))},
        {b"/w": rm.Req(104, [(0, c) for c in (0, 1, 2, 3, 0, 1)])}),
        [("upd", i % 4) for i in range(10)] + [("sub", b"/w", 5), ("upd", 5), ("unsub", 2), ("unsub", 3),
                                               ("upd", 2)])
    add("no_channels", rm.State({1: rm.Sub(101, [], ("u", 0))}, {b"/z": rm.Req(102, [])}),
        [("upd", 1), ("sub", b"/z", 2), ("upd", 2), ("unsub", 1), ("upd", 1)], n_chans=0)
    add("spans_only", base_state(), [("hb",), ("unsub", 1), ("wr", 1, 2), ("sub", b"/p/a", 6)])
    add("rows_only", base_state(), [("upd", i % 7) for i in range(9)])
    add("empty", base_state(), [])
    return out


# ---- seeded batches of chosen sizes ------------------------------------------------------------------
def random_case(n_rows, n_spans, seed, n_live=24, n_pend=24, n_chans=5, once=False):
    """n_rows Updates and n_spans control messages, interleaved at random, over n_live
    subscriptions and n_pend requests. once: no Id is named by two Unsubscribed / Subscribed spans
    and no message is the host's, so one call takes the whole batch."""
    rng = random.Random(seed * 1000003 + n_rows * 1009 + n_spans)
    n_ids = n_live + n_pend + 16
    subs = {}
    for i in range(n_live):
        ns = rng.choice([0, 1, 1, 2, 3, 6])
        subs[i] = rm.Sub(1000 + i, [rng.randrange(n_chans) for _ in range(ns)],
                         ("u", 0) if rng.random() < 0.8 else None)
    pend = {}
    for q in range(n_pend):
        flags = lambda: rng.choice([0, 0, 0, rm.STOP_COLLECTING_LAST, rm.NO_SPURIOUS])
        pend[b"/r/%d/y%s" % (q, b"x" * rng.randrange(0, 20))] = rm.Req(
            2000 + q, [(flags(), rng.randrange(n_chans)) for _ in range(rng.choice([0, 1, 2, 5]))],
            alive=rng.random() < 0.85)
    paths = list(pend)
    absent = [b"/none/%d" % i for i in range(4)]
    fresh = list(range(n_live, n_live + n_pend))  # Ids the publisher hands to new subscriptions
    named = set()
    kinds = ["upd"] * n_rows + ["ctl"] * n_spans
    rng.shuffle(kinds)

    def any_id():
        return rng.choice([rng.randrange(n_live), rng.randrange(n_ids), rng.choice(fresh),
                           rng.choice(WIDE_IDS)])

    def unnamed(pool):
        for _ in range(8):
            i = pool()
            if not once or i not in named:
                named.add(i)
                return i
        return None

    msgs = []
    for kd in kinds:
        if kd == "upd":
            msgs.append(("upd", any_id()))
            continue
        x = rng.random()
        m = ("hb",)
        if 0.15 <= x < 0.25:
            m = ("wr", any_id(), rng.randrange(2**20))
        elif x < 0.40:
            m = (rng.choice(["nsv", "den"]), rng.choice(paths + absent))
        elif x < 0.60:
            i = unnamed(any_id)
            m = ("unsub", i) if i is not None else m
        elif x < 0.95 or once:
            # a live Id here is an alias, unless the batch unsubscribed it first
            i = unnamed((lambda: rng.choice(fresh)) if once or rng.random() < 0.8 else any_id)
            if i is not None:
                m = ("sub", rng.choice(paths + absent) if i < n_ids else rng.choice(absent), i)
        else:
            m = rng.choice([("sub", rng.choice(paths) + b"/", rng.choice(fresh)),
                            ("nsv", b"/r//%d" % rng.randrange(9)),
                            ("sub", rng.choice(paths), n_ids + rng.randrange(4))])
        msgs.append(m)
    name = "random_%d_%d_%d%s" % (n_rows, n_spans, seed, "_once" if once else "")
    return (name, rm.State(subs, pend), msgs, n_ids, n_chans, {})


# spans and rows at 1, around a wave and a block of the scans (kRwBlock 256) and past two blocks;
# rows also at the dispatch's 128-row segment edge
SIZES = [(1, 1), (63, 64), (64, 65), (65, 63), (255, 257), (256, 256), (257, 255), (513, 513),
         (127, 9), (128, 9), (129, 9), (0, 513), (513, 0), (1, 0), (0, 1)]


def sized_cases():
    """One call each (once=True): the sizes reach every block and segment edge of the kernels."""
    return [random_case(r, k, 7, n_live=max(24, k // 3), n_pend=max(24, k // 3), once=True)
            for r, k in SIZES]


def random_cases():
    return [random_case(r, k, seed) for seed, (r, k) in
            enumerate([(40, 40), (10, 90), (90, 10), (200, 120), (33, 300), (300, 33)])]
