"""Python restatement of the subscriber's ConnectionCtx::process_batch (netidx/src/subscriber/
connection.rs:409-541), unsubscribe() (:67-83) and handle_connect_stream (:321-361), line by line,
over dict state: the reference for nxg_route_replies. It is sequential, knows no stop rules and
shares no code with the library; To::Unsubscribe is built with the primitives of tests/golden/
make_golden.py (through to_twin.mg()).

Then, separately: `contract_call`, a small statement of one nxg_route_replies call as
include/nxg_codec.h words it (tables in, outputs and stops out), and `run_chained`, the host loop
that chains calls, applies their outputs to its state and handles the messages a call leaves to it.
tests/test_reply_route_cases_cpu.py proves run_chained(contract_call) == process_batch on whole
batches; the GPU test runs the same driver over the library.

Messages, decoded, as process_batch sees them (paths are bytes, taken as canonical):
  ("upd", id) | ("hb",) | ("wr", id, wid) | ("nsv", path) | ("den", path) | ("unsub", id) |
  ("sub", path, id)
"""
import to_twin as tw

NONE, WRITE_RESULT, FAILED, UNSUBSCRIBED, ORPHAN, DROPPED, SUBSCRIBED = range(7)
ALIAS, ALIAS_DROPPED = 7, 8  # the model's own: outcomes of messages a call leaves to the host
ENT_SPAN = 1 << 63
NO_ID = 2**64 - 1
NO_SLOT = 0xFFFFFFFF
BEGIN_WITH_LAST, STOP_COLLECTING_LAST, NO_SPURIOUS = 1, 2, 4  # UpdatesFlags, as the model's bits


def to_unsubscribe(id):
    """To::Unsubscribe(id): variant 1 (netproto publisher.rs:50-70)."""
    m = tw.mg()
    return m.enc_msg(1, m.enc_varint(id))


def is_plain(p):
    if len(p) == 0 or b"\\" in p or b"//" in p:
        return False
    return not p.endswith(b"/") or p == b"/"


# ---- the reference, restated ----------------------------------------------------------------------
class Sub:
    """connection.rs:54-60. last: None (not collected), ("s", span) the Subscribed's value,
    ("u", row) an Update's, or "unsub". val_alive: sub.val.upgrade() is Some."""

    def __init__(self, sub_id, streams, last, val_alive=True):
        self.sub_id, self.streams, self.last, self.val_alive = sub_id, list(streams), last, val_alive

    def copy(self):
        return Sub(self.sub_id, self.streams, self.last, self.val_alive)


class Req:
    """SubscribeValRequest: streams [(flags, chan)], alive: the `finished` receiver still listens."""

    def __init__(self, sub_id, streams, alive=True):
        self.sub_id, self.streams, self.alive = sub_id, list(streams), alive

    def copy(self):
        return Req(self.sub_id, self.streams, self.alive)


class State:
    def __init__(self, subscriptions=None, pending=None):
        self.subscriptions = {i: s.copy() for i, s in (subscriptions or {}).items()}
        self.pending = {p: r.copy() for p, r in (pending or {}).items()}

    def copy(self):
        return State(self.subscriptions, self.pending)


class Result:
    def __init__(self):
        self.by_chan = {}        # chan -> [(sub_id, row | ENT_SPAN | span)]
        self.reply = bytearray()
        self.n_replies = 0
        self.outcome = {}        # span -> outcome
        self.failed = []         # (span, sub_id of the request, variant)
        self.subscribed = []     # (span, sub_id, id)
        self.unsubscribed = []   # (span, id, sub_id)
        self.last = {}           # sub_id -> last, of every subscription the batch touched or left
        self.stream_batch = []   # ids whose BEGIN_WITH_LAST value the host pushes afterwards


def handle_connect_stream(st, res, id, chan, flags):
    """connection.rs:321-361 (channel gc left out: the model's channels are all open)."""
    sub = st.subscriptions.get(id)
    if sub is None:                                            # :328
        return
    already_have = chan in sub.streams                         # :329-340
    if flags & BEGIN_WITH_LAST and not (already_have and flags & NO_SPURIOUS):   # :341-343
        if sub.last is not None and sub.last != "unsub":       # :344-348
            res.stream_batch.append(id)
    if flags & STOP_COLLECTING_LAST:                           # :350-353
        sub.last = None
    if not already_have:                                       # :354-358
        sub.streams.append(chan)


def unsubscribe(st, res, sub, k):
    """connection.rs:67-83 (durable_* and `subscribed`, :84-117, are the host's bookkeeping)."""
    for chan in sub.streams:                                   # :74-80
        res.by_chan.setdefault(chan, []).append((sub.sub_id, ENT_SPAN | k))
    if sub.last is not None:                                   # :81-83
        sub.last = "unsub"
    res.last[sub.sub_id] = sub.last


def handle_message(st, res, m, row, k):
    """One turn of the loop of connection.rs:416-534. row: the Update's row; k: the span's index.
    Returns the outcome of a control message (None for an Update)."""
    def queue(msg):
        res.reply += msg
        res.n_replies += 1

    if m[0] == "upd":                                          # :419-433
        sub = st.subscriptions.get(m[1])
        if sub is not None:
            for chan in sub.streams:                           # :421-427
                res.by_chan.setdefault(chan, []).append((sub.sub_id, row))
            if sub.last is not None:                           # :428-430
                sub.last = ("u", row)
        else:
            queue(to_unsubscribe(m[1]))                        # :432
        return None
    if m[0] == "hb":                                           # :434
        return NONE
    if m[0] == "wr":                                           # :435-445: pending_writes only
        return WRITE_RESULT
    if m[0] in ("nsv", "den"):                                 # :446-455
        r = st.pending.pop(m[1], None)
        if r is None:
            return NONE
        res.failed.append((k, r.sub_id, 0 if m[0] == "nsv" else 1))
        return FAILED
    if m[0] == "unsub":                                        # :456-461
        s = st.subscriptions.pop(m[1], None)
        if s is None:
            return NONE
        unsubscribe(st, res, s, k)
        res.unsubscribed.append((k, m[1], s.sub_id))
        return UNSUBSCRIBED
    assert m[0] == "sub"                                       # :462-532
    _, path, id = m
    req = st.pending.pop(path, None)                           # :463
    if req is None:
        queue(to_unsubscribe(id))                              # :464-467
        return ORPHAN
    sub = st.subscriptions.get(id)                             # :468
    if sub is not None:
        if sub.val_alive:                                      # :469-483
            for f, c in req.streams:
                handle_connect_stream(st, res, id, c, f | BEGIN_WITH_LAST)
            return ALIAS
        return ALIAS_DROPPED                                   # :484-489
    if not req.alive:                                          # :501-505
        queue(to_unsubscribe(id))
        oc = DROPPED
    else:                                                      # :506-518
        st.subscriptions[id] = Sub(req.sub_id, [], ("s", k))
        res.subscribed.append((k, req.sub_id, id))
        oc = SUBSCRIBED
    for f, c in req.streams:                                   # :520-528
        handle_connect_stream(st, res, id, c, f | BEGIN_WITH_LAST)
    return oc


def process_batch(st, msgs):
    """connection.rs:409-541 over the whole batch. Rows and spans are numbered as the decode
    numbers them: Updates are rows, everything else is a control span."""
    res = Result()
    row = k = 0
    for m in msgs:
        if m[0] == "upd":
            handle_message(st, res, m, row, None)
            row += 1
        else:
            res.outcome[k] = handle_message(st, res, m, None, k)
            k += 1
    for s in st.subscriptions.values():
        res.last[s.sub_id] = s.last
    return res


# ---- one call, as the header words it ---------------------------------------------------------------
def split(msgs):
    """The decoded view: the rows' Ids, and per control span (ctl_row, message)."""
    ids, spans = [], []
    for m in msgs:
        if m[0] == "upd":
            ids.append(m[1])
        else:
            spans.append((len(ids), m))
    return ids, spans


def contract_call(tab, ids, spans, row_begin, ctl_begin):
    """nxg_route_replies. tab: n_ids, slot_of_id (list), slots [(sub_id, [chan], has_last)],
    n_chans, pending {path: q}, pend_slot [q], pend_alive [q] | None."""
    slot_of = lambda i: tab["slot_of_id"][i] if i < tab["n_ids"] else NO_SLOT
    n_ctl, n_rows = len(spans), len(ids)
    # where the call stops: the lowest span that is a stop, judged from the spans before it
    named_ids, named_q = set(), set()
    stop, stopped = n_ctl, 0
    for k in range(ctl_begin, n_ctl):
        m = spans[k][1]
        kind = 0
        if m[0] in ("nsv", "den", "sub") and not is_plain(m[1]):
            kind = 2
        elif m[0] in ("unsub", "sub"):
            id = m[1] if m[0] == "unsub" else m[2]
            if id < tab["n_ids"] and id in named_ids:
                kind = 1
            elif m[0] == "sub":
                q = tab["pending"].get(m[1])
                if q is not None and q not in named_q and (id >= tab["n_ids"] or slot_of(id) != NO_SLOT):
                    kind = 2
        if kind:
            stop, stopped = k, kind
            break
        if m[0] in ("nsv", "den", "sub") and m[1] in tab["pending"]:
            named_q.add(tab["pending"][m[1]])
        if m[0] in ("unsub", "sub"):
            named_ids.add(m[1] if m[0] == "unsub" else m[2])
    row_end = spans[stop][0] if stop < n_ctl else n_rows
    out = {"outcome": [], "span_q": [], "span_id": [], "chan": [[] for _ in range(tab["n_chans"])],
           "last_row": [0] * len(tab["slots"]), "sub": [], "unsub": [], "reply": bytearray(),
           "n_replies": 0, "n_unmatched": 0, "next_row": row_end, "next_ctl": stop,
           "stopped": stopped}
    cur = {}      # Id -> slot, where this call changed it
    taken = set()  # requests a span of this call named

    def entries(slot, ent):
        sub_id, chans, _ = tab["slots"][slot]
        for c in chans:
            if c < tab["n_chans"]:
                out["chan"][c].append((sub_id, ent))

    def reply(id):
        out["reply"] += to_unsubscribe(id)
        out["n_replies"] += 1

    k, row = ctl_begin, row_begin
    while k < stop or row < row_end:
        if k < stop and spans[k][0] <= row:
            m = spans[k][1]
            oc, q, sid = NONE, NO_ID, NO_ID
            if m[0] == "wr":
                oc = WRITE_RESULT
            elif m[0] in ("nsv", "den"):
                qq = tab["pending"].get(m[1])
                if qq is not None and qq not in taken:
                    taken.add(qq)
                    oc, q = FAILED, qq
            elif m[0] == "unsub":
                sid = m[1]
                slot = cur.get(sid, slot_of(sid))
                if slot != NO_SLOT:
                    oc = UNSUBSCRIBED
                    entries(slot, ENT_SPAN | k)
                    out["unsub"].append((sid, slot))
                    cur[sid] = NO_SLOT
            elif m[0] == "sub":
                sid = m[2]
                qq = tab["pending"].get(m[1])
                if qq is None or qq in taken:
                    oc = ORPHAN
                    reply(sid)
                else:
                    taken.add(qq)
                    q = qq
                    if tab["pend_alive"] is not None and not tab["pend_alive"][qq]:
                        oc = DROPPED
                        reply(sid)
                    else:
                        oc = SUBSCRIBED
                        out["sub"].append((k, qq, sid))
                        cur[sid] = tab["pend_slot"][qq]
            out["outcome"].append(oc)
            out["span_q"].append(q)
            out["span_id"].append(sid)
            k += 1
        else:
            id = ids[row]
            slot = cur.get(id, slot_of(id))
            if slot == NO_SLOT:
                reply(id)
                out["n_unmatched"] += 1
            else:
                entries(slot, row)
                if tab["slots"][slot][2]:
                    out["last_row"][slot] = row + 1
            row += 1
    out["reply"] = bytes(out["reply"])
    return out


# ---- the host loop ------------------------------------------------------------------------------------
def tables_of(st, n_ids, n_chans):
    """The call's tables from the host's state: a slot per live subscription (by Id), then a slot
    per pending request (by path); q numbers the requests in that order. Returns (tab, the Ids of
    the subscription slots, the paths by q)."""
    n_ids = max([n_ids] + [i + 1 for i in st.subscriptions])
    slot_of_id = [NO_SLOT] * n_ids
    slots, live = [], sorted(st.subscriptions)
    for i in live:
        s = st.subscriptions[i]
        if i < n_ids:
            slot_of_id[i] = len(slots)
        slots.append((s.sub_id, list(s.streams), 1 if s.last is not None else 0))
    paths = sorted(st.pending)
    pend_slot, pend_alive = [], []
    for p in paths:
        r = st.pending[p]
        chans = []
        for _, c in r.streams:  # what the loop of :521-528 leaves in sub.streams
            if c not in chans:
                chans.append(c)
        pend_slot.append(len(slots))
        pend_alive.append(1 if r.alive else 0)
        slots.append((r.sub_id, chans,
                      0 if any(f & STOP_COLLECTING_LAST for f, _ in r.streams) else 1))
    tab = {"n_ids": n_ids, "slot_of_id": slot_of_id, "slots": slots, "n_chans": n_chans,
           "pending": {p: q for q, p in enumerate(paths)}, "pend_slot": pend_slot,
           "pend_alive": pend_alive}
    return tab, live, paths


def run_chained(st, msgs, call, n_ids, n_chans, log=None):
    """process_batch through calls: `call(tab, ids, spans, row_begin, ctl_begin)` answers as
    contract_call does. Applies every call's outputs to `st`, handles what a call leaves to the
    host with handle_message, and returns a Result comparable with process_batch's. log: a list
    that receives (stopped, outcomes) per call."""
    ids, spans = split(msgs)
    res = Result()
    row = k = 0
    while True:
        tab, live, paths = tables_of(st, n_ids, n_chans)
        out = call(tab, ids, spans, row, k)
        if log is not None:
            log.append((out["stopped"], list(out["outcome"])))
        assert len(out["outcome"]) == out["next_ctl"] - k
        for c, ents in enumerate(out["chan"]):
            if ents:
                res.by_chan.setdefault(c, []).extend(ents)
        res.reply += out["reply"]
        res.n_replies += out["n_replies"]
        for j, oc in enumerate(out["outcome"]):
            res.outcome[k + j] = oc
            m = spans[k + j][1]
            if oc == FAILED:
                r = st.pending.pop(paths[out["span_q"][j]])
                res.failed.append((k + j, r.sub_id, 0 if m[0] == "nsv" else 1))
            elif oc == DROPPED:
                st.pending.pop(paths[out["span_q"][j]])
        new = {}
        for (sk, q, id) in out["sub"]:
            # the host's share of :506-528: the subscription, then the request's streams; what
            # that leaves is what the request's slot promised
            r = st.pending.pop(paths[q])
            slot = tab["pend_slot"][q]
            st.subscriptions[id] = s = Sub(r.sub_id, [], ("s", sk))
            for f, c in r.streams:
                handle_connect_stream(st, res, id, c, f | BEGIN_WITH_LAST)
            assert (s.sub_id, s.streams, 1 if s.last is not None else 0) == tab["slots"][slot]
            new[slot] = s
            res.subscribed.append((sk, s.sub_id, id))
        unsub_spans = [k + j for j, oc in enumerate(out["outcome"]) if oc == UNSUBSCRIBED]
        assert len(unsub_spans) == len(out["unsub"])
        gone = {slot: st.subscriptions.pop(id) for (id, slot) in out["unsub"]}
        for slot, lr in enumerate(out["last_row"]):
            if lr:
                s = gone.get(slot) or new.get(slot) or st.subscriptions[live[slot]]
                s.last = ("u", lr - 1)
        for sk, (id, slot) in zip(unsub_spans, out["unsub"]):
            s = gone[slot]
            if s.last is not None:                             # :81-83, from unsub_slot[]
                s.last = "unsub"
            res.last[s.sub_id] = s.last
            res.unsubscribed.append((sk, id, s.sub_id))
        row, k = out["next_row"], out["next_ctl"]
        if out["stopped"] == 0:
            assert k == len(spans) and row == len(ids)
            break
        if out["stopped"] == 2:  # the host's message
            res.outcome[k] = handle_message(st, res, spans[k][1], None, k)
            k += 1
    for s in st.subscriptions.values():
        res.last[s.sub_id] = s.last
    return res


def same(a, b):
    """Every field of two Results that process_batch defines, compared; returns the differing names."""
    bad = []
    for f in ("by_chan", "outcome", "failed", "subscribed", "unsubscribed", "last", "n_replies"):
        if getattr(a, f) != getattr(b, f):
            bad.append(f)
    if bytes(a.reply) != bytes(b.reply):
        bad.append("reply")
    if sorted(a.stream_batch) != sorted(b.stream_batch):
        bad.append("stream_batch")
    return bad
