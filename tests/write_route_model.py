"""Python restatement of the publisher's write path: the `Write` and `Unsubscribe` arms of
ClientCtx::handle_batch_inner (netidx/src/publisher/server.rs:497-576) and write()
(server.rs:171-245), line by line, over dict state. The reference for nxg_route_writes; replies are
built with the primitives of tests/golden/make_golden.py (through to_twin.mg()) and nothing here
shares code with the library.

Messages are given decoded, as handle_batch_inner sees them:
  ("w", id, r, wid | None)   To::Write(id, r, v, wid); None: no WriteId on the wire, so the decode
                             allotted WriteId::default() = WriteId::new() (netproto publisher.rs:11-15)
  ("unsub", id)              To::Unsubscribe(id)
  ("sub", anything)          To::Subscribe: handled by the caller's `on_subscribe(state, msg)`
The Value of a Write plays no part in routing and is left out.
"""
import to_twin as tw

WRITE = 0x04  # Permissions::WRITE (resolver_server/auth.rs:26)
ROUTED, UNSUBSCRIBED, DENIED, NOT_ACCEPTED = 0, 1, 2, 3
MSG = {UNSUBSCRIBED: b"cannot write to unsubscribed value",  # server.rs:201-202
       DENIED: b"write permission denied",                    # server.rs:204
       NOT_ACCEPTED: b"writes not accepted"}                  # server.rs:206, 216


def unsubscribed(id):
    """From::Unsubscribed(id): variant 2 (netproto publisher.rs:83-99)."""
    m = tw.mg()
    return m.enc_msg(2, m.enc_varint(id))


def write_result(id, msg, wid):
    """From::WriteResult(id, Value::Error(String(msg)), wid): variant 6; Error(String) is wire
    tag 18 (netidx-value/src/lib.rs:437-441)."""
    m = tw.mg()
    return m.enc_msg(6, m.enc_varint(id) + m.enc_value((18, msg)) + m.enc_varint(wid))


class State:
    """What write() and unsubscribe() read and change for one client: cl.subscribed (None: the
    publisher does not know the client, t.clients.get(&client) is None) and t.on_write with open
    channels only (the retain of server.rs:207-214 has run; gc_on_write is the host's)."""

    def __init__(self, subscribed, on_write):
        self.subscribed = None if subscribed is None else dict(subscribed)
        self.on_write = {i: list(c) for i, c in on_write.items()}

    def copy(self):
        return State(self.subscribed, self.on_write)


class Result:
    def __init__(self):
        self.outcome = []    # per Write, in row order
        self.batches = {}    # write_batches: chan -> [(id, row)]
        self.reply = bytearray()
        self.n_replies = 0
        self.wait = []       # wait_write_res: (row, id, wid)
        self.unsub = []      # Ids handed to unsubscribe()
        self.n_fresh = 0


def write(st, res, row, id, r, wid):
    """server.rs:171-245; returns the outcome."""
    def or_qwe(outcome):  # server.rs:186-199
        if r:
            res.reply += write_result(id, MSG[outcome], wid)
            res.n_replies += 1
        return outcome

    if st.subscribed is None:              # t.clients.get(&client), server.rs:201
        return or_qwe(UNSUBSCRIBED)
    perms = st.subscribed.get(id)          # cl.subscribed.get(&id), server.rs:202
    if perms is None:
        return or_qwe(UNSUBSCRIBED)
    if not perms & WRITE:                  # server.rs:203-205
        return or_qwe(DENIED)
    ow = st.on_write.get(id)               # server.rs:206
    if ow is None:
        return or_qwe(NOT_ACCEPTED)
    if len(ow) == 0:                       # server.rs:215-217
        return or_qwe(NOT_ACCEPTED)
    if r:                                  # server.rs:218-224
        res.wait.append((row, id, wid))
    for cid in ow:                         # server.rs:225-240
        res.batches.setdefault(cid, []).append((id, row))
    return ROUTED


def handle_batch(st, msgs, fresh_wid=0, on_subscribe=None):
    """server.rs:504-568 over `msgs`; `st` is updated in place. Returns a Result."""
    res = Result()
    row = 0
    for m in msgs:
        if m[0] == "sub":
            if on_subscribe is not None:
                on_subscribe(st, m)
        elif m[0] == "w":
            _, id, r, wid = m
            if wid is None:                # allotted when the message was decoded
                wid = (fresh_wid + res.n_fresh) & tw.M64
                res.n_fresh += 1
            res.outcome.append(write(st, res, row, id, r, wid))
            row += 1
        else:                              # server.rs:562-566
            id = m[1]
            if st.subscribed is not None:  # unsubscribe(): cl.subscribed.remove(&id)
                st.subscribed.pop(id, None)
            res.unsub.append(id)
            res.reply += unsubscribed(id)
            res.n_replies += 1
    return res
