"""Python restatement of the publisher's subscribe path: the `Subscribe` arm of
ClientCtx::handle_batch_inner (netidx/src/publisher/server.rs:506-549) and subscribe()
(server.rs:60-137), line by line, over dict state. The reference for nxg_route_subscribes; replies
are built with the primitives of tests/golden/make_golden.py (through to_twin.mg()) and nothing
here shares code with the library.

A Subscribe is given decoded, as handle_batch_inner sees it: its path (bytes, already canonical:
Path::decode canonises, and the device decides plain paths only, which are canonical as they
stand) and what the host made of its token: None for DesiredAuth::Anonymous, DENY for "no stored
secret" and "token invalid" (server.rs:520-535), else the permission bits check_token returned.
"""
import bisect

import to_twin as tw

ALL = 0x3F          # Permissions::all() (resolver_server/auth.rs:24-29)
DENY = 0xFFFFFFFF   # NXG_SUB_PERM_DENY
MAX_DEFERRED = 1000000  # server.rs:56
SUBSCRIBED, NO_SUCH_VALUE, DENIED, DEFERRED, IGNORED = 0, 1, 2, 3, 4


def _path(p):
    m = tw.mg()
    return m.enc_varint(len(p)) + p


def no_such_value(path):
    """From::NoSuchValue(path): variant 0 (netproto publisher.rs:83-99)."""
    return tw.mg().enc_msg(0, _path(path))


def denied(path):
    """From::Denied(path): variant 1."""
    return tw.mg().enc_msg(1, _path(path))


def subscribed(path, id, value):
    """From::Subscribed(path, id, value): variant 3."""
    m = tw.mg()
    return m.enc_msg(3, _path(path) + m.enc_varint(id) + m.enc_value(value))


def is_plain(p):
    """The paths the device decides: no `\\`, not empty, no `//`, no trailing `/` unless `/`."""
    if len(p) == 0 or b"\\" in p or b"//" in p:
        return False
    return not p.endswith(b"/") or p == b"/"


class State:
    """What subscribe() reads and changes: t.by_path, t.by_id (Id -> current value), t.default
    (the bases of the default publishers whose channel is open, as sorted keys: the `continue` on
    a closed channel, server.rs:81, is the host's), deferred_subs.inner().len(), extended_auth as
    the set of Ids it denies this client (None: no extended_auth) and cl.subscribed."""

    def __init__(self, by_path, by_id, default=(), deferred_len=0, denied_ids=None,
                 subscribed=None):
        self.by_path = dict(by_path)
        self.by_id = dict(by_id)
        self.default = sorted(set(default))
        self.deferred_len = deferred_len
        self.denied_ids = None if denied_ids is None else set(denied_ids)
        self.subscribed = {} if subscribed is None else dict(subscribed)

    def copy(self):
        return State(self.by_path, self.by_id, self.default, self.deferred_len, self.denied_ids,
                     self.subscribed)


class Result:
    def __init__(self):
        self.outcome = []   # per Subscribe, in span order
        self.span_id = []   # the Id its path resolves to, or None
        self.sub = []       # cl.subscribed.insert(id, permissions), in order
        self.deferred = []  # span indices handed to a default publisher
        self.reply = bytearray()
        self.n_replies = 0


def subscribe(st, res, k, path, permissions):
    """server.rs:60-137; returns the outcome."""
    def queue(msg):
        res.reply += msg
        res.n_replies += 1

    id = st.by_path.get(path)                         # server.rs:68
    res.span_id.append(id)
    if id is None:
        # t.default.range_mut((Unbounded, Included(path))).next_back(): the greatest base <= path;
        # the loop's second turn is reached only through the closed-channel `continue`
        i = bisect.bisect_right(st.default, path)     # server.rs:70-75
        if i > 0 and path.startswith(st.default[i - 1]) and st.deferred_len < MAX_DEFERRED:
            st.deferred_len += 1                      # server.rs:76-86
            res.deferred.append(k)
            return DEFERRED
        queue(no_such_value(path))                    # server.rs:88-91
        return NO_SUCH_VALUE
    if id not in st.by_id:                            # server.rs:97
        return IGNORED
    if st.denied_ids is not None and id in st.denied_ids:  # server.rs:98-106
        queue(denied(path))
        return DENIED
    st.subscribed[id] = permissions                   # server.rs:108-110
    res.sub.append((id, permissions))
    queue(subscribed(path, id, st.by_id[id]))         # server.rs:125-126
    return SUBSCRIBED


def handle_subscribe(st, res, k, path, span_perm):
    """The Subscribe arm, server.rs:506-549."""
    if span_perm is None:                             # DesiredAuth::Anonymous
        res.outcome.append(subscribe(st, res, k, path, ALL))
    elif span_perm == DENY:                           # no stored secret / token invalid
        res.span_id.append(None)
        res.reply += denied(path)
        res.n_replies += 1
        res.outcome.append(DENIED)
    else:
        res.outcome.append(subscribe(st, res, k, path, span_perm))


def route(st, paths, span_perm=None, k0=0):
    """A run of Subscribes: paths[j] is span k0 + j. Stops in front of the first path that is not
    plain. Returns (Result, the number of spans handled)."""
    res = Result()
    for j, p in enumerate(paths):
        if not is_plain(p):
            return res, j
        handle_subscribe(st, res, k0 + j, p, None if span_perm is None else span_perm[k0 + j])
    return res, len(paths)


def on_subscribe(sst, res):
    """The hook of write_route_model.handle_batch: messages ("sub", path, k, span_perm | None).
    The write model's state `st` shares cl.subscribed with `sst` (subscribe() inserts into it)."""
    def hook(st, m):
        _, path, k, perm = m
        sst.subscribed = st.subscribed
        handle_subscribe(sst, res, k, path, perm)
    return hook
