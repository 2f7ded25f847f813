"""GPU tests of nxg_route_subscribes on crafted keys and on failures, against the Python model
(tests/subscribe_route_model.py) at the bar of test_gpu_subscribe_route.check_run: every output
equal to the model's. The keys come from tests/path_table_cases.py: plain paths with one hash, and
the plain-check sweep with each defect at every position around the 8-byte words. Also here: paths
placed around the edge of a workgroup's LDS staging window, one PathTable kept and changed between
calls, and current values that cannot be encoded."""
import os
import re

import numpy as np
import pytest

import path_table_cases as pc
import subscribe_route_model as sm
import to_twin as tw
from test_gpu_path_table import Model
from test_gpu_subscribe_route import BLOCK, F64_1, check_run, codec, decode  # noqa: F401

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "netidx_amd", "csrc")


def k_stage():
    """kStage of nxg_route_subscribes.hip: the bytes of a workgroup's spans staged in LDS."""
    with open(os.path.join(CSRC, "nxg_route_subscribes.hip")) as f:
        m = re.search(r"constexpr uint32_t kStage = (\d+) \* (\d+);", f.read())
    if m is None:
        raise RuntimeError("nxg_route_subscribes.hip: kStage is no longer stated as a product; "
                           "re-read stage_spans() and LSrc::word against the window tests")
    return int(m.group(1)) * int(m.group(2))


def subs(paths):
    return [("sub", p, None) for p in paths]


def path_pos(wire, off):
    """Where the path of the Subscribe at wire[off:] starts: behind varint(L), the variant byte
    and varint(|p|)."""
    p = off
    while wire[p] & 0x80:
        p += 1
    p += 2
    while wire[p] & 0x80:
        p += 1
    return p + 1


# ---- paths with one hash, compared through LDS ----------------------------------------------------
@pytest.mark.parametrize("g", range(2))
def test_a_subscribe_to_the_hash_partner_of_a_published_path(codec, g):
    a, b = pc.plain_collision_pairs()[g]
    only_a = sm.State({a: 1}, {1: F64_1, 2: (12, b"bee")})
    want, _ = check_run(codec, only_a, subs([b, a, b]), want_stop=0)
    assert want.outcome == [1, 0, 1]                   # NoSuchValue for the partner
    dflt = sm.State({a: 1}, {1: F64_1}, default=[b[:3]])
    want, _ = check_run(codec, dflt, subs([b, a]), want_stop=0)
    assert want.outcome == [3, 0]                      # ... or deferred under a matching default
    both = sm.State({a: 1, b: 2}, {1: F64_1, 2: (12, b"bee")})
    want, _ = check_run(codec, both, subs([b, a]), want_stop=0)
    assert want.outcome == [0, 0] and want.span_id == [2, 1]
    # the pair in spans 0 and 256: different workgroups, different staging windows
    fill = [b"/fill/%03d" % i for i in range(BLOCK + 3)]
    items = subs([a] + fill[:BLOCK - 1] + [b] + fill[BLOCK - 1:])
    assert items[0][1] == a and items[BLOCK][1] == b
    for st, o in ((only_a, [0, 1]), (both, [0, 0])):
        st = sm.State({**st.by_path, fill[7]: 2}, st.by_id)
        want, _ = check_run(codec, st, items, want_stop=0)
        assert [want.outcome[0], want.outcome[BLOCK]] == o and want.outcome[8] == 0


# ---- the plain check, each defect at every position -----------------------------------------------
def test_the_plain_sweep_stops_at_every_path_that_is_not_plain(codec):
    sw = pc.sweep()
    items = subs([p for p, _ in sw])
    # every third clean path is published, the next falls under a default base, the third under none
    clean = [pc.clean_path(n) for n in pc.SWEEP_LENGTHS]
    st = sm.State({p: i for i, p in enumerate(clean) if i % 3 == 0},
                  {i: (9, i) if i % 2 else (12, b"v%d" % i) for i in range(len(clean))},
                  default=[p[:2] for i, p in enumerate(clean) if i % 3 == 1])
    decoded = decode(codec, items)
    frame, cols, _ = decoded
    wire = frame.cpu().numpy().tobytes()
    off = cols.t["ctl_off"][:len(items)].cpu().numpy()
    starts = {(frame.data_ptr() + path_pos(wire, int(o))) % 8 for o in off}
    assert starts == set(range(8))                      # paths start at every address modulo 8
    tab = sm_table(codec, st)
    stops, ctl, seen = [], 0, []
    while True:
        want, r = check_run(codec, st, items, ctl_begin=ctl, tab=tab, decoded=decoded)
        seen += want.outcome
        if r.stopped != 2:
            break
        stops.append(r.next_ctl)                        # the host handles that one; resume behind
        ctl = r.next_ctl + 1
    assert r.stopped == 0 and r.next_ctl == len(sw)
    assert stops == [k for k, (_, plain) in enumerate(sw) if not plain]
    assert len(seen) == len(sw) - len(stops) and all(seen.count(o) > 3 for o in (0, 1, 3))


def sm_table(codec, st, n_ids=None):
    from netidx_amd.codec import SubscribeTable
    return SubscribeTable.from_state(codec, st.by_path, st.by_id, n_ids=n_ids,
                                     denied_ids=st.denied_ids, defaults=st.default,
                                     deferred_room=sm.MAX_DEFERRED - st.deferred_len)


# ---- the edge of the staging window ---------------------------------------------------------------
PROBE_LEN = 20
# the probe path's first byte, relative to the byte one past the window
EDGE_STARTS = {"ends at the edge": -PROBE_LEN, "crosses by 1": 1 - PROBE_LEN,
               "crosses by 7": 7 - PROBE_LEN, "crosses by 8": 8 - PROBE_LEN,
               "crosses by 9": 9 - PROBE_LEN, "starts at the edge": 0, "starts 1 before": -1,
               "starts 8 after": 8}


@pytest.mark.parametrize("where", list(EDGE_STARTS))
def test_a_path_at_the_edge_of_the_staging_window(codec, where):
    stage = k_stage()
    fillers = [b"/fill/%03d/" % i + b"x" * 390 for i in range(60)]
    pre = b"".join(tw.subscribe(p, timestamp=n, permissions=n & 0xFF, token=b"tok")
                   for n, p in enumerate(fillers[:56]))
    in_table = b"/tabl/" + b"t" * (PROBE_LEN - 6)
    probes = {"in the table": (in_table, 0), "under a default base": (b"/dflt/" + b"d" * 14, 3),
              "a miss in the last byte": (in_table[:-1] + b"u", 1)}
    st = sm.State({in_table: 5, fillers[3]: 6, fillers[58]: 7}, {5: (12, b"across"), 6: F64_1,
                                                                 7: F64_1}, default=[b"/dflt"])
    for kind, (probe, outcome) in probes.items():
        assert len(probe) == PROBE_LEN
        # the pad span's path length puts the probe's path (3 bytes into its message) in place
        target = stage + EDGE_STARTS[where] - 3
        pads = [n for n in range(130, 900) if len(pre) + len(
            tw.subscribe(b"/pad/" + b"p" * n, timestamp=56, permissions=56, token=b"tok")) == target]
        assert len(pads) == 1, (where, len(pre), target)
        items = subs(fillers[:56] + [b"/pad/" + b"p" * pads[0], probe] + fillers[56:])
        decoded = decode(codec, items)
        frame, cols, _ = decoded
        off = cols.t["ctl_off"][:len(items)].cpu().numpy()
        wire = frame.cpu().numpy().tobytes()
        a0 = (frame.data_ptr() + int(off[0])) & ~7      # the window of the one workgroup
        at = frame.data_ptr() + path_pos(wire, int(off[57]))
        assert at - (a0 + stage) == EDGE_STARTS[where] and wire[path_pos(wire, int(off[57])):][
            :PROBE_LEN] == probe
        assert len(wire) > stage + 1000                 # the window is cut at kStage
        want, _ = check_run(codec, st, items, want_stop=0, decoded=decoded)
        assert want.outcome[57] == outcome and want.outcome[3] == 0 and want.outcome[59 + 1] == 0, kind


# ---- one table, changed between calls -------------------------------------------------------------
def test_a_long_lived_table_routes_after_every_change(codec):
    from netidx_amd.codec import PathTable, SubscribeTable
    (a, b), (c, d) = pc.plain_collision_pairs()[:2]
    last, before = pc.wrap_paths(128)
    paths = [a, c, d] + list(last) + list(before) + [b"/live/%02d" % i for i in range(20)]
    st = sm.State({p: i for i, p in enumerate(paths)},
                  {i: (9, i) if i % 3 else (12, b"text%d" % i) for i in range(64)},
                  default=[b"/live/0"], denied_ids={4, 11})
    pt, m = PathTable(codec, 64, 1 << 14), Model(64, 1 << 14)
    assert pt.insert(paths, list(range(len(paths)))) == m.insert(paths, list(range(len(paths)))) == 0
    pub = sm_table(codec, sm.State({}, st.by_id, denied_ids=st.denied_ids), n_ids=64)
    tab = SubscribeTable(pt, pub.pub, pub.allow_of_id.cpu().numpy(), st.default,
                         max_value_len=pub.max_value_len)
    asked = paths + [b, b"/live/0x", b"/live/77", b"/none"]
    items = subs(asked + asked[::-1])
    decoded = decode(codec, items)

    def route():
        assert m.d == st.by_path and len(pt) == len(m.d)
        want, _ = check_run(codec, st, items, want_stop=0, tab=tab, decoded=decoded)
        return dict(zip(asked, want.outcome))

    o = route()
    assert (o[a], o[b], o[c], o[d]) == (0, 1, 0, 0) and o[b"/live/0x"] == 3
    gone = [a, d, last[0], before[1], b"/live/05", b"/live/17"]
    assert pt.remove(gone) == m.remove(gone) == 0
    for p in gone:
        del st.by_path[p]
    o = route()
    assert (o[a], o[c], o[d], o[last[1]], o[last[2]], o[b"/live/05"]) == (1, 0, 1, 2, 0, 3)
    assert pt.insert([a, b], [40, 41]) == m.insert([a, b], [40, 41]) == 0  # a again, a new Id; b
    st.by_path.update({a: 40, b: 41})
    o = route()
    assert (o[a], o[b]) == (0, 0)
    for rnd in range(6):                                # tombstones pile up until a rehash
        churn = [b"/churn/%d/%02d" % (rnd, i) for i in range(64 - len(m.d))]
        assert pt.insert(churn, [50] * len(churn)) == m.insert(churn, [50] * len(churn)) == 0
        assert pt.remove(churn) == m.remove(churn) == 0
        if m.rehashes:
            break
    assert m.rehashes == 1
    route()


# ---- current values that cannot be encoded --------------------------------------------------------
UNKNOWN, NO_ROOM, DEEP = ("unknown tag", "a container past MAX_VEC, or no child columns",
                          "nested deeper than NXG_MAX_DEPTH")


def nested(n, tag):
    """A chain of n containers around one F64: Error(Error(... F64)) or [[... [F64]]]."""
    v = F64_1
    for _ in range(n):
        v = (tag, v) if tag == 22 else (tag, [v])
    return v


def raw_table(codec, by_path, rows, kids=((0, 0, 0),), no_children=False, denied=(), n_ids=None):
    """A SubscribeTable whose current values are given as columns: rows[i] = (tag, fixed, aux) of
    Id i (slot i), kids the child columns."""
    from netidx_amd.codec import PathTable, PubTable, SubscribeTable
    n = len(rows)
    pt = PathTable(codec, max(len(by_path), 1), 1 << 12)
    pt.insert(list(by_path), list(by_path.values()))
    col = lambda a, k, dt: np.array([x[k] for x in a], dtype=dt)
    ck = {} if no_children else dict(cur_ctag=col(kids, 0, np.uint8), cur_cfixed=col(kids, 1, np.uint64),
                                     cur_caux=col(kids, 2, np.uint32))
    soi = list(range(n)) if n_ids is None else list(range(n_ids)) + [0xFFFFFFFF] * (n - n_ids)
    pub = PubTable(soi, [0] * (n + 1), [], 0, col(rows, 0, np.uint8), col(rows, 1, np.uint64),
                   col(rows, 2, np.uint32), np.zeros(8, np.uint8), "cuda", **ck)
    allow = np.ones(n, np.uint8)
    allow[list(denied)] = 0
    return SubscribeTable(pt, pub, allow if denied else None, max_value_len=64)


GOOD = (9, F64_1[1], 0)
BAD = {  # name: (rows of Id 1.., kids, no_children, the cause)
    "a root of tag 17": ([(17, 0, 0)], [(0, 0, 0)], False, UNKNOWN),
    "a root of tag 28": ([(28, 0, 0)], [(0, 0, 0)], False, UNKNOWN),
    "an unknown tag in a child": ([(19, 0, 2)], [GOOD, (17, 0, 0)], False, UNKNOWN),
    "a container without child columns": ([(22, 0, 1)], None, True, NO_ROOM),
    "an Array past MAX_VEC": ([(19, 0, (1 << 27) + 1)], [GOOD], False, NO_ROOM),
}


def route_raw(codec, tab, items, decoded=None, ctl_begin=0):
    frame, cols, _ = decoded or decode(codec, items)
    return codec.route_subscribes(tab, frame, cols, 0, ctl_begin, None)


@pytest.mark.parametrize("name", list(BAD))
def test_a_current_value_that_cannot_be_encoded_fails_the_call(codec, name):
    import netidx_amd
    rows, kids, no_children, cause = BAD[name]
    by_path = {b"/good": 0, b"/bad": 1}
    tab = raw_table(codec, by_path, [GOOD] + rows, kids or [(0, 0, 0)], no_children)
    # the lowest bad span is named, with its own cause
    items = subs([b"/good", b"/none", b"/good", b"/bad", b"/good", b"/bad"])
    with pytest.raises(netidx_amd.CodecError, match=r"span 3's Id cannot be encoded \(%s\)"
                       % re.escape(cause)):
        route_raw(codec, tab, items)
    st = sm.State(by_path, {0: F64_1, 1: F64_1})
    # behind the stop it does not matter: a path that is not plain, or an Unsubscribe, in front
    for stopper, stop in ((("sub", b"/a//b", None), 2), (("unsub", 1), 1)):
        items = subs([b"/good", b"/good"]) + [stopper] + subs([b"/bad", b"/good"])
        want, r = check_run(codec, st, items, want_stop=stop, tab=tab)
        assert r.next_ctl == 2 and want.outcome == [0, 0]
        with pytest.raises(netidx_amd.CodecError, match=r"span 3's Id cannot be encoded"):
            route_raw(codec, tab, items, ctl_begin=3)
    # nor under an Id that is denied, that by_id does not have, or that nobody asks for
    items = subs([b"/good", b"/bad", b"/good"])
    denied = raw_table(codec, by_path, [GOOD] + rows, kids or [(0, 0, 0)], no_children, denied=[1])
    st.denied_ids = {1}
    want, _ = check_run(codec, st, items, want_stop=0, tab=denied)
    assert want.outcome == [0, 2, 0]
    ignored = raw_table(codec, by_path, [GOOD] + rows, kids or [(0, 0, 0)], no_children, n_ids=1)
    want, _ = check_run(codec, sm.State(by_path, {0: F64_1}), items, want_stop=0, tab=ignored)
    assert want.outcome == [0, 4, 0]
    want, _ = check_run(codec, st, subs([b"/good", b"/none"]), want_stop=0, tab=tab)
    assert want.outcome == [0, 1]


@pytest.mark.parametrize("first,second", [("a root of tag 17", "an Array past MAX_VEC"),
                                          ("an Array past MAX_VEC", "an unknown tag in a child"),
                                          ("deep", "a root of tag 28"), ("a root of tag 28", "deep")])
def test_of_two_bad_spans_the_lower_one_is_named_with_its_own_cause(codec, first, second):
    import netidx_amd
    from netidx_amd.codec import _flatten_value
    kids, heap = [GOOD, (17, 0, 0)], bytearray()
    deep = _flatten_value(nested(40, 22), kids, heap)
    rows = {"deep": deep, "a root of tag 17": (17, 0, 0), "a root of tag 28": (28, 0, 0),
            "an Array past MAX_VEC": (19, 0, (1 << 27) + 1), "an unknown tag in a child": (19, 0, 2)}
    cause = {"deep": DEEP, **{k: v[3] for k, v in BAD.items()}}
    tab = raw_table(codec, {b"/good": 0, b"/one": 1, b"/two": 2}, [GOOD, rows[first], rows[second]],
                    kids)
    paths = [b"/good"] * (BLOCK + 60)
    paths[5], paths[300] = b"/one", b"/two"             # spans 5 and 300: two workgroups
    decoded = decode(codec, subs(paths))
    for _ in range(3):
        with pytest.raises(netidx_amd.CodecError, match=r"span 5's Id cannot be encoded \(%s\)"
                           % re.escape(cause[first])):
            route_raw(codec, tab, None, decoded)


def encoder_accepts(codec, value):
    """Whether nxg_encode_updates encodes an Update carrying `value`."""
    import netidx_amd
    from netidx_amd.codec import _flatten_value
    kids, heap = [], bytearray()
    t, f, a = _flatten_value(value, kids, heap)
    col = lambda k, dt: np.array([x[k] for x in kids], dtype=dt)
    cols = netidx_amd.columns_from_arrays(np.array([7], np.uint64), np.array([f], np.uint64),
                                          np.array([t], np.uint8), np.array([a], np.uint32),
                                          col(0, np.uint8), col(1, np.uint64), col(2, np.uint32))
    try:
        wire = codec.encode_batch(cols)
    except netidx_amd.CodecError:
        return False
    return wire.cpu().numpy().tobytes().endswith(bytes(tw.mg().enc_value(value)))


@pytest.mark.parametrize("tag", [22, 19])
def test_routing_nests_exactly_as_deep_as_the_encoder(codec, tag):
    """The deepest chain of Error(...) / of one-element Arrays around an F64 that
    nxg_encode_updates accepts, measured here, is the deepest that routing answers (with the
    model's reply bytes); one level more fails the call. Measured on the MI355X: 32 containers
    for both (the F64 at level 32 = NXG_MAX_DEPTH, the root being level 0)."""
    import netidx_amd
    ok = [n for n in range(28, 38) if encoder_accepts(codec, nested(n, tag))]
    limit = max(ok)
    print("deepest nesting the encoder accepts, tag %d: %d containers" % (tag, limit))
    assert ok == list(range(28, limit + 1)) and limit < 37
    st = sm.State({b"/deep": 3, b"/flat": 4}, {3: nested(limit, tag), 4: F64_1})
    want, _ = check_run(codec, st, subs([b"/flat", b"/deep", b"/flat"]), want_stop=0)
    assert want.outcome == [0, 0, 0]
    st.by_id[3] = nested(limit + 1, tag)
    tab = sm_table(codec, st)
    with pytest.raises(netidx_amd.CodecError, match=r"span 1's Id cannot be encoded \(%s\)"
                       % re.escape(DEEP)):
        route_raw(codec, tab, subs([b"/flat", b"/deep", b"/flat"]))
