"""GPU tests of the fast To decoder: Codec.decode_writes(fast=True) (nxg_decode_writes_opts) over
the case table of tests/writes_fast_cases.py.

Bar, for every case: the twin's (tests/to_twin.py) columns, counts, wflags, wid and control spans
bit for bit; identical arrays from fast=False (the general decoder) in the same test; the path
the case's class demands (must: 8, decline: 6, may: 6 or 8); and the guard bands behind every
capacity intact (tests/guards.py; wflags / wid carry sentinel rows of their own behind cap_rows).
Valid frames decode into columns of exactly the frame's counts, so a store one element too far
lands in a guard band. Every test takes a fresh Codec.
"""
import numpy as np
import pytest

import guards
import to_twin as tw
import writes_fast_cases as wf

pytestmark = pytest.mark.gpu

SPARE = guards.MIN_SPARE
FAST, GENERAL = 8, 6


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
    return torch.from_numpy(np.frombuffer(bytes(wire), np.uint8).copy()).cuda()


def u64(xs):
    return np.array(list(xs), dtype=np.uint64)


def outputs(n_rows, n_children, n_ctl, device="cuda"):
    """Guarded Columns and WriteCols of exactly these capacities."""
    import torch
    from netidx_amd.codec import LAYOUT_MIXED, WriteCols
    cols = guards.guarded_columns(n_rows, n_children, n_ctl, LAYOUT_MIXED, device)
    wc = WriteCols(n_rows + SPARE, device)
    wc.s.cap_rows = n_rows
    wc.guard_cap = n_rows
    wc.wflags.fill_(guards.SENTINEL)
    wc.wid.view(torch.uint8).fill_(guards.SENTINEL)
    if wc.device.type == "cuda":
        torch.cuda.synchronize()
    return cols, wc


def assert_all_guards(cols, wc):
    guards.assert_guards(cols)
    cap = wc.guard_cap
    assert (wc.wflags[cap:].cpu().numpy() == guards.SENTINEL).all(), "wflags behind cap_rows"
    tail = wc.wid[cap:].cpu().numpy().view(np.uint8)
    assert (tail == guards.SENTINEL).all(), "wid behind cap_rows"


def run(codec, wire, fast, caps, host_frame=False, host_out=False):
    cols, wc = outputs(*caps, device="cpu" if host_out else "cuda")
    frame = bytes(wire) if host_frame else dev(wire)
    codec.decode_writes(frame, cols, wc, check=False, fast=fast)
    st = codec.writes_status
    assert codec.last_status()[2] == st.path
    return cols, wc, st


def arrays(cols, wc, st):
    g = cols.numpy()
    w = wc.numpy(st.n_rows)
    out = {k: g[k] for k, _, _ in cols.FIELDS}
    out["wflags"], out["wid"] = w["wflags"], w["wid"]
    return out


def assert_twin(cols, wc, st, e):
    assert st.err_kind == 0
    assert (st.n_rows, st.n_children, st.n_ctl, st.n_heartbeat) == \
        (len(e.rows), len(e.children), len(e.ctl), 0)
    assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == \
        (len(e.rows), len(e.children), len(e.ctl))
    a = arrays(cols, wc, st)
    for k, name in enumerate(("id", "tag", "fixed", "aux")):
        assert np.array_equal(a[name].astype(np.uint64), u64(r[k] for r in e.rows)), name
    for k, name in enumerate(("ctag", "cfixed", "caux")):
        assert np.array_equal(a[name].astype(np.uint64), u64(r[k] for r in e.children)), name
    for k, name in enumerate(("ctl_row", "ctl_off", "ctl_len", "ctl_variant")):
        assert np.array_equal(a[name].astype(np.uint64), u64(r[k] for r in e.ctl)), name
    assert np.array_equal(a["wflags"].astype(np.uint64), u64(e.wflags))
    assert np.array_equal(a["wid"], u64(e.wid))
    return a


def check_valid(codec, wire, e, want_paths, **kw):
    """fast=True and fast=False into guarded columns of exactly the frame's counts: the twin's
    answer from both, identical arrays, the path, the guards."""
    caps = (len(e.rows), len(e.children), len(e.ctl))
    cf, wf_, sf = run(codec, wire, True, caps, **kw)
    assert sf.path in want_paths, (sf.path, want_paths)
    if sf.path == FAST:
        assert sf.err_kind == 0 and sf.n_children == 0
    af = assert_twin(cf, wf_, sf, e)
    assert_all_guards(cf, wf_)
    cg, wg, sg = run(codec, wire, False, caps, **kw)
    assert sg.path == GENERAL
    ag = assert_twin(cg, wg, sg, e)
    assert_all_guards(cg, wg)
    for name in af:
        assert np.array_equal(af[name], ag[name]), name
    return sf


PATHS = {"must": (FAST,), "may": (FAST, GENERAL), "decline": (GENERAL,)}
CLEAN = None


def clean():
    global CLEAN
    if CLEAN is None:
        wire = wf.seeded(300, 77)
        CLEAN = (wire, tw.decode(wire)[0])
    return CLEAN


def ids(cls):
    return [k.name for k in wf.by_class(cls)]


# ---- the table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", wf.by_class("must"), ids=ids("must"))
def test_must_take(codec, k):
    e, err = tw.decode(k.wire)
    assert err is None
    check_valid(codec, k.wire, e, PATHS["must"])


@pytest.mark.parametrize("k", wf.by_class("may"), ids=ids("may"))
def test_may_take(codec, k):
    e, err = tw.decode(k.wire)
    assert err is None
    check_valid(codec, k.wire, e, PATHS["may"])


@pytest.mark.parametrize("k", wf.by_class("decline"), ids=ids("decline"))
def test_declines_and_then_takes_a_clean_frame(codec, k):
    n = len(k.wire)
    if k.err is None:
        e, err = tw.decode(k.wire)
        assert err is None
        check_valid(codec, k.wire, e, PATHS["decline"])
    else:
        for fast in (True, False):
            cols, wc, st = run(codec, k.wire, fast, (n // 5 + 1, n + 1, n // 3 + 1))
            assert st.path == GENERAL
            assert (st.err_kind, st.err_offset) == k.err
            assert (st.n_rows, st.n_children, st.n_ctl) == (0, 0, 0)
            assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == (0, 0, 0)
            assert_all_guards(cols, wc)
    # no skip state: the next frame on the same context goes to the fast decoder
    wire, e = clean()
    check_valid(codec, wire, e, (FAST,))


# ---- 10^5 messages ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["writes", "unsubscribes", "subscribes",
                                  "writes_with_an_unsubscribe_every_100"])
def test_100k_messages(codec, name):
    wire, e = tw.batch(wf.big_frames()[name])
    check_valid(codec, wire, e, (FAST,))


# The resolve pass's last block scans the block sums 256 at a time: 65,536 tiles (256 sums, one
# round) and 65,537 (a second round that carries the running total). Such a frame is 256 MiB, far
# past what the twin decodes in seconds, so the expectation is built from the twin's decode of the
# one 127-byte Write the frame repeats: row i is that row with its text 127 i bytes further on.
@pytest.mark.parametrize("tiles", [65536, 65537])
def test_block_sums_in_one_round_and_two(codec, tiles):
    import torch
    msg = next(m for m in (wf.W(300, True, (12, b"w" * k), 2**40) for k in range(90, 121))
               if len(m) == 127)
    one = tw.decode(msg)[0]
    (i0, tag, fixed, aux), = one.rows
    n = (65536 * wf.TILE) // 127 + (1 if tiles == 65537 else 0)
    wire = np.tile(np.frombuffer(msg, np.uint8), n)
    assert (len(wire) + wf.TILE - 1) // wf.TILE == tiles
    frame = torch.from_numpy(wire).cuda()
    want = {"id": np.full(n, i0, np.uint64), "tag": np.full(n, tag, np.uint8),
            "fixed": fixed + 127 * np.arange(n, dtype=np.uint64), "aux": np.full(n, aux, np.uint32),
            "wflags": np.full(n, one.wflags[0], np.uint8), "wid": np.full(n, one.wid[0], np.uint64)}
    for fast, path in ((True, FAST), (False, GENERAL)):
        cols, wc = outputs(n, 0, 0)
        codec.decode_writes(frame, cols, wc, fast=fast)
        st = codec.writes_status
        assert (st.path, st.err_kind, st.n_rows, st.n_children, st.n_ctl) == (path, 0, n, 0, 0)
        a = arrays(cols, wc, st)
        for name, w in want.items():
            assert np.array_equal(a[name], w), (fast, name)
        assert_all_guards(cols, wc)


def test_empty_frame_launches_nothing_and_reports_the_general_path(codec):
    cols, wc = outputs(4, 4, 4)
    codec.decode_writes(b"", cols, wc, fast=True)
    st = codec.writes_status
    assert (st.path, st.err_kind, st.n_rows, st.n_ctl) == (GENERAL, 0, 0, 0)
    assert_all_guards(cols, wc)


# ---- capacity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["rows", "ctl"])
def test_capacity_exact_and_one_short(codec, short):
    from netidx_amd import CodecError
    wire = wf.seeded(700, 21)
    assert len(wire) > 2 * wf.TILE and wf.fast_must_take(wire)
    e = tw.decode(wire)[0]
    exact = {"rows": len(e.rows), "children": 0, "ctl": len(e.ctl)}
    check_valid(codec, wire, e, (FAST,))  # exactly enough room: path 8
    caps = dict(exact)
    caps[short] -= 1
    msgs = []
    for fast in (True, False):
        cols, wc = outputs(caps["rows"], caps["children"], caps["ctl"])
        with pytest.raises(CodecError, match="NXG_CAPACITY") as x:
            codec.decode_writes(dev(wire), cols, wc, fast=fast)
        msgs.append(str(x.value))
        assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == (0, 0, 0)
        assert_all_guards(cols, wc)  # nothing at or past any capacity was written
    assert msgs[0] == msgs[1]
    check_valid(codec, wire, e, (FAST,))  # and the context decodes on


# ---- memory kinds -------------------------------------------------------------------------------
@pytest.mark.parametrize("host_frame,host_out", [(True, False), (False, True), (True, True)])
def test_host_frame_and_pinned_host_columns(codec, host_frame, host_out):
    wire = wf.seeded(700, 33)
    check_valid(codec, wire, tw.decode(wire)[0], (FAST,), host_frame=host_frame,
                host_out=host_out)


# ---- through routing ----------------------------------------------------------------------------
def test_routing_is_the_same_on_fast_and_general_columns(codec, monkeypatch):
    import random
    import test_gpu_subscribe_route as R
    sm, wm = R.sm, R.wm
    rng = random.Random(4)
    paths = {b"/p%d" % i: i for i in range(1, 9)}
    items = []
    for n in range(400):
        r = rng.random()
        if r < 0.15:
            for _ in range(rng.randrange(1, 4)):
                items.append(("sub", rng.choice(list(paths) + [b"/nope"]), None))
        elif r < 0.25:
            items.append(("unsub", rng.randrange(1, 9)))
        else:
            items.append(("w", rng.randrange(1, 10), rng.random() < 0.7,
                          None if rng.random() < 0.1 else n))
    assert wf.fast_must_take(R.wire_of(items))
    paths_seen = []

    def decode_with(fast):
        def decode(c, its):
            from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
            w = R.wire_of(its)
            frame = dev(w)
            cols = Columns(len(w) // 5 + 1, len(w) + 1, len(w) // 3 + 1, LAYOUT_MIXED, "cuda")
            wcols = WriteCols(len(w) // 5 + 1, "cuda")
            c.decode_writes(frame, cols, wcols, fast=fast)
            paths_seen.append(c.writes_status.path)
            return frame, cols, wcols
        return decode

    got = []
    for fast in (True, False):
        monkeypatch.setattr(R, "decode", decode_with(fast))
        sst = sm.State(dict(paths), {i: R.F64_1 for i in paths.values()})
        wst = wm.State({}, {i: [0] for i in paths.values()})
        s, w, handled, calls = R.drive(codec, sst, wst, items, 16)
        got.append((s.outcome, s.sub, s.deferred, bytes(s.reply), w.outcome, bytes(w.reply),
                    w.unsub, handled, calls))
    assert paths_seen == [FAST, GENERAL]
    assert got[0] == got[1]
    assert len(got[0][0]) > 20 and len(got[0][4]) > 100 and got[0][8] > 10
