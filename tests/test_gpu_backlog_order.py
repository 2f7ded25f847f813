"""Async backlogs (nxg_decode_updates_async, nxg_decode_frames_async, nxg_encode_updates_async,
nxg_ctx_sync) against the sequential model of tests/backlog_model.py.

A call whose fast kernel declines is finished inside nxg_ctx_sync, after every later call of the
backlog has run; nxg_ctx_sync then redoes, in order, the later calls that touched the same memory
(netidx_amd/csrc/nxg_api.cpp). Which kernel declines depends on the data and on what the context
saw before (it skips a decoder or encoder that declined recently). None of that may show in the
result: a backlog leaves behind what its calls would have, run one after another -- the model,
computed with the CPU oracle from the program alone.

  - Every committed random program runs on four context states: fresh, after one declined
    synchronous decode, after one declined synchronous encode, after both.
  - An input-stable program (no call writes what an earlier call reads) must complete and equal
    the model everywhere: every buffer byte with its margin, every id / fixed column, every
    n_rows, every len_out, the returned status.
  - A hazardous program either equals the model everywhere, or nxg_ctx_sync fails with one of the
    two "keep ... unchanged until nxg_ctx_sync" errors of include/nxg_codec.h, naming a call whose
    input the model lists as written by a later call; the context then still encodes and decodes
    bit-exact. A silent difference always fails.
"""
import re

import numpy as np
import pytest

import backlog_model as bm

pytestmark = pytest.mark.gpu

STATES = ("fresh", "declined-decode", "declined-encode", "declined-both")
LOUD = re.compile(r"(?:decode|encode) of async call (\d+) needs its (?:frame|columns) again .*"
                  r"keep (?:a frame|them) unchanged until nxg_ctx_sync")

_cache = {}


def _program(key, make):
    """(program, model result), computed once and shared (never modified)."""
    if key not in _cache:
        p = make()
        _cache[key] = (p, bm.run(p))
    return _cache[key]


def _warm_data():
    """A P frame and a P batch of 300 rows: one synchronous decode / encode of them makes a
    context skip its sequential-id decoder / encoder (and checks that it still works)."""
    if "warm" not in _cache:
        import nxo
        rng = np.random.default_rng(99)
        ids, vals = bm.perm_ids(300, rng), bm.values(300, 99)
        _cache["warm"] = (ids, vals, nxo.encode_f64(ids, vals))
    return _cache["warm"]


def _plain_decode(codec):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    ids, vals, wire = _warm_data()
    cols = Columns(len(wire) // 4 + 1, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
    st = codec.decode_into(torch.from_numpy(wire.copy()).cuda(), len(wire), cols)
    g = cols.numpy()
    assert st.n_rows == len(ids) and st.err_kind == 0
    assert np.array_equal(g["id"], ids) and np.array_equal(g["fixed"], vals)
    assert codec.last_diag()[1] != 1, "the sequential-id decoder took ids out of order"


def _plain_encode(codec):
    import torch
    import netidx_amd
    ids, vals, wire = _warm_data()
    cols = netidx_amd.columns_from_arrays(ids, vals)
    out = torch.full((len(wire) + 64,), bm.SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert codec.encode_into(cols, None, out.data_ptr(), len(wire)) == len(wire)
    h = out.cpu().numpy()
    assert np.array_equal(h[:len(wire)], wire) and (h[len(wire):] == bm.SENT).all()
    assert codec.last_encode_kernel() == "tile"


def _context(state):
    import netidx_amd
    codec = netidx_amd.Codec(0)
    try:
        if state in ("declined-decode", "declined-both"):
            _plain_decode(codec)
        if state in ("declined-encode", "declined-both"):
            _plain_encode(codec)
    except BaseException:
        codec.close()
        raise
    return codec


def _run(codec, prog, res):
    """Issue the program's calls on `codec` and sync. Returns (error text or None, observed)."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    n = prog.n
    dbufs = [torch.from_numpy(b.copy()).cuda() for b in prog.buffers()]
    assert all(b.data_ptr() % 16 == 0 and b.numel() == prog.cap + bm.MARGIN for b in dbufs)
    # capacity bounds of include/nxg_codec.h for a frame of cap bytes: no bytes a call of the
    # backlog can meet in a buffer decode to more
    dcols = []
    for ids, vals in prog.cols:
        c = Columns(prog.cap // 4 + 1, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
        c.id[:n].copy_(torch.from_numpy(ids.view(np.int64)))
        c.fixed[:n].copy_(torch.from_numpy(vals.view(np.int64)))
        c.s.n_rows = n
        dcols.append(c)
    dcols.append(Columns.for_frame(prog.cap, netidx_amd.LAYOUT_MIXED, "cuda"))
    torch.cuda.synchronize()  # (the uploads ran on torch's stream, the codec has its own)
    groups = dict(prog.groups)
    lens = {}
    i = 0
    while i < len(prog.ops):
        if i in groups:
            run = range(i, groups[i])
            codec.decode_frames_async([dbufs[prog.ops[k].buf].data_ptr() for k in run],
                                      [res.d_len[k] for k in run],
                                      [dcols[prog.ops[k].cols] for k in run])
            i = groups[i]
            continue
        op = prog.ops[i]
        if op.kind == "D":
            codec.decode_async(dbufs[op.buf].data_ptr(), res.d_len[i], dcols[op.cols])
        else:
            lens[i] = codec.encode_async(dcols[op.cols], None, dbufs[op.buf].data_ptr(), prog.cap)
        i += 1
    error, st = None, None
    try:
        st = codec.sync(check=False)
    except netidx_amd.CodecError as e:
        error = str(e)
    torch.cuda.synchronize()
    got = {"bufs": [b.cpu().numpy() for b in dbufs],
           "cols": [{"n_rows": int(c.s.n_rows), "n_heartbeat": int(c.s.n_heartbeat),
                     "id": c.id.cpu().numpy().view(np.uint64),
                     "fixed": c.fixed.cpu().numpy().view(np.uint64)} for c in dcols],
           "len_out": {k: int(v.value) for k, v in lens.items()},
           "status": None if st is None else (int(st.n_rows), int(st.err_kind),
                                              int(st.n_heartbeat))}
    return error, got


def _differences(prog, res, got):
    """Every observed value that is not the model's (empty: the backlog ran in order)."""
    bad = []
    for b, (g, m) in enumerate(zip(got["bufs"], res.bufs)):
        if not np.array_equal(g, m):
            k = int(np.flatnonzero(g != m)[0])
            where = "margin" if k >= prog.cap else "frame"
            bad.append(f"buffer {b}: {int((g != m).sum())} bytes differ, first at {k} ({where})")
    for c, (g, m) in enumerate(zip(got["cols"], res.cols)):
        if g["n_rows"] != m["n_rows"] or g["n_heartbeat"] != m["n_heartbeat"]:
            bad.append(f"columns {c}: n_rows/n_heartbeat {g['n_rows']}/{g['n_heartbeat']}, "
                       f"model {m['n_rows']}/{m['n_heartbeat']}")
            continue
        k = m["n_rows"]
        for f in ("id", "fixed"):
            if not np.array_equal(g[f][:k], m[f]):
                r = int(np.flatnonzero(g[f][:k] != m[f])[0])
                bad.append(f"columns {c}: {f} differs from row {r}: {int(g[f][r])}, "
                           f"model {int(m[f][r])}")
    for i, v in got["len_out"].items():
        if v != res.len_out[i]:
            bad.append(f"call {i}: len_out {v}, model {res.len_out[i]}")
    if got["status"] != res.status:
        bad.append(f"status (n_rows, err_kind, n_heartbeat) {got['status']}, model {res.status}")
    return bad


def _check(prog, res, state, must_be_exact=None):
    """Run `prog` on a context in `state` and hold it to the model (module docstring). Returns
    "exact" or "loud"."""
    if must_be_exact is None:
        must_be_exact = res.stable
    codec = _context(state)
    try:
        error, got = _run(codec, prog, res)
        what = f"{prog.describe()} [{state}]"
        if error is None:
            bad = _differences(prog, res, got)
            assert not bad, f"{what}: silently differs from the model: " + "; ".join(bad)
            return "exact"
        assert not must_be_exact, f"{what}: must complete, but nxg_ctx_sync failed: {error}"
        m = LOUD.search(error)
        assert m, f"{what}: nxg_ctx_sync failed with another error: {error}"
        readers = sorted({i for i, _ in res.hazards})
        assert int(m.group(1)) in readers, \
            f"{what}: the error names call {m.group(1)}, the model's readers are {readers}: {error}"
        # the context stays usable
        _plain_encode(codec)
        _plain_decode(codec)
        return "loud"
    finally:
        codec.close()


@pytest.mark.parametrize("state", STATES)
def test_random_backlogs_equal_the_sequential_model(state):
    """Every committed random program (tests/backlog_model.py SEEDS), each on a context of its
    own in `state`: input-stable ones equal the model, hazardous ones equal it or fail loudly."""
    outcomes = {"exact": 0, "loud": 0}
    for seed in bm.SEEDS:
        prog, res = _program(("seed", seed), lambda: bm.generate(seed))
        outcomes[_check(prog, res, state)] += 1
    print(f"{state}: {outcomes}")
    assert outcomes["exact"] >= sum(_cache[("seed", s)][1].stable for s in bm.SEEDS)


@pytest.mark.parametrize("n", [300, 3000])
@pytest.mark.parametrize("make", [
    lambda n: bm.scenario_late_decode_shared_columns(n, "P"),
    lambda n: bm.scenario_late_decode_shared_columns(n, "H"),
    bm.scenario_late_decode_then_encode, bm.scenario_late_encode_then_decode],
    ids=["late-decode-P", "late-decode-H", "late-decode-encode", "late-encode-decode"])
def test_input_stable_hand_built_backlogs(make, n):
    """The earlier hand-built scenarios (late decode into shared columns, late decode then an
    encode of its columns, late encode then a decode of its output) at the model's sizes, on
    every context state: input-stable, so exact."""
    prog, res = _program(("stable", make, n), lambda: make(n))
    assert res.stable
    for state in STATES:
        assert _check(prog, res, state) == "exact"


@pytest.mark.parametrize("n", [300, 3000])
def test_write_after_write_on_an_encode_output(n):
    """encode(c1 -> X) with permuted ids, decode(X -> d1), encode(c2 -> X) with sequential ids,
    decode(X -> d2). The first encode is done again on the tiled encoder at sync and puts c1's
    frame back into X after the second encode wrote c2's; the second encode must be done again
    too (its output was overwritten), or d2 gets c1's rows and X is left holding c1's frame while
    the second encode reports success. On a context that skips the sequential-id decoder no
    decode falls back, nothing needs bytes that are gone, and the result must be exact. On the
    other states: exact, or the loud error naming the first decode (whose frame the second
    encode writes)."""
    prog, res = _program(("waw", n), lambda: bm.scenario_write_after_write(n))
    assert res.hazards == [(1, 2)]
    assert _check(prog, res, "declined-decode", must_be_exact=True) == "exact"
    for state in ("fresh", "declined-encode", "declined-both"):
        _check(prog, res, state)


@pytest.mark.parametrize("n", [300, 3000])
def test_redone_decode_does_not_read_an_overwritten_frame(n):
    """decode(F0 -> C) of a P frame (falls back at sync on a fresh context), decode(F1 -> C) that
    the fast path accepts, encode(K -> F1) that the sequential-id encoder accepts. The fallback
    rewrites C, so the second decode has to be done again -- from F1, which by then holds the
    encode's output. Exact (nothing fell back), or the loud error naming call 1; never K's rows
    in C."""
    prog, res = _program(("stale", n), lambda: bm.scenario_stale_redo(n))
    assert res.hazards == [(1, 2)]
    for state in STATES:
        _check(prog, res, state)


@pytest.mark.parametrize("n", [300, 3000])
def test_relay_over_one_set_of_columns(n):
    """decode f1 -> cols, encode cols -> o1, decode f2 -> cols, encode cols -> o2: a relay that
    reuses its columns, as include/nxg_codec.h allows. With sequential ids no encode needs its
    columns again, so every state must be exact. With permuted ids the first encode may need
    columns that the second decode has overwritten: exact or the loud error naming call 1."""
    prog, res = _program(("relay", "S", n), lambda: bm.scenario_relay(n, "S"))
    for state in STATES:
        assert _check(prog, res, state, must_be_exact=True) == "exact"
    prog, res = _program(("relay", "P", n), lambda: bm.scenario_relay(n, "P"))
    assert res.hazards == [(1, 2)]
    for state in STATES:
        _check(prog, res, state)


@pytest.mark.parametrize("shuffle", ["permuted", "two-swapped"])
def test_declined_encode_into_a_small_buffer_stays_inside_it(shuffle):
    """A batch the sequential-id encoder declines (every id out of place, or just two swapped, so
    that most of its waves would write) into a buffer that is too small, synchronously and as
    an async call: the error is "too small", no byte outside [out, out + cap) changes (inside,
    a failed encode may leave anything), and the context then encodes the batch bit-exact."""
    import torch
    import netidx_amd
    import nxo
    n = 3000
    rng = np.random.default_rng(11)
    ids = bm.perm_ids(n, rng)
    if shuffle == "two-swapped":
        ids = np.sort(ids)
        ids[[700, 2200]] = ids[[2200, 700]]
    vals = bm.values(n, 11)
    ref = nxo.encode_f64(ids, vals)
    for cap, off, use_async in [(len(ref) - 1, 64, False), (len(ref) // 2, 64, False),
                                (len(ref) - 1, 69, True), (len(ref) // 2 + 3, 64, True)]:
        codec = netidx_amd.Codec(0)  # fresh: the sequential-id encoder is tried first
        try:
            cols = netidx_amd.columns_from_arrays(ids, vals)
            buf = torch.full((off + len(ref) + 64,), bm.SENT, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(netidx_amd.CodecError, match="too small"):
                if use_async:
                    codec.encode_async(cols, None, buf.data_ptr() + off, cap)
                    codec.sync()
                else:
                    codec.encode_into(cols, None, buf.data_ptr() + off, cap)
            h = buf.cpu().numpy()
            assert (h[:off] == bm.SENT).all() and (h[off + cap:] == bm.SENT).all(), \
                f"bytes outside [out, out + cap) changed (cap {cap}, async {use_async})"
            assert codec.encode_into(cols, None, buf.data_ptr() + off, len(ref)) == len(ref)
            h = buf.cpu().numpy()
            assert np.array_equal(h[off:off + len(ref)], ref)
            assert (h[:off] == bm.SENT).all() and (h[off + len(ref):] == bm.SENT).all()
        finally:
            codec.close()
