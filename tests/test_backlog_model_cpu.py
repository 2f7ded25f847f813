"""The sequential backlog model and its program generator (tests/backlog_model.py), on the CPU.

tests/test_gpu_backlog_order.py compares what nxg_ctx_sync leaves behind with this model, so the
model itself is pinned here: it reproduces the expected results of the three hand-built async
backlog tests (restated on the model's pool), its classification of a program as input-stable
or hazardous comes from the program alone, and the committed seeds cover what they are meant to.
"""
import numpy as np

import backlog_model as bm
import nxo


def _rows(cols):
    return cols["id"], cols["fixed"]


def _initial_rows(prog, b):
    o = nxo.decode(prog.frames[b]).trim()
    return o["id"], o["fixed"]


def test_model_late_decode_into_shared_columns():
    """test_async_backlog_keeps_wire_order_after_a_late_fallback, parts 1 and 3: the later
    frame's rows are the ones left, whichever decoder the first frame needed."""
    for first in "PH":
        p = bm.scenario_late_decode_shared_columns(300, first)
        r = bm.run(p)
        c = bm.MIXED if first == "H" else 0
        ids_b, vals_b = _initial_rows(p, 1)
        assert r.stable and r.frame_kind[:2] == [first, "S"]
        assert np.array_equal(r.cols[c]["id"], ids_b) and np.array_equal(r.cols[c]["fixed"], vals_b)
        assert r.cols[c]["n_rows"] == 300 and r.cols[c]["n_heartbeat"] == 0
        assert r.status == (300, 0, 0)
        assert r.d_len[:2] == [len(p.frames[0]), len(p.frames[1])]
        for b in range(3):  # decodes write no buffer
            assert np.array_equal(r.bufs[b], p.buffers()[b])


def test_model_late_decode_then_encode():
    """The same test, part 2: the encode reads the declined frame's rows."""
    p = bm.scenario_late_decode_then_encode(300)
    r = bm.run(p)
    ids_a, vals_a = _initial_rows(p, 0)
    wire_a = p.frames[0]
    assert r.stable and r.frame_kind[0] == "P" and r.batch_kind[1] == "P"
    assert r.len_out == [None, len(wire_a), None]
    assert np.array_equal(r.bufs[2][:len(wire_a)], wire_a)
    assert np.array_equal(r.cols[1]["id"], ids_a) and np.array_equal(r.cols[1]["fixed"], vals_a)
    ids_b, vals_b = _initial_rows(p, 1)
    assert np.array_equal(r.cols[0]["id"], ids_b) and np.array_equal(r.cols[0]["fixed"], vals_b)
    assert bm.late_decode_then_touch(p, r)


def test_model_late_encode_then_decode():
    """test_seq_encode_async_backlog_with_late_fallback: every frame is the oracle's encoding of
    its batch, and the decode returns the second batch."""
    p = bm.scenario_late_encode_then_decode(300)
    r = bm.run(p)
    refs = [nxo.encode_f64(i, v) for i, v in p.cols]
    assert r.stable and r.batch_kind[:3] == ["S", "P", "S"]
    for b in range(3):
        assert r.len_out[b] == len(refs[b])
        assert np.array_equal(r.bufs[b][:len(refs[b])], refs[b])
        # past the new frame: the longer old frame's tail, then the untouched margin
        assert np.array_equal(r.bufs[b][len(refs[b]):], p.buffers()[b][len(refs[b]):])
        assert (r.bufs[b][p.cap:] == bm.SENT).all() and len(r.bufs[b]) == p.cap + bm.MARGIN
    assert np.array_equal(r.cols[bm.MIXED]["id"], p.cols[1][0])
    assert np.array_equal(r.cols[bm.MIXED]["fixed"], p.cols[1][1])
    assert r.status == (300, 0, 0) and r.d_len[3] == len(refs[1])
    assert bm.late_encode_then_read(p, r)


def test_model_frame_overwritten_is_hazardous():
    """test_async_fallback_frame_overwritten_fails_loudly: the model lists the decode as a
    reader whose frame a later call writes; run in order, the decode still sees its frame."""
    p = bm.scenario_frame_overwritten(300)
    r = bm.run(p)
    assert not r.stable and r.hazards == [(0, 1)]
    ids_a, vals_a = _initial_rows(p, 0)
    assert np.array_equal(r.cols[0]["id"], ids_a) and np.array_equal(r.cols[0]["fixed"], vals_a)
    ref = nxo.encode_f64(*p.cols[1])
    assert r.len_out[1] == len(ref) and np.array_equal(r.bufs[0][:len(ref)], ref)


def test_model_named_scenarios_classified():
    cases = [(bm.scenario_write_after_write(300), [(1, 2)]),
             (bm.scenario_stale_redo(300), [(1, 2)]),
             (bm.scenario_relay(300, "S"), [(1, 2)]),
             (bm.scenario_relay(300, "P"), [(1, 2)])]
    for p, hz in cases:
        r = bm.run(p)
        assert r.hazards == hz and not r.stable, p.describe()
    # write-after-write: each decode returns the batch encoded just before it
    p = cases[0][0]
    r = bm.run(p)
    assert np.array_equal(r.cols[2]["id"], p.cols[0][0])
    assert np.array_equal(r.cols[bm.MIXED]["id"], p.cols[1][0])
    assert np.array_equal(r.cols[bm.MIXED]["fixed"], p.cols[1][1])
    # relay: o1 holds f1 again, o2 holds f2 again
    p = cases[3][0]
    r = bm.run(p)
    assert np.array_equal(r.bufs[1][:len(p.frames[0])], p.frames[0])
    assert np.array_equal(r.bufs[3][:len(p.frames[2])], p.frames[2])


def test_frame_kinds():
    rng = np.random.default_rng(1)
    for n in bm.ROWS:
        ids = bm.perm_ids(n, rng)
        assert len(np.unique(ids)) == n and int(ids.max() - ids.min()) == n - 1
        # one varint width: every record of the frame has one length
        assert len(bm.frame(ids, bm.values(n, 1))) % n == 0
        assert bm.ids_kind(ids) == ("S" if n == 1 else "P")
        assert bm.ids_kind(bm.seq_ids(n, 100)) == "S"
    ids, vals = bm.seq_ids(300, 100), bm.values(300, 2)
    f = bm.frame(ids, vals, 28)
    k = len(nxo.encode_f64(ids[:28], vals[:28]))
    assert bytes(f[k:k + 2]) == bm.HEARTBEAT and len(f) == len(nxo.encode_f64(ids, vals)) + 2
    o = nxo.decode(f).trim()
    assert o["err_kind"] == 0 and o["n_heartbeat"] == 1 and np.array_equal(o["id"], ids)


def test_committed_seeds_cover_what_they_should():
    seeds = bm.SEEDS
    assert len(seeds) >= 32 and len(set(seeds)) == len(seeds)
    stable = hazardous = late_dec = late_enc = grouped = 0
    rows = set()
    for s in seeds:
        p = bm.generate(s)
        q = bm.generate(s)  # the same program every time
        assert p.describe() == q.describe() and all(
            np.array_equal(a, b) for a, b in zip(p.frames, q.frames))
        assert 3 <= len(p.ops) <= 8 and p.n in bm.ROWS and len(p.frames) == bm.N_BUFS
        assert p.cap % 16 == 0
        r = bm.run(p)
        assert r.stable == (not r.hazards)
        # the classification, restated: a later call writes what an earlier call reads
        hz = []
        for i, a in enumerate(p.ops):
            for j in range(i + 1, len(p.ops)):
                b = p.ops[j]
                if a.kind == "D" and b.kind == "E" and a.buf == b.buf:
                    hz.append((i, j))
                if a.kind == "E" and b.kind == "D" and a.cols == b.cols:
                    hz.append((i, j))
        assert sorted(hz) == sorted(r.hazards)
        for i, o in enumerate(p.ops):
            assert (r.d_len[i] is not None) == (o.kind == "D")
            assert (r.len_out[i] is not None) == (o.kind == "E")
            if o.kind == "D" and r.frame_kind[i] == "H":
                assert o.cols == bm.MIXED
        for b in r.bufs:
            assert len(b) == p.cap + bm.MARGIN and (b[p.cap:] == bm.SENT).all()
        stable += r.stable
        hazardous += not r.stable
        late_dec += bm.late_decode_then_touch(p, r)
        late_enc += bm.late_encode_then_read(p, r)
        grouped += bool(p.groups)
        rows.add(p.n)
    assert 2 * stable >= len(seeds), stable
    assert late_dec >= 8, late_dec
    assert late_enc >= 8, late_enc
    assert hazardous >= 6, hazardous
    assert grouped >= 4 and rows == set(bm.ROWS)
