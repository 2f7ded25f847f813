"""The fan-out edge cases (tests/fanout_cases.py) on the CPU: (a) plan(), which restates the
kernels' launch decisions from constants read out of the kernel sources, says that every case
reaches the branch it is named for; (b) on every case the C oracle (nxo_dispatch,
nxo_publish_commit) equals a Python restatement of the reference's loop --
process_updates_batch (netidx/src/subscriber/connection.rs:546-567, tests/test_dispatch_cpu.py)
and UpdateBatch::commit for F64 rows (netidx/src/publisher/mod.rs:776-845, below). Cases above
10^5 rows are restated on their first 20 000 rows. The oracle then checks the GPU
(tests/test_gpu_fanout_edges.py)."""
import math
import struct

import numpy as np
import pytest

import fanout_cases as fc
import nxo
from test_dispatch_cpu import process_updates_batch

K = fc.constants()


# ---- the constants are read, and a miss is loud ------------------------------------------------
def test_constants_come_from_the_kernel_sources():
    for name in ("NXG_DISP_SEG", "NXG_DISP_U", "LCH", "SCAN_K", "TPB", "MAX_M", "RF", "kLookup",
                 "NARROW_BOUND", "PUB_SEG", "PUB_BINS", "NXG_PUB_GCAP"):
        assert K[name] > 0, name
    assert K["SCAN_B"] == K["SCAN_K"] * K["TPB"]


@pytest.mark.parametrize("fname,old,new", [
    ("nxg_dispatch.hip", "constexpr uint32_t LCH = ", "constexpr uint32_t LDS_CHANS = "),
    ("nxg_dispatch.hip", "#define NXG_DISP_SEG ", "#define NXG_DISP_SEGMENT "),
    ("nxg_dispatch.hip", "tb.n_chans < 0xfeu}", "tb.n_chans < narrow_bound()}"),
    ("nxg_dispatch.hip", ") seg *= 2;", ") seg *= 4;"),
    ("nxg_publish.hip", "#define NXG_PUB_GCAP ", "#define NXG_PUB_GRID "),
    ("nxg_publish.hip", "shift < bits; shift += 8", "shift < bits; shift += 4"),
])
def test_a_constant_that_is_not_found_fails_loudly(tmp_path, monkeypatch, fname, old, new):
    import os
    for f in ("nxg_dispatch.hip", "nxg_publish.hip"):
        with open(os.path.join(fc.CSRC, f)) as src:
            text = src.read()
        if f == fname:
            assert old in text
            text = text.replace(old, new)
        (tmp_path / f).write_text(text)
    monkeypatch.setattr(fc, "CSRC", str(tmp_path))
    fc.constants.cache_clear()
    try:
        with pytest.raises(RuntimeError, match=fname):
            fc.constants()
    finally:
        monkeypatch.undo()
        fc.constants.cache_clear()
    assert fc.constants()["LCH"] == K["LCH"]


def test_plan_restates_the_segment_doubling():
    # the smallest batches that double the segment once and twice on 2^20 channels
    n = 1 << 20
    per = K["MAX_M"] // n  # segments that still fit
    assert fc.plan(per * K["NXG_DISP_SEG"], n)["seg_rows"] == K["NXG_DISP_SEG"]
    assert fc.plan(per * K["NXG_DISP_SEG"] + 1, n)["seg_rows"] == 2 * K["NXG_DISP_SEG"]
    assert fc.plan(2 * per * K["NXG_DISP_SEG"] + 1, n)["seg_rows"] == 4 * K["NXG_DISP_SEG"]
    assert fc.plan(0, 0)["M"] == 0 and fc.plan(10, 0)["seg_rows"] == K["NXG_DISP_SEG"]


# ---- (a) every dispatch case reaches what its name claims --------------------------------------
def _dup_rows(c):
    """Rows whose subscription names some channel more than once."""
    dup_slot = np.array([len(set(c.stream_chan[a:b].tolist())) < b - a
                         for a, b in zip(c.stream_off[:-1], c.stream_off[1:])], bool)
    _, s = c.fan_of_rows()
    hit = s != fc.NO_SLOT
    out = np.zeros(c.n_rows, bool)
    out[hit] = dup_slot[s[hit]]
    return out


def _named(c, slot):
    return bool((c.ids == c.id_of_slot[slot]).any())


@pytest.mark.parametrize("name", fc.DISPATCH_CASES)
def test_dispatch_case_reaches_its_branch(name):
    c = fc.dispatch_case(name)
    p = fc.plan(c.n_rows, c.n_chans)
    fan, slot = c.fan_of_rows()
    assert c.reaches
    if len(c.stream_chan):
        assert int(c.stream_chan.max()) < c.n_chans  # within the ABI's contract
    if name.startswith("seg"):
        assert p["seg_rows"] == c.want_seg, p
        assert p["iterations"] == c.want_seg // p["group"] >= 2
        # the last segment is short, some segment is full
        assert c.n_rows % p["seg_rows"] not in (0,) and c.n_rows > p["seg_rows"]
    if name.endswith("_global"):
        assert not p["lds"]
    if name in ("seg256_global", "seg512_global"):
        assert p["cache"] == "none" and not p["fused"] and p["top_rounds"] > 1
    if name == "seg256_lds":
        assert p["lds"] and p["fused"] and p["nb"] == 8193 and p["top_rounds"] > 1
        assert int(fan.max()) <= 1
    if name.startswith("top_fused"):
        assert p["fused"] and p["nb"] == c.want_nb
        assert p["top_rounds"] == (1 if c.want_nb == K["TOP_CHAN"] else 2)
        # one fewer row stays within one round
        assert fc.plan(524288, 1024)["nb"] == K["TOP_CHAN"]
    if name == "top_unfused":
        assert not p["fused"] and p["nb"] > K["TOP"] and p["top_rounds"] == 2
        assert p["cache"] == "wide"
    if name.startswith("cache_"):
        n = c.n_chans
        want = "narrow" if n < K["NARROW_BOUND"] else "wide" if n < K["kLookup"] else "none"
        assert p["cache"] == want
        # the eight cases sit on both sides of both bounds
        assert {K["NARROW_BOUND"] - 1, K["NARROW_BOUND"], K["kLookup"] - 1,
                K["kLookup"]} <= set(fc.CACHE_CHANS)
        assert set(range(6)) <= set(fan.tolist())  # slots of 0..5 streams are named
        firsts, seconds = set(), set()
        for s in c.must_slots:
            assert _named(c, s), s
            ch = c.stream_chan[c.stream_off[s]:c.stream_off[s + 1]].tolist()
            if len(ch) == 2:
                firsts.add(ch[0])
                seconds.add(ch[1])
        assert {0, n - 2, n - 1} <= firsts and {0, n - 2, n - 1} <= seconds
    if name.startswith("dup_"):
        d = _dup_rows(c)
        assert p["lds"] == (name == "dup_lds")
        for group, lo, hi in (("two", 2, 2), ("few", 3, 4), ("many", K["RF"] + 1, 99)):
            rows = 0
            for s in c.groups[group]:
                ch = c.stream_chan[c.stream_off[s]:c.stream_off[s + 1]].tolist()
                assert lo <= len(ch) <= hi and len(set(ch)) < len(ch), (group, s, ch)
                assert _named(c, s), (group, s)
                rows += int((c.ids == c.id_of_slot[s]).sum())
            assert rows >= len(c.groups[group])
        assert int(d.sum()) >= 1000, int(d.sum())  # at least 1000 rows really repeat a channel
        # one channel named 2, 3, 4, 5 and 6 times by one row
        most = {max(np.bincount(c.stream_chan[a:b]).tolist()) for a, b in
                zip(c.stream_off[:-1], c.stream_off[1:]) if b > a}
        assert {2, 3, 4, 5, 6} <= most
        # steps in which only the repeat sends the wave to the match loop: no row above RF
        # streams, exactly one repeating row (k % 4 == 0) or several (k % 4 == 1)
        starts = np.arange(0, c.n_rows, fc.STEP)
        wide = np.add.reduceat((fan > K["RF"]).astype(np.int64), starts)
        rpt = np.add.reduceat(d.astype(np.int64), starts)
        k = np.arange(len(starts))
        assert (wide[k % 4 <= 1] == 0).all()
        assert (rpt[k % 4 == 0] == 1).all()
        assert (rpt[k % 4 == 1] > 1).all()
        two = np.zeros(c.n_rows, bool)  # the cached form: two streams on one channel
        two[slot != fc.NO_SLOT] = (fan[slot != fc.NO_SLOT] == 2)
        assert (np.add.reduceat((two & d).astype(np.int64), starts)[k % 4 <= 1] > 0).sum() >= 5
    if name.startswith("fan_"):
        assert p["lds"] == (name == "fan_lds")
        wide = fan > K["RF"]
        assert set(range(K["RF"] + 1, K["RF"] + 6)) <= set(fan[wide].tolist())
        per_step = np.add.reduceat(wide.astype(np.int64), np.arange(0, c.n_rows, fc.STEP))
        k = np.arange(len(per_step))
        assert (per_step[k % 3 == 0] == 1).all()   # the whole wave takes the match loop for one
        assert (per_step[k % 3 == 1] == 0).all()
        assert (per_step[k % 3 == 2] > 1).any()
    if name == "none_match":
        assert (slot == fc.NO_SLOT).all() and c.n_slots > 0
    if name == "no_chans":
        assert c.n_chans == 0 and p["M"] == 0 and c.n_slots > 0 and c.keep.any()
    if name == "no_slots":
        assert c.n_slots == 0 and c.n_chans > 0 and (c.slot_of_id == fc.NO_SLOT).all()
    # every case: Ids past the table, 2^64 - 1, holes
    assert (c.ids == np.uint64(fc.U64_MAX)).any()
    assert ((c.ids >= np.uint64(len(c.slot_of_id))) & (c.ids != np.uint64(fc.U64_MAX))).any()
    inside = c.ids < np.uint64(len(c.slot_of_id))
    assert (c.slot_of_id[c.ids[inside].astype(np.int64)] == fc.NO_SLOT).any()
    # a kept-`last` Id named twice in one step, in the next step, in another segment
    if name not in ("none_match", "no_slots"):
        r = c.repeat_rows
        assert (c.ids[r] == np.uint64(c.repeat_id)).all()
        assert c.keep[c.slot_of_id[c.repeat_id]] == 1
        assert r[0] // fc.STEP == r[1] // fc.STEP and r[1] // fc.STEP != r[2] // fc.STEP
        assert len({x // p["seg_rows"] for x in r}) >= 2
        if c.n_rows > 3 * p["seg_rows"] + 9:
            assert len({x // p["seg_rows"] for x in r}) >= 3


# ---- (b) oracle == restatement: dispatch -------------------------------------------------------
def _subscriptions(c):
    subs = {}
    for i in np.flatnonzero(c.slot_of_id != fc.NO_SLOT).tolist():
        s = int(c.slot_of_id[i])
        subs[i] = (int(c.sub_id[s]), c.stream_chan[c.stream_off[s]:c.stream_off[s + 1]].tolist(),
                   bool(c.keep[s]))
    return subs


@pytest.mark.parametrize("name", fc.DISPATCH_CASES)
def test_dispatch_oracle_equals_restatement(name):
    c = fc.dispatch_case(name)
    if c.n_rows > fc.LARGE_ROWS:
        c = fc.prefix(c, fc.PREFIX_ROWS)
    subs = _subscriptions(c)
    ids = c.ids.tolist()
    want, want_last = process_updates_batch(ids, subs, c.n_chans)
    off, esub, erow, last_row, um = nxo.dispatch(c.ids, *c.table(), c.n_chans)
    assert len(off) == c.n_chans + 1 and int(off[-1]) == len(esub) == len(erow)
    got = {int(ch): list(zip(esub[off[ch]:off[ch + 1]].tolist(),
                             erow[off[ch]:off[ch + 1]].tolist()))
           for ch in np.flatnonzero(np.diff(off.astype(np.int64)) > 0)}
    assert got == want
    last = {int(c.id_of_slot[s]): int(last_row[s]) - 1 for s in np.flatnonzero(last_row)}
    assert last == want_last
    assert um == sum(1 for i in ids if i not in subs)
    if name in ("none_match", "no_slots", "no_chans"):
        assert len(esub) == 0 and not off.any()
    if name == "no_chans":
        assert last and um > 0  # last rows and unmatched counts are still due
    if name.startswith("dup_"):
        # a repeated channel: one entry per stream, in stream order (adjacent, same row)
        s = int(c.groups["two"][0])
        ch = int(c.stream_chan[c.stream_off[s]])
        rows = [r for _, r in got[ch] if ids[r] == int(c.id_of_slot[s])]
        assert rows and rows == sorted(rows) and all(rows.count(r) == 2 for r in rows)


# ---- (b) oracle == restatement: commit ---------------------------------------------------------
def f64_eq(a, b):
    """Value::eq on two F64s given as bits (netidx-value/src/op.rs:133-172): NaN == NaN."""
    l, r = (struct.unpack("<d", struct.pack("<Q", x))[0] for x in (a, b))
    return (math.isnan(l) and math.isnan(r)) or l == r


def commit_f64(c):
    """UpdateBatch::commit (publisher/mod.rs:776-845) for F64 rows, on the case's arrays. For
    each queued message in order: Update(Some(cl)) goes to client cl alone if it is connected;
    otherwise the Id must be published (pb.by_id); UpdateChanged is dropped when the value's
    current equals it; the message goes to every subscribed client and becomes current.
    Returns ({client: [(id, row)]}, {slot: row that became current}, unmatched)."""
    batch, became, unmatched = {}, {}, 0
    current = {}
    n_ids = len(c.slot_of_id)
    for i, (idv, kd, to, v) in enumerate(zip(c.ids.tolist(), c.kind.tolist(),
                                             c.to_client.tolist(), c.fixed.tolist())):
        if kd == fc.PUB_UPDATE_CLIENT:
            if to < c.n_clients:
                batch.setdefault(to, []).append((idv, i))
            continue
        s = int(c.slot_of_id[idv]) if idv < n_ids else fc.NO_SLOT
        if s == fc.NO_SLOT:
            unmatched += 1
            continue
        if kd == fc.PUB_UPDATE_CHANGED and f64_eq(current.get(s, int(c.cur_fixed[s])), v):
            continue
        for cl in c.client[c.client_off[s]:c.client_off[s + 1]].tolist():
            batch.setdefault(cl, []).append((idv, i))
        current[s] = v
        became[s] = i
    return batch, became, unmatched


def oracle_commit(c):
    tag, aux, cur_tag, cur_aux = c.columns()
    heap = np.zeros(1, np.uint8)
    return nxo.publish_commit(c.ids, tag, c.fixed, aux, heap, c.kind, c.to_client, c.slot_of_id,
                              c.client_off, c.client, c.n_clients, cur_tag, c.cur_fixed, cur_aux,
                              heap)


CUS = 256  # any CU count sizes the stride case for this file; the GPU test uses the device's


@pytest.mark.parametrize("name", fc.COMMIT_CASES)
def test_commit_case_and_oracle(name):
    c = fc.commit_case(name, CUS)
    pp = fc.pub_plan(c.n_rows, c.n_slots, CUS)
    assert c.reaches
    # (a) the case is what its name says
    if name.startswith("single_repeat_"):
        p, q = c.pair
        ids = c.ids
        uniq, counts = np.unique(ids, return_counts=True)
        assert counts.max() == 2 and (counts == 2).sum() == 1 and uniq[counts == 2][0] == ids[p]
        assert ids[p] == ids[q] and c.kind[p] == fc.PUB_UPDATE and c.fixed[p] == fc.B
        assert c.kind[q] == fc.PUB_UPDATE_CHANGED
        assert c.fixed[q] == (fc.A if c.pushed else fc.B)
        assert (c.kind == fc.PUB_UPDATE_CHANGED).sum() > 1
        tpb = K["PUB_TPB"]
        where = name[len("single_repeat_"):].split("-")[0]
        if where in ("adjacent", "same_word_far"):
            assert p // 64 == q // 64 and p // 32 == q // 32  # one wave, one bitmap word
        if where == "other_run":
            assert p // 64 == q // 64 and p // 32 != q // 32
        if where == "lane63_64":
            assert p % 64 == 63 and q == p + 1 and p // tpb == q // tpb
        if where == "wg_edge":
            assert p % tpb == tpb - 1 and q == p + 1
        if where == "first_last":
            assert p == 0 and q == c.n_rows - 1
        if where == "stride":
            assert c.n_rows > tpb * K["NXG_PUB_GCAP"] * CUS and pp["strided"]
            assert q - p == pp["stride"]  # one thread's consecutive visits
        else:
            assert not pp["strided"]
        if c.order == "asc":
            # ascending Ids on an identity table: the slots of a wave fall in 2 bitmap words, the
            # repeat adds at most 2 runs -- within the runs path's bound
            assert (np.diff(np.delete(ids, q).astype(np.int64)) > 0).all()
            assert (c.slot_of_id[: c.n_rows] == np.arange(c.n_rows)).all()
            assert 2 + 2 <= K["PUB_HEADS"] and (c.kind != fc.PUB_UPDATE_CLIENT).all()
        else:
            assert (c.kind == fc.PUB_UPDATE_CLIENT).any() and (ids >= len(c.slot_of_id)).any()
    if name.startswith("repeat_only_directed"):
        p, q = c.pair
        same = np.flatnonzero(c.ids == c.ids[q])
        assert len(same) == 4 and (c.kind[same[:-1]] == fc.PUB_UPDATE_CLIENT).all()
        assert same[-1] == q and c.kind[q] == fc.PUB_UPDATE_CHANGED
        nd = c.ids[c.kind != fc.PUB_UPDATE_CLIENT]
        assert (np.unique(nd, return_counts=True)[1].max() == 2) == c.with_sort
    if name == "radix_4_passes":
        assert pp["passes"] == 4 and fc.pub_plan(c.n_rows, c.n_slots - 1, CUS)["passes"] == 3
        assert c.ids[10] == c.ids[12] == c.n_slots - 1 and c.kind[11] == fc.PUB_UPDATE_CLIENT
        assert (c.ids < 40).any() and (c.ids >= len(c.slot_of_id)).any()
    if name.startswith("directed_edges_"):
        d = c.kind == fc.PUB_UPDATE_CLIENT
        n = c.n_clients
        assert {0, n - 1, n, 0xFFFFFFFF} <= set(c.to_client[d].tolist())
        assert {0, n - 2, n - 1} <= set(c.client.tolist())
        assert fc.plan(c.n_rows, n)["cache"] == ("narrow" if n < K["NARROW_BOUND"] else "wide"
                                                 if n < K["kLookup"] else "none")
    # (b) the oracle equals the restatement
    full = c
    if c.n_rows > fc.LARGE_ROWS:
        c = fc.prefix(c, fc.PREFIX_ROWS)
    want, became, unmatched = commit_f64(c)
    off, eid, erow, cur_row, um = oracle_commit(c)
    got = {int(cl): list(zip(eid[off[cl]:off[cl + 1]].tolist(), erow[off[cl]:off[cl + 1]].tolist()))
           for cl in np.flatnonzero(np.diff(off.astype(np.int64)) > 0)}
    assert got == want
    assert {int(s): int(cur_row[s]) - 1 for s in np.flatnonzero(cur_row)} == became
    assert um == unmatched
    # the repeated row is pushed exactly when the case says so
    if hasattr(full, "pushed") and full.pair[1] < c.n_rows:
        q = full.pair[1]
        assert any(r == q for v in want.values() for _, r in v) == full.pushed
    if name == "slot_bits_31_32":
        pushed_rows = {r for v in want.values() for _, r in v}
        for r, s in full.again.items():
            assert (r in pushed_rows) == (int(c.fixed[r]) == fc.A), (r, s)
    if name.startswith("directed_edges_"):
        assert max(want) == c.n_clients - 1 and min(want) == 0


@pytest.mark.parametrize("n_clients", fc.DIRECTED_CLIENTS)
def test_unsubscribe_case(n_clients):
    ids, cl = fc.unsubscribe_case(n_clients)
    assert {0, n_clients - 2, n_clients - 1, n_clients, n_clients + 1, 0xFFFFFFFF} <= set(cl.tolist())
    off, ent = nxo.publish_unsubscribes(ids, cl, n_clients)
    want = {}
    for i, c in zip(ids.tolist(), cl.tolist()):
        if c < n_clients:
            want.setdefault(c, []).append(i)
    got = {int(c): ent[off[c]:off[c + 1]].tolist()
           for c in np.flatnonzero(np.diff(off.astype(np.int64)) > 0)}
    assert got == want
