"""nxg_replay_window / nxg_replay_image without a GPU: the two models of tests/replay_model.py agree
on every case of tests/replay_cases.py, every case reaches the branch it is named for, the stop
protocol is observably the reference's playback, one commit of a window is the per-record commits
concatenated (through the oracle's publish_commit), and the calls are declared and exported."""
import ctypes
import os
import re

import numpy as np
import pytest

import nxo
import replay_cases as rc
import replay_model as rm

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
K = rc.constants()
CASES = rc.cases(K)
SHORT = rc.short_cases(K)
IMAGES = rc.image_cases(K)
WINDOWS = {**CASES, **SHORT}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_models_agree(name):
    c = WINDOWS[name]
    a, b = rm.window_loop(c.cols, c.infos, c.table), rm.window_numpy(c.cols, c.infos, c.table)
    assert a.same(b)
    assert a.n_rows == int(a.rec_off[-1]) and a.rec_off[0] == 0
    assert (np.diff(a.rec_off.astype(np.int64)) >= 0).all()
    assert (a.rec_off[a.n_done:] == a.rec_off[a.n_done]).all()
    assert (a.n_miss == 0) == (a.n_done == len(c.infos))


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_image_models_agree(name):
    c = IMAGES[name]
    a, b = rm.image_loop(c.image, c.order, c.table), rm.image_numpy(c.image, c.order, c.table)
    assert a.same(b)
    assert a.n_rows + a.n_dropped + a.n_miss == len(c.order)


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_case_reaches_its_branch(name):
    c = WINDOWS[name]
    f = rc.features(c, K)
    assert set(c.want) <= f, (name, sorted(set(c.want) - f), sorted(f))


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_image_case_reaches_its_branch(name):
    c = IMAGES[name]
    f = rc.image_features(c, K)
    assert set(c.want) <= f, (name, sorted(set(c.want) - f), sorted(f))


def test_every_named_branch_has_a_case():
    reached = set().union(*(rc.features(c, K) for c in WINDOWS.values()))
    for b in ("n_recs_0", "no_rows", "empty_front", "empty_between", "empty_behind",
              "empty3_at_tile_edge", "all_kept", "all_dropped", "rows_tile-1", "rows_tile+0",
              "rows_tile+1", "boundary_on_tile_edge", "record_over_3_tiles", "recs_gt_tile",
              "pub_above_2_32", "pub_near_miss", "unsub_kept", "array_kept", "text_kept",
              "miss_rec0", "miss_last", "miss_first_row_of_tile", "two_miss_records",
              "miss_ge_n_ids", "miss_behind_drop", "n_miss_below_cap", "n_miss_at_cap",
              "n_miss_above_cap", "cap_exact", "cap_short", "gaps", "lead"):
        assert b in reached, b
    reached = set().union(*(rc.image_features(c, K) for c in IMAGES.values()))
    for b in ("empty_image", "n_order_0", "absent", "present", "unsub_in_image", "unsorted",
              "duplicates", "order_ge_n_ids", "misses", "misses_above_cap", "drops",
              "order_tile-1", "order_tile+0", "order_tile+1", "order_3_tiles", "cap_exact"):
        assert b in reached, b


# ---- the stop protocol ---------------------------------------------------------------------------
def playback_window(seed, n_recs, n_arch, cap_miss):
    """A recording in which paths appear as it goes: (cols, infos, published, has_path, n_ids)."""
    rng = np.random.RandomState(seed)
    sizes = rng.randint(0, 40, n_recs)
    infos, row = [], 0
    for s in sizes:
        infos.append((row, int(s)))
        row += int(s)
    # later records draw from more Ids: new paths keep turning up; a few Ids lie past the table
    ids = np.concatenate([rng.randint(0, 5 + (n_arch * (i + 1)) // n_recs, s)
                          for i, s in enumerate(sizes)] or [np.zeros(0, np.int64)])
    vals = [rc.VALUE_CYCLE[k] for k in rng.randint(0, len(rc.VALUE_CYCLE), row)]
    cols = {"id": ids.astype(np.uint64), "tag": np.array([v[0] for v in vals], np.uint8),
            "fixed": np.array([v[1] + j for j, v in enumerate(vals)], np.uint64),
            "aux": np.array([v[2] for v in vals], np.uint32)}
    has_path = {a for a in range(n_arch + 5) if a % 5 != 3}  # the others: no path / filtered out
    published = {a: 10 + a for a in range(4) if a in has_path}
    return cols, infos, published, has_path, n_arch - 6


@pytest.mark.parametrize("replay", [rm.window_loop, rm.window_numpy], ids=["loop", "numpy"])
@pytest.mark.parametrize("seed,cap_miss", [(1, 64), (2, 2), (3, 1), (4, 64)])
def test_stop_protocol_is_the_reference_playback(seed, cap_miss, replay):
    cols, infos, published, has_path, n_ids = playback_window(seed, 30, 60, cap_miss)
    want, wpub = rm.reference_playback(cols, infos, published, has_path)
    got, gpub, calls = rm.protocol_playback(cols, infos, published, has_path, n_ids, cap_miss,
                                            replay)
    assert sum(len(p) for p, _ in want) > 10 and calls > 5  # paths did turn up as it went
    assert got == want
    assert gpub.current == wpub.current and gpub.next_id == wpub.next_id


# ---- one commit of a window = the per-record commits ----------------------------------------------
def commit(rows, lo, hi, pt):
    """nxo.publish_commit of rows [lo, hi), every row a Val::update (PUB_UPDATE)."""
    n = hi - lo
    return nxo.publish_commit(rows["id"][lo:hi], rows["tag"][lo:hi], rows["fixed"][lo:hi],
                              rows["aux"][lo:hi], np.zeros(1, np.uint8),
                              np.full(n, nxo.PUB_UPDATE, np.uint8), np.zeros(n, np.uint32), *pt)


@pytest.mark.parametrize("name", ["empty_records_around", "more_records_than_a_tile",
                                  "two_records_miss", "all_kept"])
def test_one_commit_equals_the_per_record_commits(name):
    c = CASES[name]
    res = c.expected()
    # scalar values only: the property is about routing, not about the values
    rows = dict(res.rows)
    rows["tag"] = np.where(np.isin(rows["tag"], (12, 19)), 3, rows["tag"]).astype(np.uint8)
    pubs = sorted(set(int(t) for t in c.table.tolist() if t not in (rm.DROP, rm.MISS)))
    n_clients, n_slots = 3, len(pubs)
    soi = np.full(max(pubs) + 1, nxo.NO_SLOT, np.uint32)
    soi[pubs] = np.arange(n_slots)
    fan = [[cl for cl in range(n_clients) if (s + cl) % 3 != 0] for s in range(n_slots)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in fan])]).astype(np.uint32)
    client = np.array([cl for x in fan for cl in x], np.uint32)
    pt = (soi, off, client, n_clients, np.full(n_slots, 16, np.uint8), np.zeros(n_slots, np.uint64),
          np.zeros(n_slots, np.uint32), np.zeros(1, np.uint8))
    coff, eid, erow, last, um = commit(rows, 0, res.n_rows, pt)
    whole = [list(zip(eid[int(coff[k]):int(coff[k + 1])].tolist(),
                      erow[int(coff[k]):int(coff[k + 1])].tolist())) for k in range(n_clients)]
    parts = [[] for _ in range(n_clients)]
    last_parts = np.zeros(n_slots, np.uint64)
    for i in range(res.n_done):
        lo, hi = int(res.rec_off[i]), int(res.rec_off[i + 1])
        if lo == hi:
            continue
        co, ei, er, la, u = commit(rows, lo, hi, pt)
        assert u == 0
        for k in range(n_clients):
            parts[k] += list(zip(ei[int(co[k]):int(co[k + 1])].tolist(),
                                 (er[int(co[k]):int(co[k + 1])] + np.uint64(lo)).tolist()))
        last_parts = np.where(la != 0, la + np.uint64(lo), last_parts)
    assert um == 0 and res.n_rows > 30
    assert whole == parts
    assert np.array_equal(last, last_parts)


# ---- the ABI ---------------------------------------------------------------------------------------
def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nxg_codec.h")).read()
    for sym in ("nxg_replay_window", "nxg_replay_image"):
        assert re.search(r"\bbool %s\(NxgCtx\*" % sym, header), f"{sym} is not declared"
    assert "#define NXG_REPLAY_DROP  0xffffffffffffffffull" in header
    assert "#define NXG_REPLAY_MISS  0xfffffffffffffffeull" in header
    for t in ("NxgReplayTable", "NxgReplayRows"):
        assert f"}} {t};" in header
    so = os.path.join(ROOT, "netidx_amd", "lib", "libnxg_codec.so")
    assert os.path.exists(so), "libnxg_codec.so is not built"
    L = ctypes.CDLL(so)
    for sym in ("nxg_replay_window", "nxg_replay_image"):
        assert hasattr(L, sym), f"{sym} is not exported"
