"""nxg_archive_index_records' and nxg_archive_scan_index's expected results, checked without a GPU:
the two writer models of tests/archive_index_model.py agree, the writer's bytes fed to the scan
model match exactly the Ids they hold (plus the count quirk), every indexed record of
tests/golden/zstd_records.bin parses and scans as the model says, every named case of
tests/archive_index_cases.py reaches the branch it is there for, and the library declares, exports
and binds both calls."""
import json
import os

import numpy as np
import pytest

import archive_index_cases as ac
import archive_index_model as am

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = ac.constants()
CASES = ac.cases(K)
REFUSALS = ac.refusal_cases(K)
SCANS = ac.scan_cases(K)


def parse_index(b):
    """(ids, bytes used) of a canonical RecordIndex."""
    L, p = am.decode_varint(b, 0)
    count, q = am.decode_varint(b, p)
    ids = []
    for _ in range(count):
        i, q = am.decode_varint(b, q)
        ids.append(i)
    assert q == L, "the length varint counts itself"
    return ids, q


# ---- the writer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_models_agree(name):
    case = CASES[name][0]
    assert am.refusal(case) is None
    blob, off, ids = am.expected(case)
    nb, noff, nids = am.indexes_numpy(case)
    assert nb == blob
    assert np.array_equal(noff, off) and np.array_equal(nids, ids)


@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_case_reaches_its_branch(name):
    case, want = CASES[name]
    p = ac.plan(case, K)
    assert ac.reaches(p, want), (want, {k: p[k] for k in want})


def test_writer_cases_cover_the_edges():
    plans = {n: ac.plan(c, K) for n, (c, _) in CASES.items() if c.n_keys <= 4 * K["tile"] or
             n.startswith(("inner", "count"))}
    widths = set().union(*(p["len_widths"] for p in plans.values()))
    assert {1, 2, 3} <= widths
    assert {1, 2} <= set().union(*(p["count_widths"] for p in plans.values()))
    assert any(p["wrapped"] for p in plans.values())
    # the widths of varint(L) change where the issue says, and one byte further up
    assert [am.varint_len(am.len_wrapped_len(t)) for t in (126, 127, 16381, 16382, 16383)] == \
        [1, 2, 2, 3, 3]


def test_first_occurrence_order_and_bytes():
    c = am.Case([9, 300, 9, 5, 300, 70000, 5], [0, 3, 7])
    recs = am.indexes_python(c)
    assert [o for _, o in recs] == [[9, 300], [5, 300, 70000]]
    assert recs[0][0] == bytes([5, 2, 9, 0xAC, 0x02])
    # golden/make_zstd.py's index_bytes writes the same form
    assert recs[1][0] == bytes([8, 3, 5, 0xAC, 0x02, 0xF0, 0xA2, 0x04])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_cases(name):
    case, what = REFUSALS[name]
    assert am.refusal(case) == what


def test_max_vec_is_out_of_reach_of_a_test():
    """count * 4 > MAX_VEC needs 2^29 + 1 distinct Ids in one record: not run."""
    assert am.MAX_VEC // 4 + 1 == (1 << 29) + 1


# ---- writer -> scanner ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["recs1000", "table", "id_widths", "same_ids_every_record",
                                  "count_128", "inner_127"])
def test_written_indexes_scan_as_their_ids(name):
    case = CASES[name][0]
    rng = np.random.default_rng(5)
    for b, order in am.indexes_python(case):
        if not b:
            continue
        assert parse_index(b) == (order, len(b))
        n_ids = 1 << 16
        small = [i for i in order if i < n_ids]
        held = set(small) | ({len(order)} if len(order) < n_ids else set())  # the count quirk
        for pick in (small[:1], small[-1:], [len(order)], [int(x) for x in rng.integers(0, 400, 3)]):
            keep = np.zeros(n_ids, np.uint8)
            keep[pick] = 1
            want = am.MATCH if held & set(pick) else am.NONE
            assert am.scan_index_at(b + b"\x09\x09", 0, len(b) + 2, keep) == want


# ---- the scanner -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCANS))
def test_scan_case_reaches_its_branch(name):
    sc = SCANS[name]
    assert ac.scan_reaches(sc, K), (sc.want, ac.scan_plan(sc, 0, K))


def test_scan_cases_cover_the_rule():
    verdicts = {sc.verdict() for sc in SCANS.values()}
    assert verdicts == {am.NONE, am.MATCH, am.ERR_SHORT, am.ERR_FORMAT}
    where = [ac.scan_plan(sc, ph, K)["where"] for sc in SCANS.values() for ph in range(16)]
    where = [w for w in where if w]
    assert {w["byte"] for w in where} == set(range(16))
    assert any(w["crosses_block"] for w in where) and any(w["crosses_step"] for w in where)
    assert any(w["crosses_piece"] for w in where) and any(w["piece"] == 2 for w in where)


def test_scan_port_details():
    keep = np.zeros(16, np.uint8)
    keep[5] = 1
    # 81 00 is index_len 1 in two bytes: the body is 1 - varint_len(1) = 0 bytes behind them
    assert am.scan_index_at(b"\x81\x00\x05", 0, 3, keep) == am.NONE
    assert am.scan_index_at(b"\x82\x00\x05", 0, 3, keep) == am.MATCH
    assert am.scan_index_at(b"\x02\x05", 0, 2, keep) == am.MATCH       # the count is walked
    assert am.scan_index_at(b"\x03\x01\x85\x80\x80\x80\x10", 0, 7, keep) == am.ERR_SHORT  # 01 85
    assert am.scan_index_at(b"\x07\x01\x85\x80\x80\x80\x10", 0, 7, keep) == am.MATCH  # 2^32 + 5


# ---- the golden indexed records ----------------------------------------------------------------------------
def golden_indexed():
    m = json.load(open(os.path.join(G, "zstd_manifest.json")))["records"]
    rec = open(os.path.join(G, "zstd_records.bin"), "rb").read()
    return rec, [e for e in m if e["indexed"]]


def test_golden_indexed_records_parse_and_scan():
    rec, ents = golden_indexed()
    assert len(ents) >= 5
    for e in ents:
        lo, end = e["rec_off"] + 4, e["rec_off"] + e["rec_len"]
        ids, used = parse_index(rec[lo:end])
        assert used == e["index_len"] and len(ids) > 0
        assert am.record_index(ids) == rec[lo:lo + used]
        n_ids = max(max(ids), len(ids)) + 2
        for pick, want in (([ids[0]], am.MATCH), ([ids[-1]], am.MATCH), ([len(ids)], am.MATCH),
                           ([], am.NONE)):
            keep = np.zeros(n_ids, np.uint8)
            keep[pick] = 1
            assert am.scan_index_at(rec, lo, end, keep) == want
        keep = np.ones(n_ids, np.uint8)
        keep[ids] = 0
        keep[len(ids)] = 0
        assert am.scan_index_at(rec, lo, end, keep) == am.NONE


# ---- the library ---------------------------------------------------------------------------------------------
def test_library_exports_and_binds_both_calls():
    import netidx_amd
    from netidx_amd import codec
    lib = netidx_amd.lib()
    for sym in ("nxg_archive_index_records", "nxg_archive_scan_index"):
        assert hasattr(lib, sym), sym
    assert hasattr(codec.Codec, "index_records") and hasattr(codec.Codec, "scan_index")
    assert (codec.INDEX_NONE, codec.INDEX_MATCH, codec.INDEX_ERR_SHORT, codec.INDEX_ERR_FORMAT) == \
        (am.NONE, am.MATCH, am.ERR_SHORT, am.ERR_FORMAT)
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "nxg_codec.h")).read()
    for code, name in ((am.NONE, "NONE"), (am.MATCH, "MATCH"), (am.ERR_SHORT, "ERR_SHORT"),
                       (am.ERR_FORMAT, "ERR_FORMAT")):
        assert f"#define NXG_INDEX_{name} {code}" in hdr


# ---- refusals that need no device ----------------------------------------------------------------------------
def _host_ptrs():
    """Host arrays standing in for every pointer (never read: each refusal comes first)."""
    a = {k: np.zeros(64, np.uint64) for k in ("key", "seg_off", "table", "out", "idx_off",
                                               "idx_ids", "dbuf", "keep")}
    return {k: v.ctypes.data for k, v in a.items()}, a


@pytest.mark.parametrize("null", ac.WRITER_NULLS)
def test_writer_null_argument_is_refused_by_name(null):
    ptrs, alive = _host_ptrs()
    ok, msg = ac.raw_index_records(None, ptrs, null)
    assert not ok and msg == f"null argument ({null})", msg


@pytest.mark.parametrize("null", ac.SCAN_NULLS)
def test_scan_null_argument_is_refused_by_name(null):
    ptrs, alive = _host_ptrs()
    ok, msg, verdict = ac.raw_scan_index(None, ptrs, null)
    assert not ok and msg == f"null argument ({null})", msg
    assert (verdict == 0xEE).all()


def test_null_arguments_that_are_allowed_and_the_null_ctx():
    ptrs, alive = _host_ptrs()
    # nothing to read: idx_ids with no records, key with no keys, the table's array with no SubIds
    for kw in (dict(null="out->idx_ids", n_recs=0), dict(null="key", n_keys=0),
               dict(null="tab->arch_id_of_sub", n_subs=0)):
        ok, msg = ac.raw_index_records(None, ptrs, **kw)
        assert not ok and msg == "null argument (ctx)", (kw, msg)
    ok, msg = ac.raw_index_records(None, ptrs, n_keys=(1 << 28) + 1)
    assert not ok and "too many positions" in msg
    ok, msg = ac.raw_index_records(None, ptrs, n_keys=1 << 28)
    assert not ok and msg == "null argument (ctx)"
    for null in ("dbuf", "idx_off", "idx_end", "verdict"):
        ok, msg, _ = ac.raw_scan_index(None, ptrs, null, n=0, off=(), end=())
        assert not ok and msg == "null argument (ctx)", (null, msg)
    ok, msg, _ = ac.raw_scan_index(None, ptrs, "keep", n_ids=0)
    assert not ok and msg == "null argument (ctx)"
    # ranges are checked before the ctx too
    ok, msg, _ = ac.raw_scan_index(None, ptrs, off=(41,))
    assert not ok and "record 0" in msg and "not a range" in msg
    ok, msg, _ = ac.raw_scan_index(None, ptrs, end=(65,))
    assert not ok and "record 0" in msg and "not a range" in msg
