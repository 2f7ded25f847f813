"""nxg_record_entries' expected results, checked without a GPU: the two models of
tests/record_model.py agree on every case of tests/record_cases.py, every case reaches the branch
it is named for, and the records decode to the kept entries' (archive Id, value) in order."""
import numpy as np
import pytest

import nxo
import record_cases as rc
import record_model as rm

K = rc.constants()
CASES = rc.cases(K)
REFUSALS = rc.refusal_cases(K)
PY_LIMIT = 70_000  # entries up to which the pure-Python writer runs (the others: the oracle alone)

_oracle = {}


def oracle(name):
    if name not in _oracle:
        _oracle[name] = rm.records_oracle(CASES[name][0])
    return _oracle[name]


def test_constants_are_read_from_the_kernels():
    assert K["tile"] % K["block"] == 0 and K["staging"] >= 16 * K["tile"] and K["top"] >= 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_models_agree(name):
    case, _, f64_too = CASES[name]
    assert rm.refusal(case) is None
    if case.n_entries <= PY_LIMIT:
        assert rm.records_python(case) == oracle(name)
    if f64_too:
        assert rm.records_oracle(case.f64_layout()) == oracle(name)
    blob, rec_off, rec_items, n_dropped = rm.expected(case, oracle(name))
    assert int(rec_off[-1]) == len(blob) and int(rec_off[0]) == 0
    assert len(blob) == int(rm.item_lens(case).sum()) + sum(
        rc._vl(int(k)) for k in rec_items if k)
    kept, _ = case.keep()
    assert int(rec_items.sum()) + n_dropped == case.n_entries - int(case.chan_off[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_branch(name):
    case, want, _ = CASES[name]
    p = rc.plan(case, K)
    assert rc.reaches(p, want), (want, p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_decode_to_the_kept_entries(name):
    case, _, _ = CASES[name]
    kept, aid = case.keep()
    span = case.is_span()
    S = case.src
    for c, rec in enumerate(oracle(name)):
        lo, hi = int(case.chan_off[c]), int(case.chan_off[c + 1])
        idx = lo + np.flatnonzero(kept[lo:hi])
        if not len(idx):
            assert rec == b""
            continue
        d, used = nxo.decode_archive(rec)
        assert used == len(rec), (c, used)
        o = d.trim()
        assert np.array_equal(o["id"], aid[idx].astype(np.uint64))
        rows = np.where(span[idx], 0, case.ent_row[idx]).astype(np.int64)
        tag = np.where(span[idx], rm.TAG_UNSUBSCRIBED, S.tag[rows])
        assert np.array_equal(o["tag"], tag)
        # (text and containers point elsewhere; a decoded bool / Null has its own `fixed`)
        same = ~np.isin(tag, (12, 13, 14, 15, 16, 18, 19, 20, 21, 22, 27, rm.TAG_UNSUBSCRIBED))
        # (a decode sign-extends the narrow signed tags: compare the bits the wire carries)
        bits = np.full(len(tag), 64)
        for ts, b in (((0, 1, 2, 3, 8), 32), ((25, 26), 16), ((23, 24), 8)):
            bits[np.isin(tag, ts)] = b
        mask = np.array([(1 << int(b)) - 1 for b in bits], np.uint64)
        assert np.array_equal((o["fixed"] & mask)[same], (S.fixed[rows] & mask)[same])
        nokid = ~np.isin(tag, (rm.TAG_UNSUBSCRIBED,))
        assert np.array_equal(o["aux"][nokid], S.aux[rows][nokid])
        for j in np.flatnonzero(np.isin(tag, (12, 13, 18, 27))):  # text: the bytes themselves
            f, a = int(o["fixed"][j]), int(o["aux"][j])
            g = int(S.fixed[rows[j]])
            assert rec[f:f + a] == S.heap[g:g + a]


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_lowest(name):
    case, what = REFUSALS[name]
    assert rm.refusal(case) == what
    if what[0] == "entry":
        kept, _ = case.keep()
        bad = [e for e in np.flatnonzero(kept)
               if int(case.ent_row[e]) >= case.src.n_rows
               or rm.value_cause(case.src, int(case.ent_row[e]))]
        assert len(bad) == 2 and bad[0] == what[1], bad


def test_max_vec_closed_form():
    assert rm.MAX_ITEMS == 89_478_485
    assert rm.f64_closed_form(rm.MAX_ITEMS, 0) == 4 + rm.MAX_ITEMS * 10
    assert rm.f64_closed_form(0, 0) == 0
