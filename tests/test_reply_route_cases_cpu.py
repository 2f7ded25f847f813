"""The contract of nxg_route_replies against the reference, before any kernel: hand-written
expectations for one message of each row of the contract's table, and on crafted and random
batches the chained calls (stops, host updates in between) equal to the sequential restatement of
process_batch on the whole batch. The case lists must reach every outcome and every stop."""
import pytest

import reply_route_cases as rc
import reply_route_model as rm


def one_call(st, msgs, n_ids, n_chans):
    tab, _, _ = rm.tables_of(st, n_ids, n_chans)
    ids, spans = rm.split(msgs)
    return rm.contract_call(tab, ids, spans, 0, 0)


@pytest.mark.parametrize("case", rc.hand_cases(), ids=lambda c: c[0])
def test_one_message_of_each_kind_by_hand(case):
    name, st, msgs, n_ids, n_chans, want = case
    out = one_call(st, msgs, n_ids, n_chans)
    for field, v in want.items():
        assert out[field] == v, field


def test_the_wire_of_an_unsubscribe_by_hand():
    assert rm.to_unsubscribe(5) == bytes([3, 1, 5])
    assert rm.to_unsubscribe(2**64 - 1) == bytes([12, 1] + [0xFF] * 9 + [1])


def chained_equals_sequential(case, log):
    name, st, msgs, n_ids, n_chans = case[:5]
    want = rm.process_batch(st.copy(), msgs)
    got = rm.run_chained(st.copy(), msgs, rm.contract_call, n_ids, n_chans, log)
    assert rm.same(want, got) == [], name
    return want


ALL = rc.crafted_cases() + rc.sized_cases() + rc.random_cases()


@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_chained_calls_equal_the_sequential_model(case):
    chained_equals_sequential(case, [])


def test_sized_cases_take_one_call():
    for case in rc.sized_cases():
        log = []
        chained_equals_sequential(case, log)
        assert len(log) == 1, case[0]


def test_the_cases_reach_every_outcome_and_every_stop():
    outcomes, stops, model_outcomes = set(), set(), set()
    for case in ALL:
        log = []
        want = chained_equals_sequential(case, log)
        for stopped, ocs in log:
            stops.add(stopped)
            outcomes |= set(ocs)
        model_outcomes |= set(want.outcome.values())
    assert stops == {0, 1, 2}
    assert outcomes == set(range(7))
    assert model_outcomes >= set(range(7)) | {rm.ALIAS}


def test_sized_cases_reach_every_outcome_too():
    seen = set()
    for case in rc.sized_cases():
        if sum(1 for m in case[2] if m[0] != "upd") > 250:
            log = []
            chained_equals_sequential(case, log)
            assert set(log[0][1]) == set(range(7)), case[0]
            seen.add(case[0])
    assert len(seen) >= 3


def test_wire_quirks_keep_the_message():
    g = rc.tw.mg()
    m = ("unsub", 5)
    assert rc.message(m) == bytes([3, 2, 5])
    assert rc.message(m, "noncanon") == bytes([0x83, 0, 2, 5])
    assert rc.message(m, "trailing") == g.enc_msg(2, b"\x05\xff\x00\x80")
