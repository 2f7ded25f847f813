"""The value table on the CPU: the sequential model (tests/value_table_model.py) carried through
chains of commits against the restatement of UpdateBatch::commit and the oracle's last_row
(tests/test_publish_values_cpu.py), the case table's branches (tests/value_table_cases.py), and
the declarations. The GPU side is tests/test_gpu_value_table.py."""
import os
import random

import numpy as np
import pytest

import test_publish_values_cpu as P
import value_table_cases as VC
from value_table_model import (Capacity, Model, Refused, Source, read_value, sizes, table_trees,
                               NULL, UNSUBSCRIBED, ROW, SLOT, NOT_F64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IDS, N_ROWS, N_CLIENTS, COMMITS = 40, 60, 4, 5


def batch_source(a):
    ct, cf, ca = a["children"]
    return Source(a["tag"], a["fixed"], a["aux"], ct, cf, ca, bytes(a["heap"][:-1]))


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_model_chain_agrees_with_commit(seed):
    rng = random.Random(seed)
    rows, kind, to_client, by_id, slot_ids = P.random_case(rng, N_ROWS, N_IDS, N_CLIENTS)
    slot_of = {i: s for s, i in enumerate(slot_ids)}
    m = Model(len(slot_ids), 1 << 30, 1 << 30)
    first = VC.source_of([by_id[i][1] for i in slot_ids])
    m.apply(first, np.arange(1, len(slot_ids) + 1, dtype=np.uint64))
    replaced = 0
    for step in range(COMMITS):
        if step:
            rows = [(rng.randrange(N_IDS + 1), P.rand_value(rng)) for _ in range(N_ROWS)]
            kind = [rng.choice([0, 1, 1, 1, 2]) for _ in range(N_ROWS)]
            to_client = [rng.randrange(N_CLIENTS + 1) for _ in range(N_ROWS)]
        want, became = P.commit(rows, kind, to_client, by_id, N_CLIENTS)
        a = P.case_arrays(rows, kind, to_client, by_id, slot_ids, N_IDS)
        co, eid, erow, cur, um = P.run_oracle(a, N_CLIENTS)
        # `became` is the model's src_row: 1 + the row that became current, 0 for the others
        src_row = np.zeros(len(slot_ids), np.uint64)
        for idv, r in became.items():
            src_row[slot_of[idv]] = r + 1
        assert np.array_equal(np.asarray(cur, np.uint64), src_row)
        before = m.counters()
        res = m.apply(batch_source(a), src_row)
        assert res["n_applied"] == len(became)
        replaced += len(became)
        for idv, r in became.items():
            by_id[idv][1] = rows[r][1]
        # `current` afterwards is the model's table, tree for tree ...
        assert m.vals == [by_id[i][1] for i in slot_ids]
        # ... also when read back out of its arrays, and the counters are exact
        assert table_trees(m.arrays(), m.heap_used, m.child_used) == m.vals
        assert m.heap_live == sum(sizes(v)[0] for v in m.vals)
        assert m.child_live == sum(sizes(v)[1] for v in m.vals)
        assert m.heap_used == before[0] + res["need_bytes"]
        assert m.child_used == before[2] + res["need_children"]
    assert replaced > COMMITS  # the chain moved values
    # compaction keeps the values and drops the dead payload
    d, res = m.rebuild(m.n_slots + 3, m.heap_live, m.child_live)
    assert d.vals == m.vals + [NULL] * 3 and d.counters() == (m.heap_live, m.heap_live,
                                                              m.child_live, m.child_live)
    with pytest.raises(Capacity):
        m.rebuild(m.n_slots, max(m.heap_live - 1, 0), max(m.child_live - 1, 0))


def test_model_refusals_leave_the_table():
    vals = [VC.text(5), VC.VALUES["nest3"][0], VC.f64(1.0)]
    m = Model(3, 200, 40)
    m.apply(VC.source_of(vals), np.array([1, 2, 3], np.uint64))
    snap = (list(m.vals), m.counters(), bytes(m.heap), list(m.ctag))
    for name, (v, edit, cause) in VC.REFUSALS.items():
        S = VC.source_of([v, v, VC.f64(2.0)])
        src_row = np.array([3, 2, 1], np.uint64)
        if edit is not None:
            edit(S, 0)
            edit(S, 1)
        elif cause == ROW:
            src_row = np.array([0, 4, 9], np.uint64)
        with pytest.raises(Refused) as e:
            m.apply(S, src_row)
        assert (e.value.slot, e.value.cause) == (1, cause), name
        assert snap == (list(m.vals), m.counters(), bytes(m.heap), list(m.ctag)), name
    # a value the table holds, edited in place, refuses the calls that walk it
    for name, (v, edit, cause) in VC.OLD_REFUSALS.items():
        t = Model(4, 200, 40)
        t.apply(VC.source_of([v, VC.f64(1.0)]), np.array([2, 1, 1, 2], np.uint64))
        undo = []
        for s in (2, 1):
            field, idx, val = edit(t, s)
            arr = getattr(t, field)
            undo.append((arr, idx, int(arr[idx])))
            arr[idx] = val
        before = (t.counters(), bytes(t.heap), t.tag.tobytes(), t.fixed.tobytes())
        calls = (lambda: t.apply(VC.source_of([VC.f64(3.0)]), np.array([0, 1, 1, 1], np.uint64)),
                 lambda: t.rebuild(5, 200, 40), lambda: t.set_unsubscribed([2, 1, 9]))
        for call in calls:
            with pytest.raises(Refused) as e:
                call()
            assert (e.value.slot, e.value.cause, e.value.old) == (1, cause, True), name
            assert before == (t.counters(), bytes(t.heap), t.tag.tobytes(), t.fixed.tobytes())
        t.apply(VC.source_of([VC.f64(3.0)]), np.array([1, 0, 0, 1], np.uint64))  # others: fine
        for arr, idx, was in undo:
            arr[idx] = was
        for call in calls[:2]:
            call()
    # capacity: exact needs, the live totals the table would have, nothing changed
    big = VC.source_of([VC.text(190)])
    with pytest.raises(Capacity) as e:
        m.apply(big, np.array([1, 0, 0], np.uint64))
    assert (e.value.need_bytes, e.value.need_children) == (190, 0)
    assert e.value.live_bytes == m.heap_live - 5 + 190
    assert snap == (list(m.vals), m.counters(), bytes(m.heap), list(m.ctag))
    # Unsubscribed: a slot named twice counts once; a slot past the table is refused
    with pytest.raises(Refused) as e:
        m.set_unsubscribed([1, 7, 3])
    assert (e.value.slot, e.value.cause) == (3, SLOT)
    live = m.counters()
    b, c, _ = sizes(m.vals[1])
    m.set_unsubscribed([1, 1])
    assert m.vals[1] == UNSUBSCRIBED
    assert m.counters() == (live[0], live[1] - b, live[2], live[3] - c)
    # an F64 table takes tag 9 only
    f = Model(2, f64=True)
    with pytest.raises(Refused) as e:
        f.apply(VC.source_of([VC.f64(1.0), ("sc", 6, 1, 0)]), np.array([1, 2], np.uint64))
    assert (e.value.slot, e.value.cause) == (1, NOT_F64)
    f.apply(VC.source_of([VC.f64(1.0), VC.f64(2.0)]), np.array([2, 1], np.uint64))
    assert f.fixed.tolist() == [VC.f64(2.0)[2], VC.f64(1.0)[2]]


def test_cases_land_on_their_branches():
    p = VC.plan()
    B, T = p["block"], p["top"]
    assert B % 64 == 0 and T % 64 == 0 and p["copy"] == 16
    want = {"one": 1, "wave-1": 1, "wave": 1, "wave+1": 1, "block-1": 1, "block": 1,
            "block+1": 2, "top-1": -(-(T - 1) // B), "top": T // B, "top+1": T // B + 1}
    for name, n, (blocks, steps) in VC.slot_cases(p):
        assert (blocks, steps) == (want[name], 1), name
    assert T + 1 > B  # top + 1 starts a block that top does not
    n2 = VC.top_step_slots(p)
    assert VC.slots_branch(p, n2) == (T + 1, 2) and VC.slots_branch(p, n2 - 1) == (T, 1)
    for name, (v, branch) in VC.VALUES.items():
        assert VC.value_branch(v) == branch, name
    assert {b for _, b in VC.VALUES.values()} == {"scalar", "leaf", "flat", "stack"}
    assert all(VC.value_branch(v) == "scalar" for v in VC.SCALARS)
    # depth: NXG_MAX_DEPTH containers are read, one more is refused
    S = VC.source_of([VC.nested(32), VC.nested(33)])
    assert read_value(S, False, 0) == VC.nested(32)
    with pytest.raises(Exception):
        read_value(S, False, 1)
    # the copy kernel: short payloads never fill a block, long ones are all blocks but their ends;
    # every length from 16 on takes the one-load path at some phase and the byte path at another
    for n in VC.TEXT_LENS:
        got = [VC.copy_branch(p, 0, ph, [n]) for ph in range(16)]
        if n < 16:
            assert all(w == 0 for w, _ in got), n
        else:
            assert any(w for w, _ in got) and any(b for _, b in got), n
        if n == 100_000:
            assert all(w >= n // 16 - 1 and b <= 2 for w, b in got)
    assert VC.copy_branch(p, 0, 0, [32]) == (2, 0) and VC.copy_branch(p, 0, 1, [32]) == (1, 2)
    assert VC.copy_branch(p, 0, 0, [8, 8]) == (0, 1)  # a block over a segment edge: byte by byte
    assert VC.copy_branch(p, 3, 13, [16]) == (1, 0)   # the address decides, not the offset


def test_header_and_binding_declare_the_calls():
    from netidx_amd import codec
    hdr = open(os.path.join(ROOT, "include", "nxg_codec.h")).read()
    for sym in ("nxg_value_table_init", "nxg_value_table_apply", "nxg_value_table_rebuild",
                "nxg_value_table_set_unsubscribed"):
        assert f"bool {sym}(NxgCtx* ctx" in hdr, sym
        assert sym in codec.SIGNATURES, sym
    for ty in ("NxgValueTable", "NxgValueApply"):
        assert f"}} {ty};" in hdr and hasattr(codec, ty)
    import ctypes
    assert ctypes.sizeof(codec.NxgValueTable) == 14 * 8
    assert ctypes.sizeof(codec.NxgValueApply) == 5 * 8
    for m in ("init", "apply", "rebuild", "set_unsubscribed", "as_pub_columns", "as_columns"):
        assert callable(getattr(codec.ValueTable, m)), m
