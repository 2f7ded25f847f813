"""The one grow routine of every grow-on-demand GPU buffer (netidx_amd/csrc/nxg_devbuf.h), through
its debug entry point nxg_debug_devbuf_grow. No GPU: the entry point runs the production steps
against a scripted fake of the four operations they call (stream synchronise, free, allocate,
memset) and reports the buffer they leave and the operations they issued.

The invariant: a buffer is empty (null, capacity 0) or holds a live allocation of exactly its
capacity. A failed synchronise leaves it as it was; any later failure leaves it empty, never a
null pointer under a capacity, so the next call grows again.
"""
import ctypes as C

import pytest

import netidx_amd
from netidx_amd.codec import NetidxError

SYNC, FREE, ALLOC, MEMSET, PINNED = 1, 2, 3, 4, 16
KIB, MIB = 1 << 10, 1 << 20

# the policy table ("Grow-on-demand buffers"): row -> (element bytes, size, zeroed)
DOUBLE, DOUBLE_64K, TSTAT, ESCRATCH, FRAME, WRITE_COLS, ZSTD_RECS, ZSTD_ENC, FIRST = range(9)
POLICY = {
    DOUBLE: (1, lambda need, cap: max(need, 2 * cap), False),
    DOUBLE_64K: (1, lambda need, cap: max(need, 2 * cap, 64 * KIB), False),
    TSTAT: (8, lambda need, cap: max(need, 2 * cap, 4096), True),
    ESCRATCH: (8, lambda need, cap: max(need, 1024), False),
    FRAME: (1, lambda need, cap: max(need, MIB), False),
    WRITE_COLS: (8, lambda need, cap: max(need, 1024), False),
    ZSTD_RECS: (1, lambda need, cap: max(need, 64 * KIB), False),
    ZSTD_ENC: (1, lambda need, cap: max(need + need // 4, 64 * KIB), False),
    FIRST: (8, lambda need, cap: max(need, 4096), True),
}
# per row: a need below its floor (the first row has none) and one above it; the third need of
# a test lies between the capacity these leave behind and twice that
NEEDS = {
    DOUBLE: (100, 5000),
    DOUBLE_64K: (100, 100_000),
    TSTAT: (100, 5000),
    ESCRATCH: (100, 5000),
    FRAME: (100 + 16, 3 * MIB + 16),
    WRITE_COLS: (100, 5000),
    ZSTD_RECS: (100, 100_000),
    ZSTD_ENC: (100, 100_000),
    FIRST: (100, 5000),
}


def grow(ptr, cap, policy, need, fail=0, elem=None, pinned=False):
    """One call on the buffer (ptr, cap). Returns (ok, message, ptr, cap, [(op, arg), ...])."""
    f = netidx_amd.lib().nxg_debug_devbuf_grow
    f.restype = C.c_bool
    p, c, n = C.c_uint64(ptr), C.c_uint64(cap), C.c_uint32(0)
    ops, args = (C.c_uint32 * 8)(), (C.c_uint64 * 8)()
    err = NetidxError()
    elem = POLICY[policy][0] if elem is None else elem
    ok = f(C.byref(p), C.byref(c), C.c_uint32(elem), C.c_bool(pinned), C.c_uint32(policy),
           C.c_uint64(need), C.c_uint32(fail), ops, args, C.byref(n), C.byref(err))
    msg = err.msg.decode() if err.msg else None
    netidx_amd.lib().nxg_error_free(C.byref(err))
    assert n.value <= 8
    return ok, msg, p.value, c.value, [(ops[i], args[i]) for i in range(n.value)]


def test_first_allocation_from_empty():
    ok, msg, p, cap, ops = grow(0, 0, DOUBLE, 300)
    assert ok and msg is None
    assert p != 0 and cap == 300
    assert ops == [(SYNC, 0), (ALLOC, 300)]  # (nothing to free)


@pytest.mark.parametrize("policy", sorted(POLICY))
def test_need_zero_leaves_an_empty_buffer_empty(policy):
    """Growing never makes a buffer non-null for a need of 0, whatever the row's floor: a call
    site whose kernels refuse a null pointer asks for at least one element (ensure_dwcols)."""
    assert grow(0, 0, policy, 0) == (True, None, 0, 0, [])
    ok, _, p, cap, ops = grow(0, 0, policy, 1)
    assert ok and p != 0 and cap == POLICY[policy][1](1, 0) and len(ops) >= 2


@pytest.mark.parametrize("policy", sorted(POLICY))
def test_need_within_capacity_issues_nothing(policy):
    ok, _, p, cap, ops = grow(0, 0, policy, NEEDS[policy][1])
    assert ok
    for need in (0, 1, cap - 1, cap):
        assert grow(p, cap, policy, need) == (True, None, p, cap, [])


@pytest.mark.parametrize("policy", sorted(POLICY))
def test_policy_sizes_and_operation_order(policy):
    elem, size, zeroed = POLICY[policy]
    p, cap = 0, 0
    below, above = NEEDS[policy]
    # (the cases are what they claim: the floor decides the first size and not the second)
    assert policy == DOUBLE or size(below, 0) > below + below // 4
    assert size(above, 0) in (above, above + above // 4)
    for step in range(3):
        need = (below, above, cap + cap // 2)[step]
        assert step < 2 or cap < need < 2 * cap
        want = size(need, cap)
        ok, msg, p2, cap2, ops = grow(p, cap, policy, need)
        assert ok and msg is None
        assert cap2 == want, (policy, need, cap)
        assert p2 != 0
        expect = [(SYNC, 0)] + ([(FREE, p)] if p else []) + [(ALLOC, want * elem)]
        if zeroed:
            expect.append((MEMSET, want * elem))  # the whole new allocation
        assert ops == expect
        p, cap = p2, cap2


def test_pinned_memory_frees_and_allocates_pinned():
    ok, _, p, cap, ops = grow(0, 0, ZSTD_ENC, 100_000, pinned=True)
    assert ok and ops == [(SYNC, 0), (ALLOC + PINNED, 125_000)]
    ok, _, p2, cap2, ops = grow(p, cap, ZSTD_ENC, 200_000, pinned=True)
    assert ok and cap2 == 250_000
    assert ops == [(SYNC, 0), (FREE + PINNED, p), (ALLOC + PINNED, 250_000)]


@pytest.mark.parametrize("policy", (DOUBLE, TSTAT))
def test_failed_alloc_empties_and_the_next_call_allocates_again(policy):
    elem, size, zeroed = POLICY[policy]
    _, _, p, cap, _ = grow(0, 0, policy, 5000)
    ok, msg, p2, cap2, ops = grow(p, cap, policy, 3 * cap, fail=ALLOC)
    assert not ok and msg and "allocation" in msg
    assert (p2, cap2) == (0, 0)
    assert [o for o, _ in ops] == [SYNC, FREE, ALLOC]  # (no memset of what is not there)
    # a smaller need than the old capacity: the stale-capacity bug returned true here and the
    # null pointer went on to a copy or a kernel
    need = cap // 2
    ok, msg, p3, cap3, ops = grow(p2, cap2, policy, need)
    assert ok and msg is None
    assert p3 != 0 and cap3 == size(need, 0)
    assert [o for o, _ in ops] == [SYNC, ALLOC] + ([MEMSET] if zeroed else [])


def test_failed_free_leaves_capacity_zero():
    _, _, p, cap, _ = grow(0, 0, DOUBLE, 5000)
    ok, msg, p2, cap2, ops = grow(p, cap, DOUBLE, 20_000, fail=FREE)
    assert not ok and msg and "free" in msg
    assert (p2, cap2) == (0, 0)
    assert ops == [(SYNC, 0), (FREE, p)]


def test_failed_sync_leaves_the_buffer_as_it_was():
    _, _, p, cap, _ = grow(0, 0, TSTAT, 5000)
    ok, msg, p2, cap2, ops = grow(p, cap, TSTAT, 20_000, fail=SYNC)
    assert not ok and msg and "synchronize" in msg
    assert (p2, cap2) == (p, cap)
    assert ops == [(SYNC, 0)]  # nothing freed


def test_failed_memset_leaves_the_buffer_empty():
    _, _, p, cap, _ = grow(0, 0, FIRST, 5000)
    ok, msg, p2, cap2, ops = grow(p, cap, FIRST, 20_000, fail=MEMSET)
    assert not ok and msg and "memset" in msg
    assert (p2, cap2) == (0, 0)
    # (the new allocation is handed back, not left under a zero capacity)
    assert [o for o, _ in ops] == [SYNC, FREE, ALLOC, MEMSET, FREE]
    assert ops[1][1] == p and ops[4][1] not in (0, p)
