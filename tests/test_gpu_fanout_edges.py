"""The fan-out kernels (nxg_dispatch.hip, nxg_publish.hip) at every internal threshold they
branch on: the cases of tests/fanout_cases.py through the product calls, compared with the CPU
oracle (nxo_dispatch / nxo_publish_commit / nxo_publish_unsubscribes, pinned to the reference's
loops by tests/test_fanout_cases_cpu.py) for exact equality of chan_off, n_entries, ent_sub and
ent_row up to n_entries, last_row and n_unmatched. Also: outputs at exactly their capacities
with guard bands behind them, at full and at short capacity; one context through a sequence of
shapes; the unsubscribe route at the row cache's bounds. Every input is within the ABI's
contract (channels < n_chans)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fanout_cases as fc
import guards
import nxo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def same(case, what, got, want):
    """Exact equality, with a message that names the case and the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError(f"{case}: {what} has {got.shape[0]} elements, the oracle "
                             f"{want.shape[0]}")
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{case}: {what} differs from the oracle in {len(bad)} of "
                             f"{len(want)} elements, first at [{i}]: {int(got[i])} != "
                             f"{int(want[i])}")


def check(case, d, want):
    """A Dispatch (or a GuardedDispatch with n_entries / n_unmatched set) against the oracle's
    (chan_off, ent_sub, ent_row, last_row, n_unmatched)."""
    w_off, w_sub, w_row, w_last, w_um = want
    if isinstance(d, guards.GuardedDispatch):
        arr = lambda k, n=None: d.host(k, n)
    else:
        arr = lambda k, n=None: getattr(d, k)[:n].cpu().numpy().view(np.uint64)
    same(case, "chan_off", arr("chan_off", len(w_off)), w_off)
    if d.n_entries != len(w_sub):
        raise AssertionError(f"{case}: n_entries {d.n_entries}, the oracle {len(w_sub)}")
    same(case, "ent_sub", arr("ent_sub", d.n_entries), w_sub)
    same(case, "ent_row", arr("ent_row", d.n_entries), w_row)
    same(case, "last_row", arr("last_row", len(w_last)), w_last)
    if d.n_unmatched != w_um:
        raise AssertionError(f"{case}: n_unmatched {d.n_unmatched}, the oracle {w_um}")


# ---- dispatch ----------------------------------------------------------------------------------
def _oracle_dispatch(name):
    c = fc.dispatch_case(name)
    return nxo.dispatch(c.ids, *c.table(), c.n_chans)


_oracle_dispatch_cached = functools.lru_cache(maxsize=None)(_oracle_dispatch)


def oracle_dispatch(name):
    """Computed once per case and shared (read-only); the 8.4 M-row case is not held."""
    return _oracle_dispatch(name) if name == "seg256_lds" else _oracle_dispatch_cached(name)


def device_case(c):
    import torch
    import netidx_amd
    tab = netidx_amd.SubTable(*c.table(), c.n_chans)
    ids = torch.from_numpy(c.ids.view(np.int64).copy()).cuda()
    return tab, ids


def run_dispatch(codec, name):
    c = fc.dispatch_case(name)
    tab, ids = device_case(c)
    d = codec.dispatch_updates(tab, ids)
    check(name, d, oracle_dispatch(name))
    return d


@pytest.mark.parametrize("name", fc.DISPATCH_CASES)
def test_dispatch_case(codec, name):
    d = run_dispatch(codec, name)
    if name in ("none_match", "no_chans", "no_slots"):
        assert d.n_entries == 0, name
    if name == "no_chans":
        assert d.n_unmatched > 0 and bool(d.last_row.any()), name


def test_one_context_through_a_sequence():
    """Scratch regrowth from nothing, a small call after a large one (stale hist, cursors and row
    cache behind it), the fused path's skipped chan_off memset, M = 0 in between."""
    import netidx_amd
    c = netidx_amd.Codec(0)
    try:
        for name in ("seg256_global", "cache_253", "top_fused_1025", "no_chans", "cache_65534",
                     "cache_253"):
            run_dispatch(c, name)
    finally:
        c.close()


# ---- commit ------------------------------------------------------------------------------------
def oracle_commit(c):
    tag, aux, cur_tag, cur_aux = c.columns()
    heap = np.zeros(1, np.uint8)
    return nxo.publish_commit(c.ids, tag, c.fixed, aux, heap, c.kind, c.to_client, c.slot_of_id,
                              c.client_off, c.client, c.n_clients, cur_tag, c.cur_fixed, cur_aux,
                              heap)


def device_commit(c):
    import torch
    import netidx_amd
    tag, aux, cur_tag, cur_aux = c.columns()
    batch = netidx_amd.columns_from_arrays(c.ids, c.fixed, tag, aux)
    tab = netidx_amd.PubTable(c.slot_of_id, c.client_off, c.client, c.n_clients, cur_tag,
                              c.cur_fixed, cur_aux)
    kind = torch.from_numpy(c.kind.copy()).cuda()
    to = torch.from_numpy(c.to_client.view(np.int32).copy()).cuda()
    return tab, batch, kind, to


@pytest.mark.parametrize("name", fc.COMMIT_CASES)
def test_commit_case(codec, cus, name):
    c = fc.commit_case(name, cus)
    if "stride" in name:  # the pair is one thread's consecutive visits on this device
        pp = fc.pub_plan(c.n_rows, c.n_slots, cus)
        assert pp["strided"] and c.pair[1] - c.pair[0] == pp["stride"], (name, cus, pp)
    want = oracle_commit(c)
    tab, batch, kind, to = device_commit(c)
    d = codec.publish_commit(tab, batch, kind, to)
    check(name, d, want)
    if hasattr(c, "pushed"):  # the repeated row, whichever way the flag could fail
        q = c.pair[1]
        assert bool((want[2] == q).any()) == c.pushed, name
        got = bool((d.ent_row[: d.n_entries] == q).any())
        assert got == c.pushed, f"{name}: row {q} pushed: {got}, expected {c.pushed}"


@pytest.mark.parametrize("n_clients", fc.DIRECTED_CLIENTS)
def test_unsubscribes_at_the_cache_bounds(codec, n_clients):
    import torch
    ids, cl = fc.unsubscribe_case(n_clients)
    off, ent = nxo.publish_unsubscribes(ids, cl, n_clients)
    d = codec.publish_unsubscribes(torch.from_numpy(ids.view(np.int64).copy()).cuda(),
                                   torch.from_numpy(cl.view(np.int32).copy()).cuda(), n_clients)
    case = f"unsubscribes_{n_clients}"
    same(case, "chan_off", d.chan_off.cpu().numpy().view(np.uint64), off)
    assert d.n_entries == len(ent), case
    same(case, "ent_id", d.ent_sub[: d.n_entries].cpu().numpy().view(np.uint64), ent)
    # entry k of client c is that client's k-th pair of the queue
    order = np.flatnonzero(cl < n_clients)
    order = order[np.argsort(cl[order], kind="stable")]
    same(case, "ent_row", d.ent_row[: d.n_entries].cpu().numpy().view(np.uint64), order)


# ---- outputs at exactly their capacities -------------------------------------------------------
def _call(fn, *args):
    """An ABI call with caller-owned outputs: (ok, message)."""
    from netidx_amd.codec import NetidxError, lib
    err = NetidxError()
    ok = bool(fn(*args, C.byref(err)))
    msg = err.msg.decode() if err.msg else ""
    if not ok:
        lib().nxg_error_free(C.byref(err))
    return ok, msg


def _guarded(case, call, n_chans, n_slots, want):
    """`call(out)` at capacity n_entries, at n_entries - 1, and at n_entries again."""
    n = len(want[1])
    full = guards.guarded_dispatch(n_chans, n_slots, n)
    out = full.struct()
    ok, msg = call(out)
    assert ok, f"{case}: {msg}"
    full.n_entries, full.n_unmatched = out.n_entries, out.n_unmatched
    guards.assert_dispatch_guards(full)
    check(case, full, want)
    if n == 0:
        return
    short = guards.guarded_dispatch(n_chans, n_slots, n - 1)
    out = short.struct()
    ok, msg = call(out)
    assert not ok, f"{case}: a call with capacity {n - 1} of {n} succeeded"
    assert f"needs {n} entries" in msg, f"{case}: {msg}"
    assert out.n_entries == n, (case, out.n_entries, n)
    guards.assert_dispatch_guards(short)
    again = guards.guarded_dispatch(n_chans, n_slots, n)
    out = again.struct()
    ok, msg = call(out)
    assert ok, f"{case}: after a failed call: {msg}"
    again.n_entries, again.n_unmatched = out.n_entries, out.n_unmatched
    guards.assert_dispatch_guards(again)
    check(case, again, want)


@pytest.mark.parametrize("name", ["cache_253", "fan_lds", "dup_lds",        # LDS counters
                                  "dup_global", "fan_global", "seg256_global",  # global
                                  "cache_65534", "no_chans", "no_slots"])
def test_dispatch_outputs_stay_within_their_capacities(codec, name):
    from netidx_amd.codec import lib
    c = fc.dispatch_case(name)
    tab, ids = device_case(c)
    tb = tab.c_struct()

    def call(out):
        return _call(lib().nxg_dispatch_updates, codec.ctx, C.byref(tb),
                     C.c_void_p(ids.data_ptr()), c.n_rows, C.byref(out))

    _guarded(name, call, c.n_chans, c.n_slots, oracle_dispatch(name))


@pytest.mark.parametrize("name", ["single_repeat_adjacent-perm-back", "directed_edges_254",
                                  "directed_edges_65534", "slot_bits_31_32"])
def test_commit_outputs_stay_within_their_capacities(codec, cus, name):
    from netidx_amd.codec import lib
    c = fc.commit_case(name, cus)
    tab, batch, kind, to = device_commit(c)
    tb = tab.c_struct()

    def call(out):
        return _call(lib().nxg_publish_commit, codec.ctx, C.byref(tb), C.byref(batch.s),
                     C.c_void_p(0), C.c_void_p(kind.data_ptr()), C.c_void_p(to.data_ptr()),
                     C.byref(out))

    _guarded(name, call, c.n_clients, c.n_slots, oracle_commit(c))
