"""One long-lived Codec across calls of different sizes: its grow-on-demand buffers (DevBuf,
netidx_amd/csrc/nxg_devbuf.h) are shared between entry points and regrown in place, so a call
must compute the same after another entry point sized, grew or left the buffer larger.

  - the scratch shared by the routing and archive entry points: dispatch_updates, decode_archive
    and route_writes interleaved at 64 rows, then about 20,000, then 64 again, every result
    bit-identical to the same call on a freshly created Codec;
  - the staged frame of a host-resident decode across its 1 MiB floor: a frame just under it, then
    one just over (one regrow), the columns against the oracle;
  - the staged write columns of a host-resident To decode whose row capacity is 0: they exist on
    a fresh codec as they do after an earlier call grew them;
  - partition_by_tag at two sizes around a doubling of its scratch.

No allocation failure is provoked here: what a failed step leaves behind is pinned on the CPU
(tests/test_devbuf_cpu.py).
"""
import random

import numpy as np
import pytest

import nxo
from test_dispatch_cpu import random_case, table_arrays
from test_gpu_archive import COLS, archive_bytes, gpu_decode
from test_gpu_partition import _check as check_view, _cols as tag_cols
from test_gpu_write_route import rand_items, rand_state, route_all

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


# ---- the three entry points: a case built once, run on any codec, its result as plain data ----
def dispatch_case(n):
    rng = random.Random(n)
    n_ids, n_chans = max(n // 8, 8), 7
    subs, ids = random_case(rng, n, n_ids, n_chans)
    return np.asarray(ids, np.uint64), table_arrays(subs, n_ids)[1:], n_chans


def run_dispatch(codec, case):
    import torch
    import netidx_amd
    ids, arrays, n_chans = case
    tab = netidx_amd.SubTable(*arrays, n_chans)
    d = codec.dispatch_updates(tab, torch.from_numpy(ids.view(np.int64).copy()).cuda())
    return [d.chan_off.cpu().numpy().tobytes(), d.n_entries, d.n_unmatched,
            d.ent_sub[: d.n_entries].cpu().numpy().tobytes(),
            d.ent_row[: d.n_entries].cpu().numpy().tobytes(), d.last_row.cpu().numpy().tobytes()]


def archive_case(n):
    from netidx_amd import synth
    return archive_bytes(synth.archive_columns(n, seed=n % 97))


def run_archive(codec, buf):
    cols, st, used = gpu_decode(codec, buf)
    g = cols.numpy()
    return [st.err_kind, st.err_offset, st.n_rows, st.n_children, st.path, used] + \
           [g[k].tobytes() for k in COLS]


def writes_case(n):
    rng = random.Random(n + 1)
    n_ids = max(n // 4, 16)
    return rand_state(rng, n_ids, 5), rand_items(rng, n, n // 16 + 3, n_ids), n_ids


def run_writes(codec, case):
    st, items, n_ids = case
    got, stops = route_all(codec, st, items, n_ids, 5, fresh=1 << 40)
    return [got.outcome, bytes(got.reply), got.n_replies, got.wait, got.unsub, got.n_fresh,
            got.n_outcome, {c: [tuple(e) for e in v] for c, v in got.batches.items()}, stops,
            got.calls]


ENTRY_POINTS = (("dispatch_updates", dispatch_case, run_dispatch),
                ("decode_archive", archive_case, run_archive),
                ("route_writes", writes_case, run_writes))


def test_shared_scratch_small_large_small(codec):
    import netidx_amd
    sizes = (64, 20_000, 64)
    cases = {n: [make(n) for _, make, _ in ENTRY_POINTS] for n in set(sizes)}
    fresh = {}
    for n in cases:  # every call on a codec of its own, which nothing else has sized
        for (name, _, run), case in zip(ENTRY_POINTS, cases[n]):
            c = netidx_amd.Codec(0)
            fresh[name, n] = run(c, case)
            c.close()
    assert fresh["decode_archive", 20_000][2] == 20_000  # (rows: the case is what it claims)
    for step, n in enumerate(sizes):
        for (name, _, run), case in zip(ENTRY_POINTS, cases[n]):
            assert run(codec, case) == fresh[name, n], (name, n, step)


# ---- the staged frame across its floor ---------------------------------------------------------
def f64_wire_of_at_most(limit):
    """(ids, vals, wire): the longest f64 frame of consecutive rows of at most `limit` bytes."""
    rng = np.random.default_rng(limit)
    ids = rng.permutation(limit // 8).astype(np.uint64)  # (more rows than fit)
    vals = rng.integers(0, 2**64, len(ids), dtype=np.uint64)
    lo, hi = 0, len(ids)  # the frame of lo rows fits, that of hi rows does not
    assert len(nxo.encode_f64(ids, vals)) > limit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(nxo.encode_f64(ids[:mid], vals[:mid])) <= limit:
            lo = mid
        else:
            hi = mid
    return ids[:lo], vals[:lo], nxo.encode_f64(ids[:lo], vals[:lo])


def test_host_frame_across_the_staging_floor():
    """The staging buffer holds the frame and 16 spare bytes and starts at 1 MiB: a frame of just
    under 1 MiB - 16 bytes fits the floor, the next one, a few records longer, regrows it once."""
    import netidx_amd
    from netidx_amd.codec import Columns
    codec = netidx_amd.Codec(0)  # (of its own: nothing has staged a larger frame on it)
    under = f64_wire_of_at_most(MIB - 16)
    over = f64_wire_of_at_most(MIB + 64)
    assert MIB - 16 - 32 < len(under[2]) <= MIB - 16 < len(over[2]) <= MIB + 64
    for ids, vals, wire in (under, over, under):
        out = Columns(len(ids), 0, 0, netidx_amd.LAYOUT_F64, "cuda")
        st = codec.decode_into(np.asarray(wire), len(wire), out)  # host memory: staged
        assert st.err_kind == 0 and st.n_rows == len(ids)
        o = nxo.decode(np.asarray(wire).tobytes()).trim()
        g = out.numpy()
        assert np.array_equal(g["id"], o["id"]) and np.array_equal(g["fixed"], o["fixed"])
        assert np.array_equal(g["id"], ids) and np.array_equal(g["fixed"], vals)
    codec.close()


# ---- staged write columns of capacity 0 ----------------------------------------------------------
@pytest.mark.parametrize("fast", (False, True))
def test_host_write_columns_of_capacity_zero_on_a_fresh_codec(fast):
    """A To frame of Unsubscribes only, into pinned host columns whose row capacity is 0, on a
    codec that never staged write columns: the staged pair must exist all the same (the
    decoders refuse null write columns), so the call succeeds, as it does after an earlier call
    grew the pair. The Python classes round capacities up to 1, so the structs say 0 here."""
    import netidx_amd
    import to_twin as tw
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    wire = tw.unsubscribe(3) + tw.unsubscribe(500_000)
    got = []
    for warm, cap in ((False, 1), (False, 0), (True, 0)):  # (the first: the reference)
        codec = netidx_amd.Codec(0)
        if warm:  # an earlier call with rows has grown the staged pair
            codec.decode_writes(tw.write(7, True, (12, b"text"), 11),
                                Columns(4, 4, 4, LAYOUT_MIXED, "cpu"), WriteCols(4, "cpu"),
                                fast=fast)
        cols, wcols = Columns(1, 1, 4, LAYOUT_MIXED, "cpu"), WriteCols(1, "cpu")
        cols.s.cap_rows = wcols.s.cap_rows = cap  # (the arrays hold one row: nothing overruns)
        codec.decode_writes(wire, cols, wcols, fast=fast)
        assert (cols.s.n_rows, cols.s.n_ctl) == (0, 2)
        g = cols.numpy()
        got.append([g[k].tolist() for k in ("ctl_row", "ctl_off", "ctl_len", "ctl_variant")])
        codec.close()
    assert got[0] == got[1] == got[2]
    e, _ = tw.decode(wire)  # (the twin's control spans: row, offset, length, variant)
    assert got[0] == [[int(r[k]) for r in e.ctl] for k in range(4)]


# ---- partition_by_tag around a doubling --------------------------------------------------------
def test_partition_around_a_doubling():
    """Its scratch (1 KiB per tile of 4096 rows and 4168 bytes) doubles or takes the need,
    whichever is larger: 8 tiles (12,360 bytes); 12 tiles (16,456: less than twice, so the buffer
    doubles to 24,720); 19 tiles (23,624: inside the doubled buffer, past the need that made it);
    30 tiles (34,888: more than twice); 8 tiles again."""
    import netidx_amd
    codec = netidx_amd.Codec(0)
    rng = np.random.default_rng(17)
    for n in (30_000, 47_000, 75_000, 120_000, 30_000):
        tag = rng.integers(0, 28, n).astype(np.uint8)
        fixed = rng.integers(0, 2**64, n, dtype=np.uint64)
        aux = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        check_view(codec.partition_by_tag(tag_cols(tag, fixed, aux)), tag, fixed, aux)
    codec.close()
