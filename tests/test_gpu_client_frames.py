"""nxg_encode_clients on the GPU: client_off and every byte against the model of
tests/client_frames_model.py, on the cases of tests/client_frames_cases.py (both layouts where
the values allow F64), chained with the commit, and under guard bands."""
import functools
import random

import numpy as np
import pytest

import client_frames_cases as cfc
import client_frames_model as model
from guards import (SENTINEL, assert_outside_untouched, guarded_buffer, out_ptr, written)

pytestmark = pytest.mark.gpu
MAX_BATCH = 0x3FFFFFFF
LAYOUTS = ("f64", "mixed")
SPARE = 512  # guard elements on both sides of client_off


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def device_batch(cols, layout, heap=None):
    """(Columns, device heap) of a case's numpy columns in the layout."""
    import torch
    import netidx_amd
    if layout == "f64":
        batch = netidx_amd.columns_from_arrays(cols["id"], cols["fixed"])
    else:
        batch = netidx_amd.columns_from_arrays(cols["id"], cols["fixed"], cols["tag"], cols["aux"],
                                               cols.get("ctag"), cols.get("cfixed"),
                                               cols.get("caux"))
    dheap = None
    if heap is not None and len(heap):
        dheap = torch.from_numpy(np.ascontiguousarray(heap).copy()).cuda()
    return batch, dheap


def device_dispatch(chan_off, ent_row):
    import torch
    from netidx_amd.codec import Dispatch
    co = torch.from_numpy(np.asarray(chan_off, np.uint64).view(np.int64).copy()).cuda()
    er = torch.from_numpy(np.asarray(ent_row, np.uint64).view(np.int64).copy()).cuda()
    return Dispatch(co, None, er, None, len(ent_row), 0)


def guarded_offsets(n_clients):
    """client_off[n_clients + 1] with SPARE sentinel elements on both sides: (whole, view)."""
    import torch
    whole = torch.full(((n_clients + 1 + 2 * SPARE) * 8,), SENTINEL, dtype=torch.uint8,
                       device="cuda").view(torch.int64)
    torch.cuda.synchronize()
    return whole, whole[SPARE:SPARE + n_clients + 1]


def assert_offset_guards(whole, n_clients):
    b = whole.cpu().numpy().view(np.uint8)
    assert np.all(b[:SPARE * 8] == SENTINEL), "an element before client_off[0] was written"
    assert np.all(b[(SPARE + n_clients + 1) * 8:] == SENTINEL), \
        "an element behind client_off[n_clients] was written"


@functools.lru_cache(maxsize=None)
def want_of(layout, name):
    c = cfc.cases(layout)[name]
    return model.expected(c.cols, c.heap, c.chan_off, c.ent_row)


def host(t):
    return t.cpu().numpy()


def check_call(codec, batch, dheap, d, want, woff):
    """The size-only form, then the writing form into a guarded buffer of exactly the size."""
    n, off = codec.encoded_clients_len(batch, d, dheap)
    assert n == len(want)
    assert np.array_equal(host(off).view(np.uint64), woff)
    nc = len(woff) - 1
    whole, view = guarded_offsets(nc)
    buf = guarded_buffer(len(want), 0)
    m, off2 = codec.encode_clients_into(batch, d, dheap, out_ptr(buf, 0), len(want), view)
    assert m == len(want)
    assert np.array_equal(host(off2).view(np.uint64), woff)
    got = written(buf, 0, len(want)).tobytes()
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"byte {at} of {len(want)} differs: {g[at]} != {w[at]}")
    assert_outside_untouched(buf, 0, len(want))
    assert_offset_guards(whole, nc)


def case_params():
    return [(l, n) for l in LAYOUTS for n in cfc.cases(l)]


@pytest.mark.parametrize("layout,name", case_params())
def test_case_matches_model(codec, layout, name):
    c = cfc.cases(layout)[name]
    want, woff = want_of(layout, name)
    batch, dheap = device_batch(c.cols, layout, c.heap)
    check_call(codec, batch, dheap, device_dispatch(c.chan_off, c.ent_row), want, woff)


@pytest.mark.parametrize("name", ["count_1", "edges", "varint_ids", "one_row_3000", "overflow"])
def test_f64_values_in_the_mixed_layout(codec, name):
    """The F64 cases (tiles of the F64 kernel's size) through the mixed kernel too."""
    c = cfc.cases("f64")[name]
    want, woff = want_of("f64", name)
    batch, dheap = device_batch(c.cols, "mixed", c.heap)
    check_call(codec, batch, dheap, device_dispatch(c.chan_off, c.ent_row), want, woff)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_with_encode_batch(codec, layout):
    """One client with entries 0..n-1 gives exactly encode_batch(batch)."""
    c = cfc.cases(layout)["one_client"]
    batch, dheap = device_batch(c.cols, layout, c.heap)
    whole = host(codec.encode_batch(batch, dheap)).tobytes()
    got, off = codec.encode_clients(batch, device_dispatch(c.chan_off, c.ent_row), dheap)
    assert host(got).tobytes() == whole
    assert host(off).view(np.uint64).tolist() == [0, len(whole)]


def test_containers_after_commit(codec):
    """Array, Map and Error(Value) three deep, Decimal and Abstract: commit on the GPU, encode,
    compare with the model (gathered rows share the batch's children).

    The commit's values also hold tag 17 (about one row in twenty, at the top or nested), which
    commit compares but no encoder writes: the oracle refuses such a row with UnknownTag. So the
    commit's own entry list must fail with that kind, as the oracle does, and the byte comparison
    runs on the entries whose rows the oracle encodes (the oracle decides, row by row)."""
    import netidx_amd
    from test_gpu_publish import gpu_commit_values
    from test_publish_values_cpu import case_arrays, random_case
    rng = random.Random(71)
    rows, kind, to_client, by_id, slot_ids = random_case(rng, 2000, 30, 5)
    a = case_arrays(rows, kind, to_client, by_id, slot_ids, 30)
    d = gpu_commit_values(codec, a, 5)
    assert d.n_entries > 1000
    ct, cf, ca = a["children"]
    cols = {"id": a["ids"], "tag": a["tag"], "fixed": a["fixed"], "aux": a["aux"], "ctag": ct,
            "cfixed": cf, "caux": ca}
    chan_off = host(d.chan_off).view(np.uint64).astype(np.int64)
    ent_row = host(d.ent_row[: d.n_entries]).view(np.uint64).astype(np.int64)
    batch, dheap = device_batch(cols, "mixed", a["heap"])

    def encodes(r):
        try:
            model.client_payload(cols, a["heap"], [r])
            return True
        except ValueError as e:
            assert str(e) == "encode error 1", (r, e)
            return False

    ok = np.array([encodes(r) for r in range(len(rows))])
    assert 0 < (~ok).sum() < len(rows) // 10 and not ok[ent_row].all()
    with pytest.raises(netidx_amd.CodecError, match="PackError kind 1"):
        codec.encode_clients(batch, d, dheap)
    keep = ok[ent_row]
    client = np.repeat(np.arange(5), np.diff(chan_off))
    kept_off = np.concatenate([[0], np.cumsum(np.bincount(client[keep], minlength=5))])
    kept_row = ent_row[keep]
    assert len(kept_row) > 1000
    for t in (19, 20, 21, 22, 27):
        assert t in set(a["tag"][kept_row].tolist())
    want, woff = model.expected(cols, a["heap"], kept_off, kept_row)
    check_call(codec, batch, dheap, device_dispatch(kept_off, kept_row), want, woff)


def encodable(v):
    """The value tree with every tag-17 scalar (compared by the commit, written by no encoder)
    turned into a Null."""
    if v[0] == "sc":
        return ("sc", 16, 0, 0) if v[1] == 17 else v
    if v[0] == "arr":
        return ("arr", [encodable(x) for x in v[1]])
    if v[0] == "map":
        return ("map", [(k, encodable(x)) for k, x in v[1]])
    if v[0] == "err":
        return ("err", encodable(v[1]))
    return v


def test_containers_chain_unfiltered(codec):
    """The same trees with their tag-17 leaves made Null, so that every row encodes: the commit's
    own chan_off and ent_row tensors go straight into the encode, and every byte is compared."""
    from test_gpu_publish import gpu_commit_values
    from test_publish_values_cpu import case_arrays, random_case
    rng = random.Random(72)
    rows, kind, to_client, by_id, slot_ids = random_case(rng, 2000, 30, 5)
    rows = [(i, encodable(v)) for i, v in rows]
    by_id = {i: [cl, encodable(v)] for i, (cl, v) in by_id.items()}
    a = case_arrays(rows, kind, to_client, by_id, slot_ids, 30)
    d = gpu_commit_values(codec, a, 5)
    assert d.n_entries > 1000
    ct, cf, ca = a["children"]
    cols = {"id": a["ids"], "tag": a["tag"], "fixed": a["fixed"], "aux": a["aux"], "ctag": ct,
            "cfixed": cf, "caux": ca}
    ent_row = host(d.ent_row[: d.n_entries]).view(np.uint64)
    for t in (19, 20, 21, 22, 27):
        assert t in set(a["tag"][ent_row.astype(np.int64)].tolist())
    want, woff = model.expected(cols, a["heap"], host(d.chan_off).view(np.uint64), ent_row)
    batch, dheap = device_batch(cols, "mixed", a["heap"])
    check_call(codec, batch, dheap, d, want, woff)


@pytest.mark.parametrize("seed,n_rows,n_ids,n_clients", [
    (23, 300, 20, 4), (24, 5000, 50, 7), (27, 100000, 70000, 1025)])
def test_chained_with_commit(codec, seed, n_rows, n_ids, n_clients):
    """publish_commit, then encode_clients; every non-empty client's payload decodes to its
    gathered columns."""
    import netidx_amd
    from netidx_amd.codec import Columns
    from test_gpu_publish import gpu_commit
    from test_publish_cpu import arrays, random_case
    rng = random.Random(seed)
    rows, kind, to_client, by_id, slot_ids, heap = random_case(rng, n_rows, n_ids, n_clients)
    a = arrays(rows, kind, to_client, by_id, slot_ids, n_ids)
    ids, tag, fixed, aux = a[:4]
    d = gpu_commit(codec, a, heap, n_clients)
    cols = {"id": ids, "tag": tag, "fixed": fixed, "aux": aux}
    batch, dheap = device_batch(cols, "mixed", heap)
    payload, off = codec.encode_clients(batch, d, dheap)
    off = host(off).view(np.uint64).astype(np.int64)
    chan_off = host(d.chan_off).view(np.uint64).astype(np.int64)
    ent_row = host(d.ent_row[: d.n_entries]).view(np.uint64).astype(np.int64)
    assert off[0] == 0 and off[-1] == payload.numel() and d.n_entries > 0
    wire = host(payload)
    longest = int(np.diff(off).max())
    out = Columns.for_frame(longest, netidx_amd.LAYOUT_MIXED, "cuda")
    seen = 0
    for c in range(n_clients):
        seg = ent_row[chan_off[c]:chan_off[c + 1]]
        if not len(seg):
            assert off[c + 1] == off[c]
            continue
        frame = payload[off[c]:off[c + 1]].clone()  # (an allocation of its own: aligned)
        st = codec.decode_into(frame, frame.numel(), out)
        assert st.n_rows == len(seg)
        r = out.numpy()
        assert np.array_equal(r["id"], ids[seg]) and np.array_equal(r["tag"], tag[seg])
        assert np.array_equal(r["aux"], aux[seg])
        text = tag[seg] == 12
        # (True, False and Null are their tag alone: `fixed` is not on the wire)
        plain = ~text & ~np.isin(tag[seg], (14, 15, 16))
        assert np.array_equal(r["fixed"][plain], fixed[seg][plain])
        fw = wire[off[c]:off[c + 1]]
        for k in np.flatnonzero(text & (aux[seg] > 0)):
            o, n = int(r["fixed"][k]), int(aux[seg][k])
            src = int(fixed[seg][k])
            assert fw[o:o + n].tobytes() == heap[src:src + n].tobytes()
        seen += len(seg)
    assert seen == d.n_entries


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bounds_at_every_phase(codec, layout):
    """The output at each of the 16 byte phases with an exact, a one-short and a zero capacity;
    client_off guarded on both sides. Nothing outside is touched whether the call succeeds or
    fails, a short call reports the need, and a clean encode follows each failure."""
    import netidx_amd
    c = cfc.cases(layout)["overflow"]  # a direct-path tile beside a staged one
    want, woff = want_of(layout, "overflow")
    batch, dheap = device_batch(c.cols, layout, c.heap)
    d = device_dispatch(c.chan_off, c.ent_row)
    n, nc = len(want), c.n_clients
    for phase in range(16):
        for cap in (n, n - 1, 0):
            buf = guarded_buffer(cap, phase)
            whole, view = guarded_offsets(nc)
            if cap == n:
                m, off = codec.encode_clients_into(batch, d, dheap, out_ptr(buf, phase), cap, view)
                assert m == n and written(buf, phase, n).tobytes() == want
                assert np.array_equal(host(off).view(np.uint64), woff)
            else:
                with pytest.raises(netidx_amd.CodecError, match="too small") as e:
                    codec.encode_clients_into(batch, d, dheap, out_ptr(buf, phase), cap, view)
                assert e.value.n_bytes == n, (phase, cap, e.value.n_bytes)
            assert_outside_untouched(buf, phase, cap)
            assert_offset_guards(whole, nc)
            if cap != n:  # the ctx is clean after a failure
                got, off = codec.encode_clients(batch, d, dheap)
                assert host(got).tobytes() == want


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refusals(codec, layout):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    T = cfc.tile_size(layout)
    c = cfc.cases(layout)["edges"]
    want, woff = want_of(layout, "edges")
    batch, dheap = device_batch(c.cols, layout, c.heap)
    n_rows = len(c.cols["id"])
    # an entry that names row n_rows: refused, with the guards intact
    bad = c.ent_row.copy()
    bad[T + 1] = n_rows
    buf = guarded_buffer(len(want), 0)
    whole, view = guarded_offsets(c.n_clients)
    with pytest.raises(netidx_amd.CodecError, match=rf"entry {T + 1} names a row"):
        codec.encode_clients_into(batch, device_dispatch(c.chan_off, bad), dheap, out_ptr(buf, 0),
                                  len(want), view)
    assert_outside_untouched(buf, 0, len(want))
    assert_offset_guards(whole, c.n_clients)
    with pytest.raises(netidx_amd.CodecError, match="names a row"):
        codec.encoded_clients_len(batch, device_dispatch(c.chan_off, bad), dheap)
    # chan_off that decreases, ends short of n_entries, or ends past it
    E = len(c.ent_row)
    for co in ([0, T, T - 1, T + 1, E], [0, T - 1, T, T + 1, E - 1], [0, T - 1, T, T + 1, E + 1],
               [0, E, 0, E, E]):
        dd = device_dispatch(co, c.ent_row)
        whole, view = guarded_offsets(c.n_clients)
        with pytest.raises(netidx_amd.CodecError, match="not a dispatch's"):
            codec.encode_clients_into(batch, dd, dheap, None, 0, view)
        assert_offset_guards(whole, c.n_clients)
    d = device_dispatch(c.chan_off, c.ent_row)
    # control messages
    batch.s.n_ctl = 1
    with pytest.raises(netidx_amd.CodecError, match="control messages"):
        codec.encode_clients(batch, d, dheap)
    batch.s.n_ctl = 0
    # out in host memory
    hout = np.zeros(len(want) + 16, np.uint8)
    with pytest.raises(netidx_amd.CodecError, match="device memory"):
        codec.encode_clients_into(batch, d, dheap, hout.ctypes.data, len(want))
    # a pending async call
    from netidx_amd import synth
    ids, vals = synth.f64_columns(100)
    frame = codec.encode_batch(netidx_amd.columns_from_arrays(ids, vals))
    out = Columns(100, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
    codec.decode_async(frame.data_ptr(), frame.numel(), out)
    try:
        with pytest.raises(netidx_amd.CodecError, match="pending"):
            codec.encode_clients(batch, d, dheap)
    finally:
        codec.sync()
    # and the ctx still encodes
    got, off = codec.encode_clients(batch, d, dheap)
    assert host(got).tobytes() == want and np.array_equal(host(off).view(np.uint64), woff)
    torch.cuda.synchronize()


def test_max_batch_per_client(codec):
    """Client 1 of 3 has 1100 entries of a 1 MiB Bytes value: more than MAX_BATCH. The size-only
    call reports the lengths; the writing call fails naming the client and writes nothing."""
    import torch
    import netidx_amd
    blen = 1 << 20
    cols, heap = cfc._text_rows([5], [blen], tag=13)
    case = cfc.Case("max_batch", cols, heap, [0, 0, 1100, 1100], np.zeros(1100, np.uint64))
    one = int(cfc.msg_lens(case)[0])
    assert one == len(netidx_amd.msg_update(5, 13, 0, blen, bytes(heap[:blen])))
    assert 1100 * one > MAX_BATCH
    batch, dheap = device_batch(cols, "mixed", heap)
    d = device_dispatch(case.chan_off, case.ent_row)
    n, off = codec.encoded_clients_len(batch, d, dheap)
    assert n == 1100 * one
    assert host(off).view(np.uint64).tolist() == [0, 0, 1100 * one, 1100 * one]
    big = torch.empty(1200 << 20, dtype=torch.uint8, device="cuda")
    big[: 1 << 20] = SENTINEL
    torch.cuda.synchronize()
    with pytest.raises(netidx_amd.CodecError, match=rf"client 1's payload of {1100 * one} bytes") as e:
        codec.encode_clients_into(batch, d, dheap, big.data_ptr(), big.numel())
    assert "nxg_encode_frames" in str(e.value)
    assert bool((big[: 1 << 20] == SENTINEL).all())


def test_commit_shape_1e6(codec):
    """bench.py's commit shape at 10^6 rows and 16 clients (about 1.1 * 10^6 entries), every byte
    against the model."""
    import torch
    import netidx_amd
    s = cfc.commit_shape(1_000_000)
    tab = netidx_amd.PubTable(s.slot_of_id, s.off, s.client, s.n_clients, None, s.cur)
    batch = netidx_amd.columns_from_arrays(s.ids, s.vals)
    d = codec.publish_commit(tab, batch, torch.from_numpy(s.kind).cuda(), cap=int(s.off[-1]))
    assert d.n_entries > 1_000_000
    want, woff = model.expected(model.f64_cols(s.ids, s.vals), None,
                                host(d.chan_off).view(np.uint64),
                                host(d.ent_row[: d.n_entries]).view(np.uint64))
    got, off = codec.encode_clients(batch, d)
    assert np.array_equal(host(off).view(np.uint64), woff)
    assert np.array_equal(host(got), np.frombuffer(want, np.uint8))
