"""nxg_ctx_sync's status path: the statuses of a backlog reach the host by a gather kernel enqueued
behind the calls (nxg_status.hip) -- by nxg_decode_frames_async for its own frames, by
nxg_ctx_sync for the calls made since -- and one wait. These tests pin, on both paths of
nxg_decode_frames_async (the sequential-id decoder per frame, and NXG_F64_PATH=run's fused
length-run launches):
  - backlogs of 1, 2, 3 and 500 tiny frames, each into its own columns: every column set equals
    the oracle's decode and the returned status is the last frame's; the 500-frame backlog three
    times on one context, so the 1024-slot status ring wraps;
  - single async calls before and after a backlog, completed by one sync;
  - a backlog with an out-of-order id in its middle frame and empty frames at its start, middle
    and end: the declined frame is decoded by a fallback, the others are unaffected.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOT = 128  # bytes per frame in the device buffer (7 records of at most 16 bytes; 16-aligned)


@pytest.fixture(params=["", "run"], ids=["seq", "run"])
def codec(request, monkeypatch):
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    monkeypatch.setenv("NXG_F64_PATH", request.param)
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def _tiny(j):
    """Frame j: 1 + j % 7 records, ids counting up from a start of its own."""
    import nxo
    from netidx_amd import synth
    n = 1 + j % 7
    i0 = (j * 2654435761) % (2**30)
    ids, vals = synth.f64_columns(n, 1000 + j, id_offset=i0)
    return np.frombuffer(bytes(nxo.encode_f64(ids, vals)), np.uint8)


def _oracle(b):
    import nxo
    return nxo.decode(np.ascontiguousarray(b), cap_rows=len(b) + 2, cap_children=len(b) + 2,
                      cap_ctl=len(b) + 2).trim()


@pytest.fixture(scope="module")
def tiny_frames():
    """500 tiny frames in one device buffer, their oracle decodes, and a column set each."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    wires = [_tiny(j) for j in range(500)]
    assert max(len(w) for w in wires) <= SLOT
    host = np.zeros(500 * SLOT, np.uint8)
    for j, w in enumerate(wires):
        host[j * SLOT: j * SLOT + len(w)] = w
    dev = torch.from_numpy(host).cuda()
    refs = [_oracle(w) for w in wires]
    outs = [Columns(8, 0, 0, netidx_amd.LAYOUT_F64, "cuda") for _ in range(500)]
    return dev, [len(w) for w in wires], refs, outs


def _run_backlog(codec, tiny_frames, k):
    import torch
    dev, lens, refs, outs = tiny_frames
    for o in outs[:k]:
        o.id.zero_()
        o.fixed.zero_()
    torch.cuda.synchronize()  # (the codec's stream does not wait for torch's)
    base = dev.data_ptr()
    codec.decode_frames_async([base + j * SLOT for j in range(k)], lens[:k], outs[:k])
    st = codec.sync()
    assert st.err_kind == 0 and st.n_rows == len(refs[k - 1]["id"])
    ids = np.stack([o.id.cpu().numpy().view(np.uint64) for o in outs[:k]])
    fixed = np.stack([o.fixed.cpu().numpy().view(np.uint64) for o in outs[:k]])
    for j in range(k):
        n = len(refs[j]["id"])
        assert outs[j].n_rows == n, j
        assert np.array_equal(ids[j][:n], refs[j]["id"]), j
        assert np.array_equal(fixed[j][:n], refs[j]["fixed"]), j


@pytest.mark.parametrize("k", [1, 2, 3, 500])
def test_backlog_of_tiny_frames(codec, tiny_frames, k):
    _run_backlog(codec, tiny_frames, k)


def test_backlogs_wrap_the_status_ring(codec, tiny_frames):
    for _ in range(3):  # 1,500 calls through a ring of 1,024 slots
        _run_backlog(codec, tiny_frames, 500)


def _frame(n, i0, seed):
    import nxo
    import torch
    from netidx_amd import synth
    ids, vals = synth.f64_columns(n, seed, id_offset=i0)
    w = np.frombuffer(bytes(nxo.encode_f64(ids, vals)), np.uint8)
    return torch.from_numpy(w.copy()).cuda(), _oracle(w)


def _check(cols, ref, what):
    n = len(ref["id"])
    assert cols.n_rows == n, what
    g = cols.numpy()
    assert np.array_equal(g["id"][:n], ref["id"]), what
    assert np.array_equal(g["fixed"][:n], ref["fixed"]), what


def test_single_calls_around_a_backlog_complete_in_one_sync(codec):
    import netidx_amd
    from netidx_amd.codec import Columns
    frames = [_frame(300 + 41 * j, 1000 * j + 7, 50 + j) for j in range(7)]
    outs = [Columns(700, 0, 0, netidx_amd.LAYOUT_F64, "cuda") for _ in range(7)]
    for j in (0, 1):
        codec.decode_async(frames[j][0].data_ptr(), frames[j][0].numel(), outs[j])
    mid = (2, 3, 4)
    codec.decode_frames_async([frames[j][0].data_ptr() for j in mid],
                              [frames[j][0].numel() for j in mid], [outs[j] for j in mid])
    for j in (5, 6):
        codec.decode_async(frames[j][0].data_ptr(), frames[j][0].numel(), outs[j])
    st = codec.sync()
    assert st.err_kind == 0 and st.n_rows == len(frames[6][1]["id"])
    for j in range(7):
        _check(outs[j], frames[j][1], j)


@pytest.mark.parametrize("path", ["", "run"], ids=["seq", "run"])
def test_declined_middle_frame_and_empty_frames(path, monkeypatch):
    import nxo
    import torch
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import Columns
    monkeypatch.setenv("NXG_F64_PATH", path)
    n = 900
    good = [_frame(n, 300 * j + 5, 70 + j) for j in range(4)]
    ids, vals = synth.f64_columns(n, 80, id_offset=4000)
    ids = ids.copy()
    ids[n // 2], ids[n // 2 + 1] = ids[n // 2 + 1], ids[n // 2]
    wb = np.frombuffer(bytes(nxo.encode_f64(ids, vals)), np.uint8)
    bad = (torch.from_numpy(wb.copy()).cuda(), _oracle(wb))
    empty = (None, {"id": np.zeros(0, np.uint64), "fixed": np.zeros(0, np.uint64)})
    backlog = [empty, good[0], good[1], empty, bad, good[2], good[3], empty]
    outs = [Columns(n, 0, 0, netidx_amd.LAYOUT_F64, "cuda") for _ in backlog]
    c = netidx_amd.Codec(0)  # fresh: the sequential-id decoder is tried on every frame
    try:
        c.decode_frames_async([f.data_ptr() if f is not None else 0 for f, _ in backlog],
                              [f.numel() if f is not None else 0 for f, _ in backlog], outs)
        st = c.sync()
        assert st.err_kind == 0 and st.n_rows == 0  # the last frame is empty
        for j, (_, ref) in enumerate(backlog):
            _check(outs[j], ref, j)
        if path == "":
            # the sequential-id decoder declined the middle frame (a fallback decoded it): the
            # context now skips that decoder for a while
            one = Columns(n, 0, 0, netidx_amd.LAYOUT_F64, "cuda")
            st = c.decode_into(good[0][0], good[0][0].numel(), one, 0, check=False)
            assert st.err_kind == 0 and c.last_diag()[1] != 1
            _check(one, good[0][1], "after")
    finally:
        c.close()
