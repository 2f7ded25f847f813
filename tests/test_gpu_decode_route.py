"""Which decoder a context sends a frame to (finish_decode's hand-overs and its three countdowns),
read through Codec.last_route(): the decoder of the last completed decode and the context's
seq_left, irregular_left and mix_left.

A sequential restatement of the host's choice (Route, below) is stepped beside a default context
over frames of a few thousand records; after every decode the decoder and the countdowns must be
the model's, and the rows the oracle's. The countdown lengths come from nxg_api.cpp
(f64_run_cases.constants()).

Left to other files: tests/test_gpu_f64_seq.py pins that the sequential-id decoder is skipped
after it declined and tried again (its diag[1] mark); tests/test_gpu_f64_enc_seq.py the encoder's
countdown. What they leave open and this file adds: the countdowns' exact values call by call,
the single-pass decoder taking frames directly while irregular_left runs, a sequential-id frame
decoded exactly while it does, a frame that is not f64 leaving irregular_left alone, and
mix_left's value after the fast mixed decoder declined.
"""
import numpy as np
import pytest

import decode_bounds_cases as dbc
import f64_run_cases as fc
import nxo
from guards import assert_guards, guarded_columns

pytestmark = pytest.mark.gpu

K = fc.constants()
LAYOUT_F64, LAYOUT_MIXED = 1, 2


class Route:
    """enqueue_dec_fast + finish_decode for f64 columns: the decoder a frame of `kind` ends on.
    seq: ids count up by one; run: one record length, ids in any order; x: record lengths vary;
    hb: not an f64 frame."""

    def __init__(self):
        self.seq_left = self.irregular_left = 0

    def decode(self, kind):
        rerun = False
        if self.seq_left == 0 and self.irregular_left == 0:
            if kind == "seq":
                return fc.ROUTE_SEQ
            # (hb: the frame's first record is an f64 Update, so the sequential-id decoder
            # reports ids out of order like for any other f64 frame, and is skipped)
            self.seq_left = K["kSeqSkipCalls"]
            rerun = True
        if not rerun and self.seq_left:
            self.seq_left -= 1
        if self.irregular_left == 0:
            if kind == "hb":
                return fc.ROUTE_MIX  # the probe: not f64 (irregular bit 1)
            if kind != "x":
                return fc.ROUTE_RUN
            self.irregular_left = K["kIrregularCalls"]
            return fc.ROUTE_X
        self.irregular_left -= 1
        return fc.ROUTE_MIX if kind == "hb" else fc.ROUTE_X


N = 3000


def _frames():
    rng = np.random.default_rng(11)
    bits = rng.choice([7, 14, 21, 28, 35], N)
    x = rng.integers(0, 2**62, N, dtype=np.uint64) >> (62 - bits).astype(np.uint64)
    ids = {"seq": 1000 + np.arange(N), "run": fc.band_ids(3, N), "x": x}
    out = {}
    for j, (k, i) in enumerate(ids.items()):
        v = fc.safe_values(N, 50 + j)
        out[k] = (fc.frame(i, v), np.asarray(i, np.uint64), v)
    return out


@pytest.fixture(scope="module")
def frames():
    import torch
    out = {}
    for k, (w, i, v) in _frames().items():
        o = nxo.decode(w, cap_rows=N + 1, cap_children=1, cap_ctl=1).trim()
        assert o["err_kind"] == 0 and np.array_equal(o["id"], i) and np.array_equal(o["fixed"], v)
        out[k] = (torch.from_numpy(np.array(w, np.uint8)).cuda(), len(w), i, v)
    assert fc.tile_plan(_frames()["x"][0], flags=0).bails
    assert not fc.tile_plan(_frames()["run"][0], flags=0).bails
    return out


def _decode(codec, frames, kind):
    d, W, ids, vals = frames[kind]
    cols = guarded_columns(N, 1, 1, LAYOUT_F64, "cuda")
    st = codec.decode_into(d, W, cols, check=False)
    assert (st.err_kind, st.n_rows, st.path) == (0, N, 1)
    g = cols.numpy()
    assert np.array_equal(g["id"], ids) and np.array_equal(g["fixed"], vals)
    assert_guards(cols)
    return codec.last_route()


def test_hand_over_to_the_single_pass_decoder_and_back(frames):
    """A frame of random id widths goes seq -> run -> single-pass and arms both countdowns; each
    following f64 decode takes the single-pass decoder directly and counts both down by one; a
    sequential-id frame decoded meanwhile is exact and not on the sequential-id decoder; the
    decode after the countdowns reach 0 tries the sequential-id decoder again."""
    import netidx_amd
    codec, m = netidx_amd.Codec(0), Route()
    try:
        assert codec.last_route() == (0, 0, 0, 0)
        assert _decode(codec, frames, "x") == (m.decode("x"), m.seq_left, m.irregular_left, 0)
        assert (m.seq_left, m.irregular_left) == (K["kSeqSkipCalls"], K["kIrregularCalls"])
        longest = max(K["kSeqSkipCalls"], K["kIrregularCalls"])
        kinds = ["seq", "run", "x"]
        for j in range(longest):
            kind = kinds[j % 3] if m.irregular_left > 1 else "seq"
            want = m.decode(kind)
            got = _decode(codec, frames, kind)
            assert got == (want, m.seq_left, m.irregular_left, 0), (j, kind, got)
            if kind == "seq" and m.irregular_left:
                assert got[0] == fc.ROUTE_X and codec.last_diag()[1] != 1
        assert (m.seq_left, m.irregular_left) == (0, 0)
        got = _decode(codec, frames, "seq")
        assert got == (fc.ROUTE_SEQ, 0, 0, 0) and codec.last_diag()[1] == 1
        # and a frame of one record length with ids out of order: seq declines, run takes it
        got = _decode(codec, frames, "run")
        assert got == (m.decode("run"), m.seq_left, 0, 0) and got[0] == fc.ROUTE_RUN
    finally:
        codec.close()


def test_a_frame_that_is_not_f64_leaves_the_f64_countdown_alone(frames):
    """A Heartbeat where the length-run probe looks for a record start: irregular bit 1, the fast
    mixed decoder's result, irregular_left untouched -- at 0 it stays 0 and the next f64 frame is
    tried on the length-run decoder again; while it runs it counts down by one and the frame
    still ends on the fast mixed decoder. Every step is the Route model's."""
    import netidx_amd
    import torch
    c = fc.BY_NAME["W10-heartbeat"]
    w = fc.wire(c.name)
    o = nxo.decode(np.ascontiguousarray(w), len(c.ids), 1, 1)
    assert (o.s.err_kind, o.s.n_rows, o.s.n_heartbeat) == (0, len(c.ids), 1)
    assert fc.tile_plan(w, flags=0).not_f64
    d = torch.from_numpy(np.array(w, np.uint8)).cuda()
    codec, m = netidx_amd.Codec(0), Route()

    def heartbeat_frame():
        cols = guarded_columns(len(c.ids), 1, 1, LAYOUT_MIXED, "cuda")
        st = codec.decode_into(d, len(w), cols, check=False)
        assert (st.err_kind, st.n_rows, st.n_heartbeat, st.path) == (0, len(c.ids), 1, 4)
        g = cols.numpy()
        assert np.array_equal(g["id"], c.ids) and np.array_equal(g["fixed"], fc.values(c.name))
        assert_guards(cols)
        return codec.last_route()

    try:
        for _ in range(2):
            assert heartbeat_frame() == (m.decode("hb"), m.seq_left, 0, 0)
            assert m.irregular_left == 0
            for kind in ("run", "seq"):
                want = m.decode(kind)
                assert want == fc.ROUTE_RUN
                assert _decode(codec, frames, kind) == (want, m.seq_left, 0, 0)
        # while irregular_left runs
        assert _decode(codec, frames, "x") == (m.decode("x"), m.seq_left, m.irregular_left, 0)
        assert m.irregular_left == K["kIrregularCalls"]
        assert heartbeat_frame() == (m.decode("hb"), m.seq_left, m.irregular_left, 0)
        assert m.irregular_left == K["kIrregularCalls"] - 1
    finally:
        codec.close()


def test_mix_left_counts_after_the_fast_mixed_decoder_declines():
    """The fast mixed decoder declines a frame whose totals exceed a capacity: mix_left is
    kMixFailCalls, each following mixed decode takes the general decoder and counts it down, and
    the decode after it reaches 0 meets the fast decoder again."""
    import netidx_amd
    import torch
    from netidx_amd.codec import Columns
    key = ("flat",)
    w = dbc.wire(key)
    short = [x for x in dbc.cases("fast", key) if x.short][0]
    d = torch.from_numpy(np.array(w, np.uint8)).cuda()
    roomy = Columns.for_frame(len(w), LAYOUT_MIXED, "cuda")
    codec = netidx_amd.Codec(0)
    try:
        assert codec.decode_into(d, len(w), roomy, short.flags).path == 4
        assert codec.last_route() == (fc.ROUTE_MIX, 0, 0, 0)
        cols = guarded_columns(*short.caps, LAYOUT_MIXED, "cuda", max(dbc.need(key)) + 512)
        st = codec.decode_into(d, len(w), cols, short.flags, check=False)
        assert st.err_kind == dbc.CAPACITY
        assert_guards(cols)
        assert codec.last_route() == (fc.ROUTE_GENERAL, 0, 0, K["kMixFailCalls"])
        for j in range(K["kMixFailCalls"]):
            assert codec.decode_into(d, len(w), roomy, short.flags).path == 2
            assert codec.last_route() == (fc.ROUTE_GENERAL, 0, 0, K["kMixFailCalls"] - 1 - j)
        assert codec.decode_into(d, len(w), roomy, short.flags).path == 4
        assert codec.last_route() == (fc.ROUTE_MIX, 0, 0, 0)
    finally:
        codec.close()
