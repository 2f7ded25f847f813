"""The length-run f64 decoder (nxg_decode_f64_run.hip) on the crafted frames of
tests/f64_run_cases.py: every per-tile choice of its probe -- end tile, one run, predicted and
searched two runs, exact tile, the frame bail-outs -- and the emit's sub-wave, edge-lane and
guarded-load paths, each reached by a named case of one to nine tiles.

Every case is decoded into guarded columns (tests/guards.py) sized to the frame's rows and compared
bit for bit with the oracle and with the independent parser (f64_run_cases.records); the tile model
(f64_run_cases.tile_plan) says how many tiles take the exact walk (DevStatus.diag[0]) and whether
the frame is handed over, so a failure names the branch. Contexts, made once for the module:

  run        NXG_F64_PATH=run NXG_F64R_FLAGS=2   never hands a frame over
  run_bail   NXG_F64_PATH=run                    hands over as the bail rule says
  run_exact  NXG_F64_PATH=run NXG_F64R_FLAGS=3   every tile on the exact walk
  default    no variable                         the sequential-id decoder first

Every decode is made twice on the same context (tile descriptors and look-back epochs of the
call before must not show).
"""
import os

import numpy as np
import pytest

import f64_run_cases as fc
import nxo
from guards import assert_guards, guarded_columns

pytestmark = pytest.mark.gpu

LAYOUT_F64, LAYOUT_MIXED = 1, 2
ENV = {"run": {"NXG_F64_PATH": "run", "NXG_F64R_FLAGS": "2"},
       "run_bail": {"NXG_F64_PATH": "run"},
       "run_exact": {"NXG_F64_PATH": "run", "NXG_F64R_FLAGS": "3"},
       "default": {}}
MIXED_COLS = ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off",
              "ctl_len", "ctl_variant")
K = fc.constants()


@pytest.fixture(scope="module")
def ctx_of():
    """context name -> its Codec, made at first use (the environment is read at creation)."""
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    made = {}

    def get(name):
        if name not in made:
            env = ENV[name]
            before = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[name] = netidx_amd.Codec(0)
            finally:
                for k, v in before.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[name]

    yield get
    for c in made.values():
        c.close()


def dev(w):
    import torch
    if len(w) == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.array(np.frombuffer(bytes(w), np.uint8))).cuda()


TINY = fc.frame(fc.band_ids(3, 5), fc.safe_values(5, 1))


def settle(codec):
    """Run down a hand-over countdown left by an earlier case, so that the next decode meets the
    length-run decoder again."""
    from netidx_amd.codec import Columns
    d, cols = dev(TINY), Columns(8, 0, 0, LAYOUT_F64, "cuda")
    for _ in range(K["kIrregularCalls"] + 1):
        if codec.last_route()[2] == 0:
            return
        codec.decode_into(d, len(TINY), cols)
    assert codec.last_route()[2] == 0


def decode_f64(codec, d, w, rec):
    """One decode into exactly sized guarded columns: the rows are the parser's, nothing behind
    them is written. Returns the status."""
    n = len(rec.start)
    cols = guarded_columns(n, 1, 1, LAYOUT_F64, "cuda")
    st = codec.decode_into(d, len(w), cols, check=False)
    assert (st.err_kind, st.n_rows, cols.s.n_rows) == (0, n, n)
    g = cols.numpy()
    assert np.array_equal(g["id"], rec.id), np.flatnonzero(g["id"] != rec.id)[:8]
    assert np.array_equal(g["fixed"], rec.value), np.flatnonzero(g["fixed"] != rec.value)[:8]
    assert_guards(cols)
    return st


CLEAN = [c.name for c in fc.CASES if fc.clean(c)]


@pytest.mark.parametrize("name", CLEAN)
def test_case(ctx_of, name):
    c = fc.BY_NAME[name]
    w = fc.wire(name)
    rec = fc.records(w)
    o = nxo.decode(np.ascontiguousarray(w), cap_rows=len(rec.start) + 1, cap_children=1,
                   cap_ctl=1).trim()
    assert o["err_kind"] == 0
    assert np.array_equal(o["id"], rec.id) and np.array_equal(o["fixed"], rec.value)
    d = dev(w)
    keep = fc.tile_plan(w, flags=fc.F_NO_BAIL)
    verdict = fc.tile_plan(w, flags=0)
    assert keep.tiles[c.tile].cls == c.cls
    what = (name, [t.cls for t in keep.tiles])
    # run: never hands over; the model's exact tiles, no decoder declined
    codec = ctx_of("run")
    for _ in range(2):
        st = decode_f64(codec, d, w, rec)
        assert st.path == 1, what
        assert codec.last_diag()[0] == keep.n_exact, (what, codec.last_diag())
        assert codec.last_status()[0] == 0, what
        assert codec.last_route()[0] == fc.ROUTE_RUN, what
    # run_bail: the model's verdict
    codec = ctx_of("run_bail")
    for _ in range(2):
        settle(codec)
        st = decode_f64(codec, d, w, rec)
        route = codec.last_route()
        assert st.path == 1, what
        if verdict.bails:
            # (DevStatus.irregular == 1 itself is not readable here: last_status() is the status
            # of the final attempt, the single-pass decoder's. Only that value makes the host
            # take the single-pass decoder and arm irregular_left, which is what is asserted.)
            assert (route[0], route[2]) == (fc.ROUTE_X, K["kIrregularCalls"]), (what, route)
        else:
            assert (route[0], route[2]) == (fc.ROUTE_RUN, 0), (what, route)
            assert codec.last_diag()[0] == verdict.n_exact, (what, codec.last_diag())
            assert codec.last_status()[0] == 0, what
    settle(codec)
    # run_exact: every tile on the exact walk; default: whichever decoder the context is on
    codec = ctx_of("run_exact")
    for _ in range(2):
        decode_f64(codec, d, w, rec)
        assert codec.last_diag()[0] == len(keep.tiles), (what, codec.last_diag())
        assert codec.last_route()[0] == fc.ROUTE_RUN and codec.last_status()[0] == 0, what
    codec = ctx_of("default")
    for _ in range(2):
        decode_f64(codec, d, w, rec)


def test_empty_frame(ctx_of):
    rec = fc.records(b"")
    for name in ("run", "default"):
        for _ in range(2):
            st = decode_f64(ctx_of(name), dev(b""), b"", rec)
            assert st.path == 1


def decode_mixed(codec, d, w, caps):
    """One decode into guarded mixed columns, against the oracle's decode into the same
    capacities: (err_kind, err_offset), and every column where the frame is valid."""
    o = nxo.decode(np.ascontiguousarray(w), *caps)
    cols = guarded_columns(*caps, LAYOUT_MIXED, "cuda")
    st = codec.decode_into(d, len(w), cols, check=False)
    print("device", (st.err_kind, st.err_offset, st.n_rows, st.n_children, st.n_ctl), "oracle",
          (o.s.err_kind, o.s.err_offset, o.s.n_rows, o.s.n_children, o.s.n_ctl), "caps", caps)
    assert (st.err_kind, st.err_offset if st.err_kind else 0) == (o.s.err_kind, o.s.err_offset)
    # (a malformed frame is rejected whole and include/nxg_codec.h leaves its counts
    # unspecified: the oracle's n_rows is the rows before the failing message, the device's is
    # what its count passes saw -- 8 and 1000 against the oracle's 7 on these frames -- so n_rows
    # is compared where the frame is valid, below)
    assert_guards(cols)
    if st.err_kind == 0:
        t = o.trim()
        assert (st.n_rows, st.n_children, st.n_ctl) == (len(t["id"]), len(t["ctag"]),
                                                        len(t["ctl_row"]))
        g = cols.numpy()
        for k in MIXED_COLS:
            assert np.array_equal(g[k], t[k]), k
    return st


@pytest.mark.parametrize("name", [c.name for c in fc.CASES if c.corrupt])
def test_malformed_where_the_probe_does_not_look(ctx_of, name):
    """W11: one byte of a record the probe does not sample is corrupted; the run emit's
    per-record check must notice, and the frame comes back as the oracle's: its (err_kind,
    err_offset), or, where the byte makes another valid message of the record, its
    columns and counts. The columns are sized to the frame's rows as the oracle counts them; for
    a frame with an error that is the rows before the failing message and that message's own
    (the oracle claims a row before it reads the message and reports NXG_CAPACITY without it:
    the smallest columns at which the error is the format error). The guard band begins there:
    nothing past the failing message's row is written, by the decoder that reports the error or
    by the run emit that declined before it. The one row inside the capacity may be written:
    what the arrays hold below the capacities of a rejected frame is unspecified."""
    c = fc.BY_NAME[name]
    w = fc.wire(name)
    d = dev(w)
    o = nxo.decode(np.ascontiguousarray(w), len(c.ids) + 1, 8, 8).s
    caps = (int(o.n_rows) + (o.err_kind != 0), max(int(o.n_children), 1), max(int(o.n_ctl), 1))
    sized = nxo.decode(np.ascontiguousarray(w), *caps).s  # a format error comes before capacity
    assert (sized.err_kind, sized.err_offset, sized.n_rows) == (o.err_kind, o.err_offset, o.n_rows)
    assert fc.tile_plan(w, flags=fc.F_NO_BAIL).tiles[0].cls == c.cls
    for ctx in ("run", "default"):
        codec = ctx_of(ctx)
        for _ in range(2):
            decode_mixed(codec, d, w, caps)
            assert codec.last_route()[0] in (fc.ROUTE_MIX, fc.ROUTE_GENERAL), codec.last_route()


def test_window_without_a_record_start_goes_to_the_mixed_decoders(ctx_of):
    """W10: a Heartbeat behind a record that ends 14 bytes into tile 1: the probe finds no record
    start in the tile's first 16 bytes, the frame is not f64 (irregular bit 1) and goes to the
    mixed decoders, not to the single-pass f64 decoder: irregular_left stays 0."""
    c = fc.BY_NAME["W10-heartbeat"]
    w = fc.wire(c.name)
    assert fc.tile_plan(w, flags=0).not_f64
    d = dev(w)
    caps = (len(c.ids), 1, 1)
    for ctx in ("run_bail", "default", "run"):
        codec = ctx_of(ctx)
        settle(codec)
        for _ in range(2):
            st = decode_mixed(codec, d, w, caps)
            route = codec.last_route()
            assert st.err_kind == 0 and st.n_heartbeat == 1 and st.path in (2, 4), (ctx, st.path)
            assert route[0] in (fc.ROUTE_MIX, fc.ROUTE_GENERAL) and route[2] == 0, (ctx, route)
