"""Decoders at the edge of their columns: capacities equal to what a frame needs, and smaller.

Every case of tests/decode_bounds_cases.py is decoded into guarded columns (tests/guards.py: each
array holds a band of sentinel elements behind its capacity) and compared with the oracle's decode
of the same frame into the same capacities (nxo.decode(wire, cap_rows=, cap_children=, cap_ctl=)):

  - err_kind is NXG_CAPACITY exactly where the oracle's is, and 0 otherwise (an archive batch:
    err_offset too);
  - no element at or behind any capacity changed, whatever the outcome;
  - where the outcome is 0, the counts and every column equal the oracle's;
  - where it is NXG_CAPACITY, n_rows, n_children and n_ctl are what the frame needs;
  - after a capacity error the same context decodes the same frame into exactly sized guarded
    columns, equal to the oracle's (a kernel that declined makes the context skip it for some
    calls: that must not show in the result);
  - a backlog (nxg_decode_frames_async) whose middle frame's columns are one row short reports that
    frame's error, leaves the two other frames' columns equal to the oracle's and all three bands
    intact.

What the arrays below the capacities hold after NXG_CAPACITY is not asserted. The band is as long
as the frame's whole need plus 512 elements, so even a decoder that ignored its capacity would
write memory the test owns. One context per decoder choice, made once for the module:

  seq      the sequential-id f64 decoder (the default for f64 frames), nxg_decode_f64_seq.hip
  run      NXG_F64_PATH=run, the length-run decoder, nxg_decode_f64_run.hip, with
           NXG_F64R_FLAGS=2 (it never hands a frame over to the single-pass decoder, which it
           otherwise does for the one-byte ids in permuted order here, and then for the next 64
           calls); its tiles of one-byte ids go through the exact walk, those of three-byte ids
           through the run emit, and DevStatus.diag[0] (the exact tiles) is asserted for both
  x        NXG_F64_PATH=x, the single-pass decoder, nxg_decode_f64_x.hip
  fast     the fast mixed decoder (NXG_DECODE_HINT_MIXED), nxg_decode_mixed.hip; it declines a
           frame whose totals exceed a capacity and the general decoder reports the error
  general  NXG_MIXED_PATH=general, nxg_decode_gen.hip
  host     pinned-host columns (NXG_MEM_HOST): the ctx decodes into device columns of its own and
           copies back what fits
  archive  nxg_decode_archive_batch: the fast path and NXG_ARCH_PATH=exact
The 256 MiB instantiation of the sequential-id kernel is left to the full-size tests.
"""
import os

import numpy as np
import pytest

import decode_bounds_cases as dbc
import f64_run_cases
import nxo
from guards import assert_guards, guarded_columns

pytestmark = pytest.mark.gpu

ENV = {"seq": {}, "run": {"NXG_F64_PATH": "run", "NXG_F64R_FLAGS": "2"},
       "x": {"NXG_F64_PATH": "x"}, "fast": {}, "general": {"NXG_MIXED_PATH": "general"},
       "host": {}, "archive_fast": {}, "archive_exact": {"NXG_ARCH_PATH": "exact"}}
MIXED_COLS = ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux", "ctl_row", "ctl_off",
              "ctl_len", "ctl_variant")
# calls for which a context skips the fast mixed decoder after it declined (nxg_api.cpp)
MIX_FAIL_CALLS = f64_run_cases.constants()["kMixFailCalls"]


@pytest.fixture(scope="module")
def ctx_of():
    """decoder name -> its context, made at first use (the environment is read at creation)."""
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
    return torch.from_numpy(np.ascontiguousarray(w)).cuda()


def spare_for(nd):
    return max(nd) + 512


def assert_columns(cols, o, st=None, names=MIXED_COLS):
    """The counts and the columns up to the counts equal the oracle's decode `o`."""
    t = o.trim()
    want = (len(t["id"]), len(t["ctag"]), len(t["ctl_row"]))
    assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == want
    if st is not None:
        assert (st.n_rows, st.n_children, st.n_ctl) == want
    g = cols.numpy()
    for k in names:
        assert np.array_equal(g[k], t[k]), k
    if "ctl_row" in names:
        assert cols.s.n_heartbeat == t["n_heartbeat"]


def run_case(codec, c, device="cuda"):
    """Decode the case's frame into guarded columns of its capacities; the outcome is the
    oracle's, the bands are intact, a decoded frame equals the oracle's. Returns the status."""
    w = dbc.wire(c.frame)
    cols = guarded_columns(*c.caps, c.layout, device, spare_for(dbc.need(c.frame)))
    st = codec.decode_into(dev(w), len(w), cols, c.flags, check=False)
    o = nxo.decode(w, *c.caps)
    what = (c.decoder, c.frame, c.label)
    assert o.s.err_kind == (dbc.CAPACITY if c.short else 0), what
    assert st.err_kind == o.s.err_kind, what
    assert_guards(cols)
    if st.err_kind == 0:
        f64 = c.layout == dbc.LAYOUT_F64
        assert_columns(cols, o, st, ("id", "fixed") if f64 else MIXED_COLS)
    else:
        assert_counts_are_the_need(cols, st, c.frame)
    return st


def assert_counts_are_the_need(cols, st, key):
    """After NXG_CAPACITY the counts are what the frame needs (include/nxg_codec.h), so that a
    caller can size its columns from them."""
    nd = dbc.need(key)
    assert (cols.s.n_rows, cols.s.n_children, cols.s.n_ctl) == nd, key
    if st is not None:
        assert (st.n_rows, st.n_children, st.n_ctl) == nd, key


def exact_of(c):
    nd = dbc.need(c.frame)
    caps = (nd[0], 1, 1) if c.layout == dbc.LAYOUT_F64 else nd
    return c._replace(caps=caps, short=False, label="exact_again")


F64 = [(d, k) for d in ("seq", "run", "x") for k in dbc.frames_of(d)]


@pytest.mark.parametrize("decoder,key", F64,
                         ids=[d + ":" + "-".join(map(str, k[1:])) for d, k in F64])
def test_f64_decoder_at_and_below_capacity(ctx_of, decoder, key):
    codec = ctx_of(decoder)
    for c in dbc.cases(decoder, key):
        st = run_case(codec, c)
        if c.short:
            st = run_case(codec, exact_of(c))
        assert st.err_kind == 0 and st.path == 1, c
        diag = codec.last_diag()
        if decoder == "seq":  # (a capacity miss is no hand-over: the kernel stays in use)
            assert diag[1] == 1, c
        elif decoder == "run":
            # the context never hands over, so path 1 is the length-run decoder's; diag[0] counts
            # its tiles on the exact walk: every tile of one-byte ids past 127 records, and none
            # of three-byte ids, which the run emit writes
            starts = np.bincount(12 * np.arange(key[1]) // 32768)  # record starts per tile
            exact = 0 if key[0] == "run14" else int((starts > 127).sum())
            assert diag[0] == exact, (c, diag)
            assert diag[2] == 0, (c, diag)
        else:  # the single-pass decoder marks the entry of the range it decoded (+1)
            assert diag[2] == 1, (c, diag)


MIXED = [("fast", ("flat",)), ("general", ("flat",)), ("general", ("rich",))]


@pytest.mark.parametrize("decoder,key", MIXED, ids=[f"{d}-{k[0]}" for d, k in MIXED])
def test_mixed_decoder_at_and_below_capacity(ctx_of, decoder, key):
    from netidx_amd.codec import Columns
    codec = ctx_of(decoder)
    w = dbc.wire(key)
    frame, roomy = dev(w), Columns.for_frame(len(w), dbc.LAYOUT_MIXED, "cuda")
    for c in dbc.cases(decoder, key):
        st = run_case(codec, c)
        if not c.short:
            assert st.path == (4 if decoder == "fast" else 2), c
            continue
        st = run_case(codec, exact_of(c))
        if decoder == "fast":
            # the fast decoder it was that declined: the context skips it now; run the skip down,
            # so that the next case meets the fast decoder again
            assert st.path == 2, c
            for _ in range(MIX_FAIL_CALLS):
                assert codec.decode_into(frame, len(w), roomy, c.flags).err_kind == 0


@pytest.mark.parametrize("decoder", ["seq", "run"])
def test_backlog_middle_frame_one_row_short(ctx_of, decoder):
    """seq: the backlog call makes one nxg_decode_updates_async call per frame; run: the frames are
    pipelined through the length-run decoder, each with its own capacity."""
    codec = ctx_of(decoder)
    jobs = dbc.backlog_cases()[decoder]
    frames = [dev(dbc.wire(k)) for k, _, _ in jobs]
    cols = [guarded_columns(*caps, dbc.LAYOUT_F64, "cuda", spare_for(dbc.need(k)))
            for k, caps, _ in jobs]
    want = [nxo.decode(dbc.wire(k), *caps) for k, caps, _ in jobs]
    assert [o.s.err_kind for o in want] == [0, dbc.CAPACITY, 0]
    codec.decode_frames_async([f.data_ptr() for f in frames], [f.numel() for f in frames], cols)
    st = codec.sync(check=False)
    assert st.err_kind == dbc.CAPACITY  # the first failing call's
    for c in cols:
        assert_guards(c)
    for j in (0, 2):
        assert_columns(cols[j], want[j], None, ("id", "fixed"))
    assert_counts_are_the_need(cols[1], st, jobs[1][0])
    key = jobs[1][0]
    n = dbc.need(key)[0]
    st = run_case(codec, dbc.Case(decoder, key, dbc.LAYOUT_F64, 0, (n, 1, 1), False, "exact_again"))
    assert st.err_kind == 0 and st.path == 1


@pytest.mark.parametrize("key", dbc.frames_of("host"), ids=lambda k: k[0])
def test_pinned_host_columns_at_and_below_capacity(ctx_of, key):
    codec = ctx_of("host")
    for c in dbc.cases("host", key):
        st = run_case(codec, c, device="cpu")
        if c.short:
            st = run_case(codec, exact_of(c), device="cpu")
        assert st.err_kind == 0, c


@pytest.mark.parametrize("path", ["fast", "exact"])
def test_archive_at_and_below_capacity(ctx_of, path):
    codec = ctx_of("archive_" + path)
    buf = dbc.archive_wire()
    d = dev(buf)
    names = MIXED_COLS[:7]
    cases = dbc.archive_cases()
    exact = cases[0][1]

    def decode(cr, cc):
        cols = guarded_columns(cr, cc, 1, dbc.LAYOUT_MIXED, "cuda", spare_for(exact))
        st, used = codec.decode_archive(d, len(buf), cols, check=False)
        o, r = nxo.decode_archive(buf, cr, cc)
        assert (st.err_kind, st.err_offset) == (o.s.err_kind, o.s.err_offset)
        assert_guards(cols)
        if st.err_kind == 0:
            assert used == r
            assert_columns(cols, o, st, names)
        return st

    for label, (cr, cc), short in cases:
        st = decode(cr, cc)
        assert st.err_kind == (dbc.CAPACITY if short else 0), label
        if short:
            assert decode(*exact).err_kind == 0, label
        else:
            assert st.path == (5 if path == "fast" else 3)
