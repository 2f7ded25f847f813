"""Byte-range decode (nxg_decode_range + nxg_range_link) at crafted cuts: the R cases of
tests/f64_run_cases.py. A frame of three to five tiles is cut into ranges that are decoded one
after another on one context, as the ranks of nxg_decode_sharded would decode them at once, and
linked. The cuts sweep every phase of a record, the first 64 bytes (the look-behind), tile and
sub-tile edges of the length-run and the single-pass decoder, the frame end, width changes and a
planted false record. The 12-byte frame and a searched split are also swept on the context that
never hands a range over, where the run decoder's exact walk and run_search take the range's tiles.

Every range is decoded into its own guarded columns (tests/guards.py), sized to exactly the rows
that start in it. Without planted bytes no range may decline: ok == 1, entry and exit are the
first record starts at or past begin and end (from the independent parser), the rows are that
slice of the frame's, the decoder that ran is the one the tile model names (with its count of
exact tiles), and the ranges link to the cumulative row offsets. With a planted false
record (R4) or a Heartbeat (R7) a range may return ok == 0; then decoding from its predecessor's
exit must succeed, and a false entry is never reported with ok == 1.
"""
import functools
import os

import numpy as np
import pytest

import f64_run_cases as fc
from guards import assert_guards, guarded_columns

pytestmark = pytest.mark.gpu

LAYOUT_F64, LAYOUT_MIXED = 1, 2
ENV = {"default": {}, "run": {"NXG_F64_PATH": "run", "NXG_F64R_FLAGS": "2"}}
EMPTY = 2**64 - 1  # entry and exit of an empty range


@pytest.fixture(scope="module")
def ctx_of():
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


def dev_at(w, off):
    """The frame on the device, `off` bytes into its allocation."""
    import torch
    buf = torch.zeros(len(w) + 64, dtype=torch.uint8, device="cuda")
    view = buf[off:off + len(w)]
    view.copy_(torch.from_numpy(np.array(w, np.uint8)))
    torch.cuda.synchronize()
    assert view.data_ptr() == buf.data_ptr() + off
    return view


class Frame:
    """A frame's messages: where each starts, which of them are rows, and the rows' columns."""

    def __init__(self, c):
        self.w = fc.rwire(c.name)
        self.W = len(self.w)
        if c.heartbeat is None:
            rec = fc.records(self.w)
            self.start, self.row0 = rec.start, np.arange(len(rec.start))
            self.id, self.value = rec.id, rec.value
            self.layout = LAYOUT_F64
        else:  # a Heartbeat (no row) before record c.heartbeat
            L = 11 + fc.id_width(c.ids)
            s = np.concatenate([[0], np.cumsum(L)])[:len(L)]
            a = fc.rinfo(c.name)["heartbeat_at"]
            s[c.heartbeat:] += 2
            self.start = np.sort(np.concatenate([s, [a]])).astype(np.int64)
            # rows before each message
            self.row0 = np.searchsorted(s, self.start)
            self.id, self.value = c.ids, fc.rvalues(c.name)
            self.layout = LAYOUT_MIXED
            self.hb = a

    def expect(self, b, e):
        """(entry, exit, first row, rows) of the messages that start in [b, e)."""
        S = self.start
        i0, i1 = (int(x) for x in np.searchsorted(S, [b, e]))
        r0 = int(self.row0[i0]) if i0 < len(S) else len(self.id)
        r1 = int(self.row0[i1]) if i1 < len(S) else len(self.id)
        return (int(S[i0]) if i0 < len(S) else self.W, int(S[i1]) if i1 < len(S) else self.W,
                r0, r1 - r0)

    def decode(self, codec, d, b, e):
        """[b, e) into guarded columns sized to its rows; (range, columns, expected)."""
        want = self.expect(b, e)
        cols = guarded_columns(want[3], 1, 2, self.layout, "cuda")
        rng = codec.decode_range(d, self.W, b, e, cols)
        assert_guards(cols)
        return rng, cols, want

    def check(self, rng, cols, want, b, e):
        """A range that reports ok == 1 is right in every field and row."""
        entry, ex, r0, n = want
        assert rng.ok == 1 and rng.err_kind == 0, (b, e, rng.err_kind)
        if b == e:
            assert (rng.entry, rng.exit, rng.n_rows) == (EMPTY, EMPTY, 0), (b, e)
            return
        assert (rng.entry, rng.exit, rng.n_rows) == (entry, ex, n), \
            (b, e, (rng.entry, rng.exit, rng.n_rows), (entry, ex, n))
        assert cols.s.n_rows == n
        g = cols.numpy()
        assert np.array_equal(g["id"], self.id[r0:r0 + n]), (b, e)
        assert np.array_equal(g["fixed"], self.value[r0:r0 + n]), (b, e)


@functools.lru_cache(maxsize=None)
def plan_of(name, b, e):
    """The probe's verdict on [b, e) of the case's frame on the case's context."""
    c = fc.RBY_NAME[name]
    return fc.tile_plan(fc.rwire(name), b, e, fc.CTX_FLAGS[c.ctx])


def check_decoder(codec, c, rng, b, e):
    """The decoder that produced the range is the one the model names: the length-run decoder
    with the model's exact tiles, or, where the probe hands the range over, the single-pass
    decoder (it marks the entry it decoded from in diag[2]; the length-run decoder leaves 0).
    Returns the range's exact tiles."""
    p = plan_of(c.name, b, e)
    st, diag = codec.last_status(), codec.last_diag()
    what = (c.name, b, e, st, diag[:4])
    assert not p.not_f64 and st[0] == 0, what
    if p.bails:
        assert c.ctx != "run" and diag[2] == rng.entry - b + 1, what
        return 0
    assert st[1] == 0 and diag[2] == 0 and diag[0] == p.n_exact, (what, p.n_exact)
    return p.n_exact


def run_cuts(codec, c, fr, d, cuts, may_decline):
    """Decode the frame at each list of cuts and link it. Returns how many ranges declined and
    how many tiles took the exact walk."""
    import netidx_amd
    declined = exact = 0
    for cut in cuts:
        rngs = []
        for b, e in fc.ranges_of(fr.W, cut):
            rng, cols, want = fr.decode(codec, d, b, e)
            if not rng.ok:
                # only next to planted bytes; the range decodes from its predecessor's exit
                assert may_decline and rngs, (c.name, cut, b, e)
                declined += 1
                at = min(max(r.exit for r in rngs if r.exit != EMPTY), e)
                rng, cols, want = fr.decode(codec, d, at, e)
                fr.check(rng, cols, want, at, e)
                rng.begin = b
            else:
                fr.check(rng, cols, want, b, e)
                if not may_decline and b < e:
                    exact += check_decoder(codec, c, rng, b, e)
            rngs.append(rng)
        offs, bad = netidx_amd.range_link(rngs, fr.W)
        assert bad is None, (c.name, cut, bad)
        assert [int(x) for x in offs] == [int(x) for x in
                                          np.cumsum([0] + [r.n_rows for r in rngs[:-1]])]
        assert sum(r.n_rows for r in rngs) == len(fr.id)
    return declined, exact


PARAMS = [(c.name, off) for c in fc.RCASES for off in ((0, 1, 8) if c.offsets else (0,))]


@pytest.mark.parametrize("name,off", PARAMS, ids=[f"{n}+{o}" for n, o in PARAMS])
def test_ranges(ctx_of, name, off):
    c = fc.RBY_NAME[name]
    fr = Frame(c)
    d = dev_at(fr.w, off)
    cuts = c.cuts
    may_decline = c.planted is not None or c.heartbeat is not None
    declined, exact = run_cuts(ctx_of(c.ctx), c, fr, d, cuts, may_decline)
    if name.startswith("R1x-"):  # the run decoder's exact walk in range mode
        assert exact >= len(cuts), (name, exact)
    if may_decline:
        print(f"{name}: {declined} of {sum(len(x) + 1 for x in cuts)} ranges returned ok == 0")


def test_single_pass_cases_reach_the_single_pass_decoder(ctx_of):
    """R5's frame: the run probe declines with irregular == 1 and the single-pass decoder in range
    mode produces the range (it marks the entry it decoded from in diag[2])."""
    c = fc.RBY_NAME["R5-head"]
    fr = Frame(c)
    d = dev_at(fr.w, 0)
    codec = ctx_of("default")
    assert fc.tile_plan(fr.w, 0, fr.W // 2, 0).bails
    rng, cols, want = fr.decode(codec, d, 0, fr.W // 2)
    fr.check(rng, cols, want, 0, fr.W // 2)
    assert codec.last_diag()[2] == rng.entry + 1 and codec.last_status()[0] == 0
