"""The guard helpers (tests/guards.py) catch what they are for: a planted one-element overrun in
each column array or fan-out output, a planted byte on either side of an encoder buffer; and pass
on clean data."""
import types

import numpy as np
import pytest

import guards

DT = {"torch.int64": np.int64, "torch.int32": np.int32, "torch.uint8": np.uint8}


def fake_columns(caps, spare, f64=False):
    """What guarded_columns returns, on numpy arrays (a Columns proper needs the device)."""
    from netidx_amd.codec import Columns
    t = {}
    for name, d, kind in Columns.FIELDS:
        if f64 and name not in ("id", "fixed"):
            t[name] = None
            continue
        dt = np.dtype(DT[d])
        raw = np.full((caps[kind] + spare) * dt.itemsize, guards.SENTINEL, np.uint8)
        t[name] = raw.view(dt)
    return types.SimpleNamespace(t=t, guard_caps=dict(caps), guard_spare=spare)


CAPS = {"rows": 7, "children": 3, "ctl": 1}


def test_clean_columns_pass():
    from netidx_amd.codec import Columns
    cols = fake_columns(CAPS, 512)
    for name, _, kind in Columns.FIELDS:  # below the capacity anything may be written
        cols.t[name][: CAPS[kind]] = 0
    guards.assert_guards(cols)
    guards.assert_guards(fake_columns(CAPS, 512, f64=True))


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_element_overrun_is_named(where):
    from netidx_amd.codec import Columns
    for name, _, kind in Columns.FIELDS:
        cols = fake_columns(CAPS, 512)
        at = CAPS[kind] if where == "first" else CAPS[kind] + 511
        cols.t[name][at] = 0
        with pytest.raises(AssertionError, match=rf"^{name}\[{at}\] was written"):
            guards.assert_guards(cols)
        cols.t[name][at] = cols.t[name][at + 1 if where == "first" else at - 1]
        guards.assert_guards(cols)


def test_one_changed_byte_of_a_wide_element_is_seen():
    cols = fake_columns(CAPS, 512, f64=True)
    cols.t["fixed"].view(np.uint8)[(CAPS["rows"] + 2) * 8 + 5] ^= 1
    with pytest.raises(AssertionError, match=r"^fixed\[9\] was written"):
        guards.assert_guards(cols)


def test_the_element_below_the_capacity_is_not_guarded():
    cols = fake_columns(CAPS, 512)
    cols.t["ctl_len"][CAPS["ctl"] - 1] = 0
    guards.assert_guards(cols)


def test_spare_is_at_least_512():
    assert guards.MIN_SPARE >= 512


@pytest.mark.parametrize("off", [0, 1, 15])
def test_buffer_guards(off):
    n = 100
    buf = guards.guarded_buffer(n, off, device="cpu")
    assert buf.numel() == 2 * guards.MARGIN + off + n
    guards.assert_outside_untouched(buf, off, n)
    lo = guards.MARGIN + off
    buf[lo: lo + n] = 0  # the output itself
    guards.assert_outside_untouched(buf, off, n)
    assert (guards.written(buf, off, n) == 0).all()
    for at, what in ((lo - 1, r"before the output .* offsets -1 \.\. -1"),
                     (lo + n, rf"behind the output .* offsets {n} \.\. {n}"),
                     (0, rf"before the output .* offsets -{lo} \.\. -{lo}"),
                     (buf.numel() - 1, r"behind the output")):
        keep = int(buf[at])
        buf[at] = 0
        with pytest.raises(AssertionError, match=what):
            guards.assert_outside_untouched(buf, off, n)
        buf[at] = keep
    guards.assert_outside_untouched(buf, off, n)
    # a shorter claim (a failed encode with cap < n): the bytes from cap on are guarded too
    with pytest.raises(AssertionError, match=r"behind the output"):
        guards.assert_outside_untouched(buf, off, n - 1)


DISPATCH_CAPS = {"chan_off": 5, "ent_sub": 9, "ent_row": 9, "last_row": 0}


def fake_dispatch(caps, spare):
    """What guarded_dispatch returns, on numpy arrays."""
    t = {k: np.full((c + spare) * 8, guards.SENTINEL, np.uint8).view(np.int64)
         for k, c in caps.items()}
    return guards.GuardedDispatch(t, dict(caps), spare)


def test_dispatch_guards_name_a_planted_overrun():
    g = fake_dispatch(DISPATCH_CAPS, 512)
    for name in guards.DISPATCH_ARRAYS:  # below the capacity anything may be written
        g.t[name][: DISPATCH_CAPS[name]] = 0
    guards.assert_dispatch_guards(g)
    for name in guards.DISPATCH_ARRAYS:
        for at in (DISPATCH_CAPS[name], DISPATCH_CAPS[name] + 511):
            keep = int(g.t[name][at])
            g.t[name][at] = 7
            with pytest.raises(AssertionError, match=rf"^{name}\[{at}\] was written: the "
                                                     rf"capacity is {DISPATCH_CAPS[name]} "):
                guards.assert_dispatch_guards(g)
            g.t[name][at] = keep
            guards.assert_dispatch_guards(g)
    # one changed byte of an element is seen
    g.t["ent_row"].view(np.uint8)[(DISPATCH_CAPS["ent_row"] + 3) * 8 + 6] ^= 1
    with pytest.raises(AssertionError, match=r"^ent_row\[12\] was written"):
        guards.assert_dispatch_guards(g)


def test_guarded_dispatch_capacities_on_the_host():
    g = guards.guarded_dispatch(4, 0, 9, device="cpu")
    assert g.guard_caps == DISPATCH_CAPS and g.guard_spare >= 512
    assert {k: v.numel() for k, v in g.t.items()} == {k: c + g.guard_spare
                                                      for k, c in DISPATCH_CAPS.items()}
    guards.assert_dispatch_guards(g)
    s = g.struct()
    assert s.cap_entries == 9 and s.chan_off == g.t["chan_off"].data_ptr()
    assert s.ent_sub == g.t["ent_sub"].data_ptr() and s.ent_row == g.t["ent_row"].data_ptr()
    assert s.last_row == g.t["last_row"].data_ptr()
    g.t["last_row"][0] = 1  # capacity 0: the first element is already the band
    with pytest.raises(AssertionError, match=r"^last_row\[0\] was written"):
        guards.assert_dispatch_guards(g)
