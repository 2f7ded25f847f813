"""The guard helpers (tests/guards.py) catch what they are for: a planted one-element overrun in
each column array, a planted byte on either side of an encoder buffer; and pass on clean data."""
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
