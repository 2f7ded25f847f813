"""Guard bands for output memory (test infrastructure).

Decoders write columns up to a capacity and encoders write `[out, out + cap)`; what lies behind
must stay as it was. These helpers hand a kernel memory with sentinel bytes around the part it may
write and check the sentinels afterwards:

  guarded_columns / assert_guards          decoder outputs: every array of a Columns holds
                                           `spare` elements behind its capacity
  guarded_buffer / assert_outside_untouched  encoder outputs: `margin` bytes on both sides

The band is memory the test owns, so an overrun is seen, not faulted on.
"""
import numpy as np

SENTINEL = 0xA5
MIN_SPARE = 512  # elements: far more than a paired or 16-byte store can overrun by
MARGIN = 4096    # bytes; a multiple of 16, so `off` is the output pointer's 16-byte phase


def _kinds(cap_rows, cap_children, cap_ctl):
    return {"rows": int(cap_rows), "children": int(cap_children), "ctl": int(cap_ctl)}


def guarded_columns(cap_rows, cap_children, cap_ctl, layout, device, spare=MIN_SPARE):
    """A netidx_amd.codec.Columns whose arrays hold `spare` (at least 512) elements more than the
    capacities its struct states, every byte of every array set to SENTINEL."""
    import torch
    from netidx_amd.codec import Columns
    spare = max(int(spare), MIN_SPARE)
    caps = _kinds(cap_rows, cap_children, cap_ctl)
    cols = Columns(caps["rows"] + spare, caps["children"] + spare, caps["ctl"] + spare, layout,
                   device)
    cols.s.cap_rows, cols.s.cap_children, cols.s.cap_ctl = (
        caps["rows"], caps["children"], caps["ctl"])
    cols.guard_caps, cols.guard_spare = caps, spare
    for t in cols.t.values():
        if t is not None:
            t.view(torch.uint8).fill_(SENTINEL)
    if cols.device.type == "cuda":
        torch.cuda.synchronize(cols.device)  # the codec runs on its own stream
    return cols


def _host_bytes(x):
    """(flat uint8 view of a host copy, element size) of a tensor or an ndarray."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.reshape(-1).view(np.uint8), x.dtype.itemsize


def assert_guards(cols):
    """Every element in [cap, cap + spare) of every array still holds the sentinel."""
    from netidx_amd.codec import Columns
    for name, _, kind in Columns.FIELDS:
        t = cols.t.get(name)
        if t is None:
            continue
        cap, spare = cols.guard_caps[kind], cols.guard_spare
        b, isz = _host_bytes(t)
        assert len(b) == (cap + spare) * isz, (name, len(b), cap, spare, isz)
        bad = np.flatnonzero(b[cap * isz:] != SENTINEL)
        if len(bad):
            at = cap + int(bad[0]) // isz
            raise AssertionError(
                f"{name}[{at}] was written: the capacity is {cap} {kind} "
                f"({len(np.unique(bad // isz))} elements of the guard band changed, the last at "
                f"{cap + int(bad[-1]) // isz})")


def guarded_buffer(n, off, margin=MARGIN, device="cuda"):
    """A uint8 tensor of margin + off + n + margin SENTINEL bytes: an encoder writes at
    `out_ptr(buf, off)`, i.e. margin + off bytes in."""
    import torch
    buf = torch.full((margin + off + n + margin,), SENTINEL, dtype=torch.uint8, device=device)
    buf.guard_margin = margin
    if buf.device.type == "cuda":
        torch.cuda.synchronize(buf.device)
    return buf


def out_ptr(buf, off):
    return buf.data_ptr() + buf.guard_margin + off


def written(buf, off, n):
    """Host copy of the n bytes at the output position."""
    b, _ = _host_bytes(buf)
    m = buf.guard_margin
    return b[m + off: m + off + n]


def assert_outside_untouched(buf, off, n):
    """No byte before margin + off or from margin + off + n on changed."""
    b, _ = _host_bytes(buf)
    lo = buf.guard_margin + off
    for side, part, base in (("before", b[:lo], -lo), ("behind", b[lo + n:], n)):
        bad = np.flatnonzero(part != SENTINEL)
        if len(bad):
            raise AssertionError(
                f"{len(bad)} bytes {side} the output were written: offsets {base + int(bad[0])} .. "
                f"{base + int(bad[-1])} relative to out (the output is [0, {n}), phase "
                f"{lo % 16})")
