"""Guard bands for output memory (test infrastructure).

Decoders write columns up to a capacity and encoders write `[out, out + cap)`; what lies behind
must stay as it was. These helpers hand a kernel memory with sentinel bytes around the part it may
write and check the sentinels afterwards:

  guarded_columns / assert_guards          decoder outputs: every array of a Columns holds
                                           `spare` elements behind its capacity
  guarded_buffer / assert_outside_untouched  encoder outputs: `margin` bytes on both sides
  guarded_dispatch / assert_dispatch_guards  fan-out outputs (NxgDispatch): chan_off, ent_sub,
                                           ent_row and last_row at exactly their capacities,
                                           `spare` elements behind each

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


DISPATCH_ARRAYS = ("chan_off", "ent_sub", "ent_row", "last_row")


class GuardedDispatch:
    """Caller-owned outputs of nxg_dispatch_updates / nxg_publish_commit (uint64 arrays held as
    int64 tensors): `caps[name]` elements the call may write, `spare` behind them, every byte
    SENTINEL."""

    def __init__(self, t, caps, spare):
        self.t, self.guard_caps, self.guard_spare = t, caps, spare

    def struct(self):
        """The NxgDispatch that states the capacities."""
        from netidx_amd.codec import NxgDispatch
        return NxgDispatch(self.guard_caps["ent_sub"], *(self.t[k].data_ptr()
                                                         for k in DISPATCH_ARRAYS), 0, 0)

    def host(self, name, n=None):
        """Host copy (uint64) of the first n (default: the capacity) elements of an array."""
        n = self.guard_caps[name] if n is None else n
        return self.t[name][:n].cpu().numpy().view(np.uint64)


def guarded_dispatch(n_chans, n_slots, cap_entries, device="cuda", spare=MIN_SPARE):
    """chan_off[n_chans + 1], ent_sub[cap_entries], ent_row[cap_entries], last_row[n_slots], each
    followed by `spare` (at least 512) guard elements."""
    import torch
    spare = max(int(spare), MIN_SPARE)
    caps = {"chan_off": int(n_chans) + 1, "ent_sub": int(cap_entries),
            "ent_row": int(cap_entries), "last_row": int(n_slots)}
    t = {k: torch.full(((c + spare) * 8,), SENTINEL, dtype=torch.uint8,
                       device=device).view(torch.int64) for k, c in caps.items()}
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)  # the codec runs on its own stream
    return GuardedDispatch(t, caps, spare)


def assert_dispatch_guards(g):
    """Every element in [cap, cap + spare) of the four arrays still holds the sentinel."""
    for name in DISPATCH_ARRAYS:
        cap, spare = g.guard_caps[name], g.guard_spare
        b, isz = _host_bytes(g.t[name])
        assert len(b) == (cap + spare) * isz, (name, len(b), cap, spare, isz)
        bad = np.flatnonzero(b[cap * isz:] != SENTINEL)
        if len(bad):
            raise AssertionError(
                f"{name}[{cap + int(bad[0]) // isz}] was written: the capacity is {cap} "
                f"({len(np.unique(bad // isz))} elements of the guard band changed, the last at "
                f"{cap + int(bad[-1]) // isz})")
