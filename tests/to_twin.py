"""Python twin of publisher::To (netidx-netproto/src/publisher.rs:50-70): the reference for the
write-batch tests. Built on the primitives of tests/golden/make_golden.py (varints, lw,
Value::encode, the expected column slots of a canonical Value); the decoder below is written from
the reference's rules and shares no code with the C++/HIP.

Wire: every message is varint(L) variant fields..., L = lw(1 + |fields|) (pack.rs:522-555).
  0 Subscribe   path Path, resolver SocketAddr (pack.rs:187-238), timestamp u64 BE,
                permissions u32 BE, token Bytes (pack.rs:251-258)
  1 Unsubscribe Id varint
  2 Write       Id varint, bool (pack.rs:1491-1497), Value, #[pack(default)] WriteId varint: a
                BufferShort while decoding it means "absent" (netidx-derive/src/lib.rs:392-401)
A frame fails as a whole with (PackError kind, offset of the first failing message).
"""
import importlib.util
import os
import struct

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

UNKNOWN_TAG, TOO_BIG, INVALID, SHORT = 1, 2, 3, 4
WRITE_REPLY, WRITE_NO_WID = 1, 2
MAX_VEC = 2 * 1024 * 1024 * 1024
M64 = (1 << 64) - 1

_mg_mod = None


def mg():
    global _mg_mod
    if _mg_mod is None:
        spec = importlib.util.spec_from_file_location("mg", os.path.join(GOLD, "make_golden.py"))
        _mg_mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_mg_mod)
    return _mg_mod


# ---- encode ---------------------------------------------------------------------------------
def write(id, reply, value, wid=None, trailing=b"", id_bytes=None):
    """To::Write(id, reply, value, wid). wid None: an old peer's message without the WriteId.
    trailing: bytes inside the length wrap after the last field. id_bytes: the id's varint
    spelled out (non-minimal forms)."""
    m = mg()
    body = (id_bytes if id_bytes is not None else m.enc_varint(id)) + bytes([1 if reply else 0])
    body += m.enc_value(value)
    if wid is not None:
        body += m.enc_varint(wid)
    return m.enc_msg(2, body + trailing)


def unsubscribe(id, trailing=b""):
    return mg().enc_msg(1, mg().enc_varint(id) + trailing)


def sockaddr(addr):
    """('v4', ip u32, port) | ('v6', 8 segments, port, flowinfo, scope_id)."""
    if addr[0] == "v4":
        return b"\x00" + struct.pack(">IH", addr[1], addr[2])
    return b"\x01" + struct.pack(">8HHII", *addr[1], addr[2], addr[3], addr[4])


def subscribe(path, resolver=("v4", 0, 0), timestamp=0, permissions=0, token=b"", trailing=b""):
    m = mg()
    p = path if isinstance(path, bytes) else path.encode()
    body = m.enc_varint(len(p)) + p + sockaddr(resolver) + struct.pack(">QI", timestamp, permissions)
    body += m.enc_varint(len(token)) + token
    return m.enc_msg(0, body + trailing)


class Expect:
    def __init__(self):
        self.rows = []      # (id, tag, fixed, aux)
        self.children = []  # (tag, fixed, aux)
        self.ctl = []       # (row, off, len, variant)
        self.wflags = []
        self.wid = []


def batch(msgs):
    """msgs: ('w', id, reply, value, wid | None) | ('unsub', id) | ('sub', kwargs) |
    ('raw', bytes of one whole control message, variant). Returns (wire, Expect): the expected
    columns from the messages themselves (make_golden.flatten), not from decoding the wire."""
    m = mg()
    wire = bytearray()
    e = Expect()
    for x in msgs:
        start = len(wire)
        if x[0] == "w":
            _, i, reply, v, wid = x
            enc = write(i, reply, v, wid)
            nfields = len(m.enc_varint(i)) + 1 + len(m.enc_value(v))
            nfields += len(m.enc_varint(wid)) if wid is not None else 0
            hdr = m.varint_len(m.lw(1 + nfields))
            payload_off = start + hdr + 1 + len(m.enc_varint(i)) + 1 + 1
            e.rows.append((i,) + m.flatten(e, v, payload_off))
            e.wflags.append((WRITE_REPLY if reply else 0) | (WRITE_NO_WID if wid is None else 0))
            e.wid.append(0 if wid is None else wid)
        elif x[0] == "unsub":
            enc = unsubscribe(x[1])
            e.ctl.append((len(e.rows), start, len(enc), 1))
        elif x[0] == "sub":
            enc = subscribe(**x[1])
            e.ctl.append((len(e.rows), start, len(enc), 0))
        else:
            enc = x[1]
            e.ctl.append((len(e.rows), start, len(enc), x[2]))
        wire += enc
    return bytes(wire), e


def update_frame(pairs):
    """The From::Update frame of the same (id, value) list (the C oracle's ground)."""
    return b"".join(mg().update(i, v) for i, v in pairs)


def value_of_columns(m, i):
    """Row i of netidx_amd.synth.MixedColumns as a make_golden Value."""
    def leaf(t, f, a):
        f = int(f)
        if t == 6:
            return (6, f - (1 << 64) if f >> 63 else f)
        if t == 9:
            return (9, f)
        if t == 10:
            return (10, (f - (1 << 64) if f >> 63 else f, int(a)))
        if t == 12:
            return (12, bytes(m.heap[f:f + int(a)]))
        raise ValueError(t)
    t = int(m.tag[i])
    if t == 19:
        b, n = int(m.fixed[i]), int(m.aux[i])
        return (19, [leaf(int(m.ctag[k]), m.cfixed[k], m.caux[k]) for k in range(b, b + n)])
    return leaf(t, m.fixed[i], m.aux[i])


# ---- decode ---------------------------------------------------------------------------------
class PErr(Exception):
    def __init__(self, kind):
        self.kind = kind


def _varint(b, p, lim):
    """decode_varint (pack.rs:504-520): at most 10 bytes, bits past 64 dropped."""
    v = 0
    for i in range(10):
        if p + i >= lim:
            raise PErr(SHORT)
        c = b[p + i]
        v |= (c & 0x7F) << (7 * i)
        if c < 0x80:
            return v & M64, p + i + 1
    raise PErr(INVALID)


def _fix(b, p, lim, n):
    if lim - p < n:
        raise PErr(SHORT)
    return int.from_bytes(b[p:p + n], "big"), p + n


def _sx(v, bits):
    return (v - (1 << bits) if v >> (bits - 1) else v) & M64


def _text(b, p, lim, utf8):
    n, p = _varint(b, p, lim)
    if n > lim - p:
        raise PErr(TOO_BIG)
    if utf8:
        try:
            bytes(b[p:p + n]).decode("utf-8")
        except UnicodeDecodeError:
            raise PErr(INVALID)
    return p, n, p + n


def _datetime_ok(secs, ns):
    if ns >= 2_000_000_000 or not -8210266876800 <= secs <= 8210266876799:
        return False
    return ns < 1_000_000_000 or secs % 60 == 59


def _value(b, p, lim, kids, depth=0):
    """Value::decode (netidx-value/src/lib.rs:470-506) at p: returns (slot, p). Children go to
    `kids`, a container's elements in one block, depth-first."""
    if p >= lim:
        raise PErr(SHORT)
    t = b[p]
    p += 1
    if t in (0, 8):
        v, p = _fix(b, p, lim, 4)
        return (t, v, 0), p
    if t == 2:
        v, p = _fix(b, p, lim, 4)
        return (2, _sx(v, 32), 0), p
    if t in (1, 3, 5, 7):
        v, p = _varint(b, p, lim)
        if t == 1:
            v &= 0xFFFFFFFF
        elif t == 3:
            u = v & 0xFFFFFFFF
            v = _sx((u >> 1) ^ (0xFFFFFFFF if u & 1 else 0), 32)
        elif t == 7:
            v = (v >> 1) ^ (M64 if v & 1 else 0)
        return (t, v, 0), p
    if t in (4, 6, 9):
        v, p = _fix(b, p, lim, 8)
        return (t, v, 0), p
    if t in (10, 11):
        s, p = _fix(b, p, lim, 8)
        ns, p = _fix(b, p, lim, 4)
        if t == 10:
            if not _datetime_ok(s - (1 << 64) if s >> 63 else s, ns):
                raise PErr(INVALID)
        elif ns >= 1_000_000_000:
            s += ns // 1_000_000_000
            ns %= 1_000_000_000
            if s > M64:
                raise PErr(INVALID)
        return (t, s, ns), p
    if t in (12, 13, 18):
        off, n, p = _text(b, p, lim, t != 13)
        return (t, off, n), p
    if t == 14:
        return (14, 1, 0), p
    if t in (15, 16, 17):
        return (16 if t == 17 else t, 0, 0), p
    if t in (19, 21):
        n, p = _varint(b, p, lim)
        unit = 16 if t == 19 else 32
        if n > MAX_VEC // unit or n * unit > ((lim - p) << 8):
            raise PErr(TOO_BIG)
        cnt = n if t == 19 else 2 * n
        base = len(kids)
        kids.extend([None] * cnt)
        for i in range(cnt):
            kids[base + i], p = _value(b, p, lim, kids, depth + 1)
        return (t, base, n), p
    if t == 20:
        if lim - p < 16:
            raise PErr(SHORT)
        return (20, p, 16), p + 16
    if t == 22:
        if p < lim and b[p] == 12:  # Error(String): tag 18 in the columns
            off, n, p = _text(b, p + 1, lim, True)
            return (18, off, n), p
        base = len(kids)
        kids.append(None)
        kids[base], p = _value(b, p, lim, kids, depth + 1)
        return (22, base, 1), p
    if t in (23, 24):
        v, p = _fix(b, p, lim, 1)
        return (t, _sx(v, 8) if t == 24 else v, 0), p
    if t in (25, 26):
        v, p = _fix(b, p, lim, 2)
        return (t, _sx(v, 16) if t == 26 else v, 0), p
    if t == 27:  # Abstract: a length-wrapped {uuid, payload} (abstract_type.rs:280-298)
        n, p = _varint(b, p, lim)
        if n < 1:
            raise PErr(SHORT)
        l2 = min(p + n - mg().varint_len(n), lim)
        if l2 - p < 16:
            raise PErr(SHORT)
        return (27, p, l2 - p), l2
    raise PErr(UNKNOWN_TAG)


def _message(b, pos, e):
    """One To message at pos: appends its columns to e, returns the next position."""
    W = len(b)
    L, p = _varint(b, pos, W)
    if L < 1:
        raise PErr(SHORT)
    lim = min(p + L - mg().varint_len(L), W)
    if p >= lim:
        raise PErr(SHORT)
    variant = b[p]
    p += 1
    if variant == 0:
        _, _, p = _text(b, p, lim, True)
        tag, p = _fix(b, p, lim, 1)
        if tag == 0:
            _, p = _fix(b, p, lim, 4)
            _, p = _fix(b, p, lim, 2)
        elif tag == 1:
            for n in (2,) * 9 + (4, 4):
                _, p = _fix(b, p, lim, n)
        else:
            raise PErr(UNKNOWN_TAG)
        _, p = _fix(b, p, lim, 8)
        _, p = _fix(b, p, lim, 4)
        _text(b, p, lim, False)
        e.ctl.append((len(e.rows), pos, lim - pos, 0))
    elif variant == 1:
        _varint(b, p, lim)
        e.ctl.append((len(e.rows), pos, lim - pos, 1))
    elif variant == 2:
        i, p = _varint(b, p, lim)
        r, p = _fix(b, p, lim, 1)
        if r > 1:
            raise PErr(UNKNOWN_TAG)
        kids = list(e.children)
        slot, p = _value(b, p, lim, kids)
        try:
            wid, p = _varint(b, p, lim)
            flags = r
        except PErr as x:
            if x.kind != SHORT:
                raise
            wid, flags = 0, r | WRITE_NO_WID
        e.children = kids
        e.rows.append((i,) + slot)
        e.wflags.append(flags)
        e.wid.append(wid)
    else:
        raise PErr(UNKNOWN_TAG)
    return lim


def decode(wire):
    """(Expect, None) or (None, (kind, offset of the first failing message))."""
    b = bytes(wire)
    e = Expect()
    pos = 0
    while pos < len(b):
        try:
            pos = _message(b, pos, e)
        except PErr as x:
            return None, (x.kind, pos)
    return e, None


def first_error(wire):
    return decode(wire)[1]
