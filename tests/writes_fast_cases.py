"""The case table of the fast To decoder (nxg_decode_writes_opts with fast = 1), shared by
tests/test_writes_fast_cases_cpu.py and tests/test_gpu_writes_fast.py.

Each case is a frame with a class:
  must     the fast decoder has to take it (NxgStatus.path 8)
  may      taking it is the implementation's choice (path 6 or 8)
  decline  it has to go to the general decoder (path 6): frames the twin rejects (`err` holds the
           twin's (kind, offset)) and valid frames outside the fast decoder's set
The reference is tests/to_twin.py everywhere. fast_must_take() restates the "must take" rule of
include/nxg_codec.h on the twin's primitives: every message a Write with a one-byte length, an id
of at most 35 bits, bool 0 / 1, a valid Value without child slots, and no or exactly one WriteId
varint; an Unsubscribe filled exactly; or a Subscribe filled exactly with address tag 0 / 1, a
UTF-8 path and at most 256 bytes in all -- canonical varints throughout.

Wire lengths: the length prefix counts itself (pack.rs:522-555), so a message at p ends at
p + L; `03 01 07` is the shortest message (an Unsubscribe), 1,366 of which start in a 4 KiB tile.
"""
import random

import to_twin as tw

TILE = 4096
MAX_FAST_MSG = 256  # bytes of the longest Subscribe the fast decoder must take, prefix included
# value tags without child slots that the fast decoder must take (22: only in front of 12)
LEAF_TAGS = frozenset([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 23,
                       24, 25, 26])
VARINT_TAGS = frozenset([1, 3, 5, 7, 12, 13, 18])  # the payload starts with a varint


class Case:
    def __init__(self, name, wire, cls, err=None):
        assert cls in ("must", "may", "decline")
        self.name, self.wire, self.cls, self.err = name, bytes(wire), cls, err

    def __repr__(self):
        return f"Case({self.name}, {len(self.wire)} B, {self.cls})"


class _No(Exception):
    pass


def _cv(b, p, lim):
    """A canonical varint at p (twin's decode_varint, then the minimal-length rule)."""
    v, q = tw._varint(b, p, lim)
    if q - p != tw.mg().varint_len(v):
        raise _No()
    return v, q


def _must_message(b, pos):
    W = len(b)
    L, p = _cv(b, pos, W)
    lim = pos + L
    if L < 1 or lim > W or p >= lim:
        raise _No()
    variant = b[p]
    p += 1
    if variant == 2:
        if p - pos != 2:
            raise _No()  # a one-byte length
        i, p = _cv(b, p, lim)
        if i >> 35 or p >= lim or b[p] > 1 or p + 1 >= lim:
            raise _No()
        t = b[p + 1]
        if t == 22:
            if p + 2 >= lim or b[p + 2] != 12:
                raise _No()
            _cv(b, p + 3, lim)
        elif t not in LEAF_TAGS:
            raise _No()
        elif t in VARINT_TAGS:
            _cv(b, p + 2, lim)
        kids = []
        _, p = tw._value(b, p + 1, lim, kids)
        if kids:
            raise _No()
        if p != lim:
            _, p = _cv(b, p, lim)
    elif variant == 1:
        _, p = _cv(b, p, lim)
    elif variant == 0:
        if L > MAX_FAST_MSG:
            raise _No()
        n, p = _cv(b, p, lim)
        if n > lim - p:
            raise _No()
        try:
            bytes(b[p:p + n]).decode("utf-8")
        except UnicodeDecodeError:
            raise _No()
        p += n
        if p >= lim or b[p] > 1:
            raise _No()
        p += 1 + (26 if b[p] else 6) + 12
        if p >= lim:
            raise _No()
        n, p = _cv(b, p, lim)
        p += n
    else:
        raise _No()
    if p != lim:
        raise _No()
    return lim


def fast_must_take(wire):
    """True when every message of the (non-empty) frame is in the fast decoder's must-take set."""
    b = bytes(wire)
    pos = 0
    try:
        while pos < len(b):
            pos = _must_message(b, pos)
    except (_No, tw.PErr):
        return False
    return len(b) > 0


# ---- builders -----------------------------------------------------------------------------------
def W(i, reply, v, wid=None):
    return tw.write(i, reply, v, wid)


def U(i):
    return tw.unsubscribe(i)


def S(path=b"/a/b", resolver=("v4", 0x7F000001, 4242), timestamp=1, permissions=7, token=b"tok"):
    return tw.subscribe(path, resolver, timestamp, permissions, token)


V6 = ("v6", (0x2001, 0xDB8, 0, 0, 0, 0, 0, 1), 443, 5, 9)


def filler(n):
    """Exactly n bytes of Unsubscribes (3- and 4-byte ones; n = 0, 3, 4 or >= 6)."""
    assert n in (0, 3, 4) or n >= 6, n
    four = n % 3  # n = 3 a + 4 b with the fewest 4-byte ones
    out = U(300) * four + U(7) * ((n - 4 * four) // 3)
    assert len(out) == n
    return out


def sub_of_len(n, path=b"/p", token_fill=b"t", resolver=("v4", 1, 2)):
    """A Subscribe of exactly n bytes in all (by the token's length)."""
    for tl in range(0, n):
        token = (token_fill * (tl // len(token_fill) + 1))[:tl]
        m = S(path, resolver, 3, 4, token)
        if len(m) == n:
            return m
    # 128 bytes: no encoder output (lw skips it), still a canonical prefix `80 01`
    mg = tw.mg()
    for tl in range(0, n):
        m = S(path, resolver, 3, 4, (token_fill * (tl + 1))[:tl])
        body = m[mg.varint_len(len(m)):]
        if mg.varint_len(n) + len(body) == n:
            return mg.enc_varint(n) + body
    raise ValueError(n)


LEAF_VALUES = [
    (0, 0xDEADBEEF), (1, 5), (1, 0xFFFFFFFF), (2, -5), (3, -70000), (4, 2**64 - 1), (5, 2**63),
    (5, 0), (6, -2**63), (7, -2**40 - 5), (8, 0x3FC00000), (9, 0x3FF0000000000000),
    (10, (1_700_000_000, 999_999_999)), (10, (-8210266876800, 0)), (10, (59, 1_500_000_000)),
    (11, (2**63 + 1, 999_999_999)), (12, b""), (12, b"plain text"), (12, "é€😀Ωж".encode()),
    (12, b"x" * 100), (13, bytes(range(200, 256)) + b"\x00\x01\x02"), (14, None), (15, None),
    (16, None), (18, b"an error"), (18, "fehler: é".encode()), (20, bytes(range(16))), (23, 200),
    (24, -100), (25, 60000), (26, -30000),
]


def seeded_msgs(n, seed):
    """n messages of all three kinds from the must-take set."""
    rng = random.Random(seed)
    alphabet = "abcxyz019/ é€😀Ωж"
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.6:
            v = rng.choice(LEAF_VALUES)
            if v[0] == 12 and rng.random() < 0.5:
                v = (12, "".join(rng.choice(alphabet) for _ in range(rng.randrange(60))).encode())
            wid = None if rng.random() < 0.2 else rng.getrandbits(rng.choice([7, 14, 35, 63, 64]))
            out.append(W(rng.getrandbits(rng.choice([7, 14, 21, 28, 35])), rng.random() < 0.5, v,
                         wid))
        elif r < 0.8:
            out.append(U(rng.getrandbits(rng.choice([7, 14, 35, 64]))))
        else:
            path = ("/" + "".join(rng.choice(alphabet) for _ in range(rng.randrange(40)))).encode()
            token = bytes(rng.getrandbits(8) for _ in range(rng.randrange(50)))
            out.append(S(path, V6 if rng.random() < 0.3 else ("v4", rng.getrandbits(32), 80),
                         rng.getrandbits(64), rng.getrandbits(32), token))
    return out


def seeded(n, seed):
    return b"".join(seeded_msgs(n, seed))


def exactly(n_bytes, seed):
    """A seeded must-take frame of exactly n_bytes."""
    body = b""
    for m in seeded_msgs(n_bytes // 16, seed):
        if len(body) + len(m) > n_bytes - 6:
            break
        body += m
    return body + filler(n_bytes - len(body))


# ---- the table ----------------------------------------------------------------------------------
F64_UNSUBS = int.from_bytes(b"\x03\x01\x07\x03\x01\x07\x03\x01", "big")   # an f64 spelling Unsubscribes
F64_WRITE = int.from_bytes(b"\x05\x02\x01\x00\x10\x03\x01\x07", "big")    # ... a Write of Null
TS_WRITE = int.from_bytes(b"\x05\x02\x01\x00\x00\x05\x02\x01", "big")
TOK_UNSUBS = b"\x03\x01\x07"
TOK_WRITES = b"\x05\x02\x01\x00\x00"


def _one_of_each():
    c = []
    add = lambda name, wire, cls="must": c.append(Case(name, wire, cls))
    add("write_alone", W(1, False, (9, 5), 3))
    add("unsubscribe_alone", U(7))
    add("subscribe_alone", S())
    for v in LEAF_VALUES:
        add(f"value_tag{v[0]}_{len(c)}", W(77, True, v, 9) + W(78, False, v, None))
    add("value_null_tag17", tw.mg().enc_msg(2, b"\x05\x01\x11\x07"))
    add("value_error_string_22_12", tw.mg().enc_msg(2, b"\x05\x00\x16\x0c\x03abc\x09"))
    for nb in range(1, 11):
        i = 1 << (7 * nb - 1) if nb < 10 else 1 << 63
        add(f"write_id_{nb}_bytes", W(i, True, (4, nb), 1) + W(i | 1, False, (12, b"s"), None),
            "must" if nb <= 5 else "may")
        add(f"unsubscribe_id_{nb}_bytes", U(i) + U(i | 1))
        add(f"wid_{nb}_bytes", W(5, False, (9, 1), i) + W(6, True, (1, 300), i | 1))
    add("wid_absent", W(5, False, (9, 1), None) + W(5, True, (12, b"abc"), None))
    add("bool_0_and_1", W(5, False, (14, None), 0) + W(5, True, (15, None), 0))
    add("subscribe_v4", S(resolver=("v4", 0xC0A80001, 65535)))
    add("subscribe_v6", S(resolver=V6))
    for n in (0, 1, 40):
        add(f"token_{n}_bytes", S(token=bytes(range(n))) + S(resolver=V6, token=bytes(range(n))))
    add("path_non_ascii", S(path="/é/€/😀".encode()) + S(path="/жж/Ω€😀😀".encode(), resolver=V6))
    add("path_empty", S(path=b""))
    add("path_130_bytes", S(path=b"/" + b"p" * 129, token=b""))
    add("token_130_bytes", S(path=b"/t", token=bytes(130)))
    add("sub_L_127", sub_of_len(127) + U(1))
    add("sub_L_128", sub_of_len(128) + U(1))
    add("sub_256_bytes", sub_of_len(256) + U(1))
    add("sub_257_bytes", sub_of_len(257) + U(1), "may")
    add("sub_5000_bytes", sub_of_len(5000) + U(1) + W(1, True, (9, 1), 1), "may")
    add("write_L_127", W(9, True, (12, b"w" * 120), 1) + U(1))
    assert len(W(9, True, (12, b"w" * 120), 1)) == 127
    add("write_two_byte_L", W(9, True, (12, b"w" * 130), 1) + U(1), "may")
    add("non_canonical_id", tw.write(5, True, (9, 1), 4, id_bytes=b"\x85\x00") + U(1), "may")
    add("non_canonical_wid", tw.mg().enc_msg(2, b"\x05\x01\x10\x84\x00") + U(1), "may")
    # texts of one round that add up to more than 256 non-ASCII bytes, and one longer than 32
    add("many_non_ascii_texts", b"".join(W(i, True, (12, "ж".encode() * 30), i) for i in range(20)))
    return c


def _geometry():
    c = []
    add = lambda name, wire, cls="must": c.append(Case(name, wire, cls))
    tail = W(3, True, (12, "é".encode() * 5), 2**40) + U(9) + S(resolver=V6)
    sub = S(path="/geo/é/path-of-some-length".encode(), resolver=V6, timestamp=2**63 + 5,
            token=bytes(range(1, 30)))
    wr = W(2**34 + 3, True, (12, b"value text " * 5), 2**63 + 11)
    assert len(sub) > 72 and len(wr) > 72
    for off in range(-70, 3):
        add(f"sub_at_edge{off:+d}", filler(TILE + off) + sub + wr + tail)
        add(f"write_at_edge{off:+d}", filler(TILE + off) + wr + sub + tail)
    for nt in (1, 4, 5, 9):
        add(f"exactly_{nt}_tiles", exactly(nt * TILE, 100 + nt))
    # the resolve pass scans 256 tiles per block: one block of sums, and two
    big = sub_of_len(250, path=b"/big/" + b"p" * 60, token_fill=b"\x03\x01\x07")
    for nt in (256, 257):
        n = nt * TILE
        body = seeded(300, nt)
        k = (n - len(body) - 300) // len(big)
        rest = n - len(body) - k * len(big)
        add(f"exactly_{nt}_tiles", body + big * k + filler(rest))
    add("tile_of_1366_unsubscribes", TOK_UNSUBS * 1366)
    add("three_tiles_of_unsubscribes", TOK_UNSUBS * (3 * 1366))
    add("last_tile_of_1_byte", filler(TILE - 7) + U(2**40))   # 8 bytes: ends at 4097
    assert len(c[-1].wire) == TILE + 1
    add("last_tile_entered_at_its_end", filler(TILE - 3) + U(2**40))  # the frame ends inside tile 1
    # rounds of 64 messages: 63, 64, 65 in one tile
    for n in (63, 64, 65, 128, 129):
        add(f"{n}_messages", b"".join(W(i, i & 1, (9, i), i) if i % 3 else U(i) for i in range(n)))
    return c


def _planted():
    c = []
    add = lambda name, wire, cls="must": c.append(Case(name, wire, cls))
    add("tokens_of_unsubscribes", b"".join(S(token=TOK_UNSUBS * k) for k in range(1, 14)) * 12)
    add("tokens_of_writes", b"".join(S(token=TOK_WRITES * k) for k in range(1, 9)) * 20)
    add("f64s_spelling_messages",
        b"".join(W(i, True, (9, F64_UNSUBS if i & 1 else F64_WRITE), i) for i in range(900)))
    add("timestamps_spelling_writes", S(timestamp=TS_WRITE, token=b"") * 300)
    add("datetimes_spelling_messages",
        b"".join(W(i, False, (10, (0x0301070301, 0x03010703)), None) for i in range(800)))
    add("paths_holding_variant_bytes",
        (S(path=b"/\x03\x00\x01x") + S(path=b"/\x03\x01\x07\x03\x01\x07") +
         S(path=b"/\x05\x02\x01\x00\x10y") + S(path=b"\x06\x02\x01\x01\x0e\x00")) * 70)
    # sparse: one planted token in front of and one behind every tile edge
    for name, tok in (("unsubscribes", TOK_UNSUBS * 20), ("writes", TOK_WRITES * 12),
                      ("unsubscribes_then_junk", TOK_UNSUBS * 20 + b"\xff\xff")):
        wire = b""
        for t in range(1, 6):
            m = S(token=tok)
            wire += filler(t * TILE - len(wire) - len(m) + 40) + m + m
        add(f"sparse_tokens_of_{name}", wire + U(1))
    # a token that crosses the tile edge: k false starts behind the edge, each on a chain of its
    # own that breaks (`03 01 07 ff`: an Unsubscribe, then no message), in front of the true one
    # -- on both sides of the number of chains a tile's entry guess tries (16). Past it the tile
    # is recounted from its predecessor's exit, which needs the predecessor's own count: planted
    # at every other edge these frames must be taken; at adjacent edges the second tile has
    # nothing to be recounted from and the frame may fall back (documented in
    # nxg_decode_writes_fast.hip; the columns are the twin's either way)
    for k in (1, 15, 16, 17, 40):
        tok = b"\x00" * 50 + (TOK_UNSUBS + b"\xff") * k + b"\xff"
        m = S(path=b"/x", token=tok)
        head = len(m) - len(tok) + 50  # the first planted byte, from the message start
        for name, edges, cls in (("every_other_edge", (1, 3, 5), "must"),
                                 ("adjacent_edges", (1, 2, 3), "must" if k < 16 else "may")):
            wire = b""
            for t in edges:
                wire += filler(t * TILE - len(wire) - head) + m
            add(f"{k}_breaking_chains_behind_{name}", wire + W(1, True, (9, 1), 1), cls)
    # one broken chain with many starts on it
    for k in (4, 40):
        tok = b"\x00" * 50 + TOK_UNSUBS * k + b"\xff\xff"
        m = S(path=b"/x", token=tok)
        head = len(m) - len(tok) + 50
        wire = b""
        for t in range(1, 4):
            wire += filler(t * TILE - len(wire) - head) + m
        add(f"{k}_starts_on_one_breaking_chain_behind_the_edge", wire + W(1, True, (9, 1), 1))
    # ... and merging ones: the token ends with its last planted message
    for k in (1, 4, 40):
        tok = b"\x00" * 50 + TOK_UNSUBS * k
        m = S(path=b"/x", token=tok)
        head = len(m) - len(tok) + 50
        wire = b""
        for t in range(1, 4):
            wire += filler(t * TILE - len(wire) - head) + m
        add(f"{k}_merging_false_starts_behind_the_edge", wire + W(1, True, (9, 1), 1))
    # a false chain that never merges: Bytes values holding two planted Writes each, the second
    # of which reaches over the real WriteId and the next real header to the next value's first.
    # A tile whose first confirmed start is a planted one follows the planted chain to its end, so
    # its exit is wrong too; the chain check then sends the frame to the general decoder
    # (documented in nxg_decode_writes_fast.hip): the columns are the twin's either way
    a = bytes([50, 2, 5, 0, 16]) + bytes(45)
    b = bytes([57, 2, 5, 0, 16]) + bytes(45)
    m = W(5, True, (13, a + b), 7)
    assert len(m) == 107 and m.index(a) == 6
    add("interleaved_false_chain_never_merges", m * 200, "may")
    # every 64-byte chunk begins with planted Unsubscribes: 64-byte Subscribes whose token starts
    # on the chunk edge; breaking (a byte left over) and merging (the token exactly filled)
    m64 = sub_of_len(64, path=b"/a/b", token_fill=TOK_UNSUBS)
    hdr = m64.index(TOK_UNSUBS)  # the token's offset in the message
    add("every_chunk_starts_planted_breaking", filler(64 - hdr) + m64 * 300)
    m63 = sub_of_len(63, path=b"/a/b", token_fill=TOK_UNSUBS)
    assert m63.index(TOK_UNSUBS) == hdr and (63 - hdr) % 3 == 0
    wire = b""
    for t in range(1, 6):
        wire += filler(t * TILE - len(wire) - hdr) + m63 * 3
    add("every_tile_starts_planted_merging", wire)
    return c


def _bad_messages():
    """name -> one message the general decoder rejects (the twin's kind is recorded per case)."""
    m = tw.mg()
    sub_body = lambda path, tag, tok: (m.enc_varint(len(path)) + path + bytes([tag]) + bytes(6) +
                                       bytes(12) + tok)
    return {
        "variant_3": m.enc_msg(3, b"\x01"),
        "bool_2": m.enc_msg(2, b"\x05\x02\x10\x01"),
        "invalid_utf8_path": m.enc_msg(0, sub_body(b"/a\xff", 0, b"\x00")),
        "overlong_utf8_path": m.enc_msg(0, sub_body(b"/\xc0\xaf", 0, b"\x00")),
        "address_tag_2": m.enc_msg(0, sub_body(b"/a", 2, b"\x00")),
        "token_length_past_the_end": m.enc_msg(0, sub_body(b"/a", 0, b"\x05ab")),
        "invalid_datetime": W(5, True, (10, (0, 2_000_000_000)), 1),
        "overlong_wid": m.enc_msg(2, b"\x05\x00\x10" + b"\xff" * 10 + b"\x01"),
        "invalid_utf8_value": m.enc_msg(2, b"\x05\x00\x0c\x02\xc3\x28\x01"),
    }


def _declines():
    c = []
    good = seeded(700, 5)
    assert 3 * TILE < len(good)
    good = exactly(3 * TILE, 5)
    # message ends of the good frame, to place the bad message first, in the middle and last
    ends, pos = [0], 0
    while pos < len(good):
        L, _ = tw._varint(good, pos, len(good))
        pos += L
        ends.append(pos)
    places = {"first": 0, "middle": ends[len(ends) // 2], "last": len(good)}
    for name, bad in _bad_messages().items():
        for where, at in places.items():
            wire = good[:at] + bad + good[at:]
            c.append(Case(f"{name}_{where}", wire, "decline", tw.first_error(wire)))
    cut = good + W(5, True, (12, b"cut here"), 77)[:-4]
    c.append(Case("frame_cut_inside_the_last_message", cut, "decline", tw.first_error(cut)))
    # valid frames the fast decoder leaves to the general one (a WriteId cut short by the message
    # end is one of them: the reference reads it as "absent", to_twin._message, so the general
    # decoder's answer is NXG_WRITE_NO_WID with no error)
    m = tw.mg()
    valid = {
        "truncated_wid": m.enc_msg(2, b"\x01\x00\x10\x80"),
        "array_value": W(5, True, (19, [(9, 1), (4, 2)]), 1),
        "map_value": W(5, True, (21, [((12, b"k"), (9, 1))]), 1),
        "error_of_a_value": W(5, True, (22, (4, 5)), 1),
        "abstract_value": W(5, True, (27, bytes(range(40, 62))), 1),
        "non_canonical_length_prefix": b"\x84\x00\x01\x07\x00",  # L = 4 in two bytes
        "unsubscribe_with_trailing_bytes": tw.unsubscribe(7, trailing=b"\x00\x00"),
        "write_with_trailing_bytes": tw.write(7, True, (9, 1), 4, trailing=b"\x00"),
        "subscribe_with_trailing_bytes": tw.subscribe(b"/a", trailing=b"\x01"),
    }
    for name, msg in valid.items():
        for where, at in places.items():
            wire = good[:at] + msg + good[at:]
            err = tw.first_error(wire)
            assert err is None, (name, err)
            c.append(Case(f"{name}_{where}", wire, "decline"))
    return c


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _one_of_each() + _geometry() + _planted() + _declines()
        for seed, n in ((1, 1), (2, 700), (3, 4000)):
            _cases.append(Case(f"seeded_{n}_messages", seeded(n, seed), "must"))
        names = [k.name for k in _cases]
        assert len(set(names)) == len(names)
    return _cases


def by_class(cls):
    return [k for k in cases() if k.cls == cls]


def big_frames():
    """name -> (wire, Expect): 10^5 messages of each pure kind and of the Writes-with-an-
    Unsubscribe-every-100 mix; the expected columns come from the messages themselves
    (to_twin.batch), which tests/test_writes_cpu.py pins against the twin's decode."""
    n = 100_000
    rng = random.Random(8)
    subs = [("sub", dict(path=b"/bench/%d/leaf" % i, resolver=("v4", i, 80), timestamp=i,
                         permissions=i & 0xFF, token=b"tok%d" % (i % 1000))) for i in range(n)]
    vals = [(9, rng.getrandbits(64)) for _ in range(64)] + LEAF_VALUES
    return {
        "writes": [("w", i, bool(i & 1), vals[i % len(vals)], i * 7) for i in range(n)],
        "unsubscribes": [("unsub", i * 3) for i in range(n)],
        "subscribes": subs,
        "writes_with_an_unsubscribe_every_100":
            [("unsub", i) if i % 100 == 99 else ("w", i, True, (9, i), i) for i in range(n)],
    }
