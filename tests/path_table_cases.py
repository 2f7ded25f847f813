"""Crafted keys for the path table (NxgPathTable) and the plain-path check of Subscribe routing.
Pure Python, deterministic, no GPU.

The table's hash (netidx_amd/csrc/nxg_path_hash.h) is restated here once; tests/
test_path_table_cases_cpu.py checks the restatement against the library's nxg_path_hash. Every
step of the hash is a bijection of its 64-bit state, so it can be run backwards: for any state
before the last word and any wanted result there is exactly one last word. That gives, in
microseconds each,
  * distinct paths of equal length with the same stored hash (the table must tell them apart by
    their bytes), also as plain ASCII paths a Subscribe can carry;
  * 8-byte paths whose raw hash is 0, 1, 2 or 3 (the stored words 0 and 1 mean "empty" and
    "tombstone": raw 0 and 1 are stored as 2 and 3, next to the paths whose raw hash is 2 and 3);
  * paths whose probe starts at a chosen slot, for chains that wrap from the last slot to slot 0.
The plain-check sweep puts each defect (`\\`, `//`, a trailing `/`) at every position of paths
around the 8-byte words the kernels read.
"""
import functools
import random

M64 = 2**64 - 1
SEED = 0x243F6A8885A308D3
K_MIX = 0x9E3779B97F4A7C15
K_FIN = 0xD6E8FEB86659FD93
K_MIX_INV = pow(K_MIX, -1, 2**64)
K_FIN_INV = pow(K_FIN, -1, 2**64)


# ---- the hash, restated ---------------------------------------------------------------------------
def mix(h, w):
    h = ((h ^ w) * K_MIX) & M64
    return h ^ (h >> 29)


def words(p):
    """The little-endian 8-byte words of p, the last one zero above p's end."""
    return [int.from_bytes(p[i:i + 8], "little") for i in range(0, len(p), 8)]


def state(p, n_words=None):
    """The hash state after the first n_words words of p (default: all of them)."""
    h = SEED ^ len(p)
    for w in words(p)[:n_words]:
        h = mix(h, w)
    return h


def finish_raw(h):
    h ^= h >> 32
    h = (h * K_FIN) & M64
    return h ^ (h >> 29)


def raw_hash(p):
    """The hash before the remap of 0 and 1."""
    return finish_raw(state(p))


def stored(raw):
    return raw + 2 if raw < 2 else raw


def path_hash(p):
    """The word the table stores for p: nxg_path_hash."""
    return stored(raw_hash(p))


def home_slot(p, slots):
    """Where the table's probe for p starts."""
    return path_hash(p) & (slots - 1)


# ---- the inverses ---------------------------------------------------------------------------------
def unxorshift(y, s):
    """x with x ^ (x >> s) == y."""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def word_for(h_in, h_out):
    """The word w with mix(h_in, w) == h_out."""
    return ((unxorshift(h_out, 29) * K_MIX_INV) & M64) ^ h_in


def unfinish(raw):
    """The state h with finish_raw(h) == raw."""
    h = (unxorshift(raw, 29) * K_FIN_INV) & M64
    return unxorshift(h, 32)


def with_last_word(prefix, length, target_state):
    """prefix (a multiple of 8 bytes, length - 8 of them) + the 8 bytes that bring the hash state
    of the whole path of `length` bytes to target_state."""
    assert len(prefix) == length - 8 and length % 8 == 0
    h = SEED ^ length
    for w in words(prefix):
        h = mix(h, w)
    return prefix + word_for(h, target_state).to_bytes(8, "little")


# ---- plain-ness, by rule ----------------------------------------------------------------------------
def plain_rule(p):
    """Not empty, no `\\` byte, no `/` followed by `/`, no `/` at the end unless the path is `/`."""
    if len(p) == 0:
        return False
    for i, c in enumerate(p):
        if c == 0x5C:
            return False
        if c == 0x2F and i + 1 < len(p) and p[i + 1] == 0x2F:
            return False
    return p[-1] != 0x2F or len(p) == 1


# ---- full-hash collisions ---------------------------------------------------------------------------
@functools.lru_cache(None)
def collision_pairs():
    """Two pairs of distinct paths of equal length and equal hash, arbitrary bytes: 16 bytes that
    differ from the first word on, and 24 bytes that share the first word."""
    rng = random.Random(0xC011)
    a = rng.randbytes(16)
    b = with_last_word(rng.randbytes(8), 16, state(a))
    c = rng.randbytes(24)
    d = with_last_word(c[:8] + rng.randbytes(8), 24, state(c))
    return ((a, b), (c, d))


@functools.lru_cache(None)
def collision_triple():
    """Three distinct 16-byte paths with one hash, arbitrary bytes."""
    rng = random.Random(0x3C011)
    a = rng.randbytes(16)
    return (a, with_last_word(rng.randbytes(8), 16, state(a)),
            with_last_word(rng.randbytes(8), 16, state(a)))


@functools.lru_cache(None)
def collision_pair_at(slots, home):
    """Two distinct 16-byte paths with one hash whose probe in a table of `slots` slots starts at
    slot `home`: the wanted stored word is run backwards to the state in front of the last word."""
    rng = random.Random(slots * 1000 + home)
    target = unfinish((rng.getrandbits(64) & ~(slots - 1) | home) & M64 | 1 << 40)
    return (with_last_word(rng.randbytes(8), 16, target),
            with_last_word(rng.randbytes(8), 16, target))


_PLAIN_BYTES =bytes(c for c in range(0x21, 0x7F) if c != 0x5C)  # printable ASCII but `\`


@functools.lru_cache(None)
def plain_collision_pairs(n=3):
    """n pairs of distinct plain ASCII paths of 16 bytes with equal hashes: the second path's last
    word is the one word that collides, and about one random first word in 3000 makes it printable."""
    rng = random.Random(0xA5C11)
    letters = b"abcdefghijklmnopqrstuvwxyz0123456789_.-"
    out = []
    for k in range(n):
        a = b"/app/%02d/" % k + bytes(rng.choice(letters) for _ in range(8))
        target = state(a)
        for _ in range(2000000):
            b = with_last_word(b"/" + bytes(rng.choice(letters) for _ in range(7)), 16, target)
            if all(c in _PLAIN_BYTES for c in b[8:]) and plain_rule(b) and b != a:
                out.append((a, b))
                break
        else:
            raise RuntimeError("no plain collision found for %r" % a)
    return tuple(out)


# ---- the reserved words -----------------------------------------------------------------------------
@functools.lru_cache(None)
def reserved_paths():
    """{raw: the 8-byte path whose raw hash is raw} for raw 0, 1, 2, 3. Raw 0 and raw 2 are both
    stored as 2 (1 and 3 as 3): same stored word, same length, different bytes."""
    return {raw: word_for(SEED ^ 8, unfinish(raw)).to_bytes(8, "little") for raw in range(4)}


# ---- chains -----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def chain_paths(slots, home, n, tag=b"w"):
    """n plain paths /<tag>/<i> whose probe in a table of `slots` slots starts at slot `home`."""
    out = []
    for i in range(1000 * slots):
        p = b"/%s/%d" % (tag, i)
        if home_slot(p, slots) == home:
            out.append(p)
            if len(out) == n:
                return tuple(out)
    raise RuntimeError("no %d paths with home slot %d of %d" % (n, home, slots))


def wrap_paths(slots=16):
    """(four paths whose home is the last slot, so their chain wraps to slot 0; three more whose
    home is the slot before it, whose chain runs through slots - 2, slots - 1 and 0)."""
    return chain_paths(slots, slots - 1, 4), chain_paths(slots, slots - 2, 3, b"v")


# ---- the plain-check sweep --------------------------------------------------------------------------
SWEEP_LENGTHS = tuple(range(1, 19)) + (23, 24, 25)


def clean_path(n):
    """A plain path of n bytes: `/` and letters (no further `/`)."""
    return (b"/" + bytes(0x61 + (i * 7 + n) % 26 for i in range(n - 1)))[:n]


@functools.lru_cache(None)
def sweep():
    """((path, plain), ...): for every length of SWEEP_LENGTHS the clean path and the path with a
    trailing `/`; for every position of it the path with `\\` there, with `//` starting there, and
    (lengths 9, 17 and 24: the word boundaries) with a single `/` there; the clean path again
    after every third position, as a plain span between two stops. Then `/` alone. The expected
    plain-ness is plain_rule's."""
    out = []

    def add(p):
        out.append((bytes(p), plain_rule(bytes(p))))

    for n in SWEEP_LENGTHS:
        c = clean_path(n)
        add(c)
        add(c[:-1] + b"/")
        for i in range(n):
            add(c[:i] + b"\\" + c[i + 1:])
            if i + 1 < n:
                add(c[:i] + b"//" + c[i + 2:])
            if n in (9, 17, 24) and i > 0:
                add(c[:i] + b"/" + c[i + 1:])
            if i % 3 == 2:
                add(c)  # a plain span between two stops
    add(b"/")
    return tuple(out)


def all_crafted():
    """Every crafted path of this file, for checks that sweep over them."""
    ps = [p for pair in collision_pairs() + plain_collision_pairs() for p in pair]
    ps += list(collision_triple()) + list(reserved_paths().values())
    for slots in (16, 128):
        a, b = wrap_paths(slots)
        ps += list(a) + list(b) + list(collision_pair_at(slots, slots - 1))
    ps += [p for p, _ in sweep()]
    return ps
