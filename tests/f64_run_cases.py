"""The case table of tests/test_gpu_f64_run.py and tests/test_gpu_f64_ranges.py (test
infrastructure, no GPU): crafted f64 frames for every per-tile choice of the length-run decoder
(nxg_decode_f64_run.hip) and every cut position of the byte-range decode (nxg_decode_range).

  constants()   the kernels' tile sizes, sampling stride, bail ratio and the host's countdown
                lengths, read from the sources; the statements tile_plan() restates are matched
                too (_SHAPES), so a retune or a rewrite fails tests/test_f64_run_cases_cpu.py
  records()     an independent pure-Python parser of f64 frames (no code shared with the oracle
                or the kernels)
  tile_plan()   a sequential restatement of probe_fast + run_search + the bail rule: the class of
                every tile of a byte range -- end | one_run | predicted_two | searched_two | exact
                -- and the frame's verdict (exact tiles, bail to the single-pass decoder, not f64)
  CASES         whole-frame cases (W1..W11), each naming the tile and the class it is there for
  RCASES        byte-range cases (R1..R7): a frame and the lists of cuts it is decoded at

Every frame is built by frame() from ids and values whose bytes are all >= 0x20, so that no byte
pair outside a record header reads as a candidate start (a byte in 12..16 followed by 04); the
cases that plant a false record put it in one named value.
"""
import functools
import os
import re
from typing import NamedTuple, Optional, Tuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "netidx_amd", "csrc")

F_FORCE_EXACT, F_NO_BAIL = 1, 2
CLASSES = ("end", "one_run", "predicted_two", "searched_two", "exact")
ROUTE_GENERAL, ROUTE_RUN, ROUTE_X, ROUTE_MIX, ROUTE_SEQ = 0, 1, 2, 3, 4  # Codec.last_route()[0]

_CONSTS = {
    "nxg_decode_f64_run.hip": {
        "T": r"#define NXG_F64R_T (\d+)",
        "EREC": r"#define NXG_F64R_EREC (\d+)",
        "TPB": r"constexpr int TPB = (\d+);",
        "BAIL": r"\(uint64_t\)nirr \* (\d+) > ntg",
        "GUARD_AHEAD": r"const bool guard = t0 \+ T \+ (\d+) > W;",
        "PRE": r"const uint64_t pre = begin < (\d+) \? begin : \d+;",
    },
    "nxg_f64_rec16.h": {
        "WIN": r"constexpr int WIN = (\d+);",
        "kXSub": r"constexpr uint32_t kXSub = (\d+);",
        "kXLo": r"constexpr uint32_t kXLo = (\d+);",
        "kXHalo": r"constexpr uint32_t kXHalo = (\d+);",
    },
    "nxg_decode_f64_x.hip": {
        "SUB": r"constexpr uint32_t SUB = (\d+);",
        "SPW": r"#define NXG_F64X_SPW (\d+)",
        "X_TPB": r"constexpr int TPB = (\d+);",
        "X_WAVE": r"constexpr int WAVES = TPB / (\d+);",
    },
    "nxg_api.cpp": {
        "kIrregularCalls": r"constexpr uint32_t kIrregularCalls = (\d+);",
        "kSeqSkipCalls": r"constexpr uint32_t kSeqSkipCalls = (\d+);",
        "kMixFailCalls": r"constexpr uint32_t kMixFailCalls = (\d+);",
    },
}
# What the table below was laid out for. A retune changes constants() and the frames follow it;
# tests/test_f64_run_cases_cpu.py then fails here until the cases have been read against the new
# values (which sub-wave boundaries a run tile crosses, which cuts are edges) and this is updated.
PINNED = {"T": 32768, "EREC": 256, "ESUB": 11, "TPB": 256, "BAIL": 8, "GUARD_AHEAD": 32,
          "PRE": 64, "WIN": 64, "kXSub": 4096, "kXLo": 64, "kXHalo": 128, "SUB": 4096, "SPW": 4,
          "WAVES": 4, "kIrregularCalls": 64, "kSeqSkipCalls": 64, "kMixFailCalls": 16}
# statements tile_plan() restates: if one changes shape, the model has to be read against it again
_SHAPES = {
    "nxg_decode_f64_run.hip": {
        "ESUB expression": r"constexpr uint32_t ESUB = \(T / 12 \+ EREC\) / EREC;",
        "window test": r"s1 < 16 && V == \(\(1u << s1\) \| \(p2 < 16 \? 1u << p2 : 0u\)\)",
        "end-of-range test": r"s1 < 16 && \(s1 == rem0 \|\| s1 >= lim\)",
        "width prediction": r"if \(nb < 5 && id0 < next && id0 \+ n > next\)",
        "three-sample check":
            r"bool ok = lok && ia == id0 \+ m && ie == id0 \+ ke && iff == id0 \+ kf;",
        "middle sample": r"ok = rec_at\(wire, W, t0, at\(m / 2\), ib\) == L;",
        "sample stride": r"const uint32_t step = \(n1 \+ 62\) / 63;",
        "second-run samples": r"lane == 63 \? n2 - 1 : lane \* \(n2 - 1\) / 63;",
        "irregular count": r"const int nirr = __syncthreads_count\(state != 0\);",
        "not-f64 test": r"nof = V == 0u \|\| \(t == 0 && first && !\(V & 1u\)\);",
    },
    "nxg_f64_rec16.h": {}, "nxg_decode_f64_x.hip": {}, "nxg_api.cpp": {
        "hand-over to the single-pass decoder":
            r"tried_fast == FAST_RUN && len > 0 && h\.fast_fail && \(h\.irregular & 3u\) == 1u",
    },
}


@functools.lru_cache(maxsize=None)
def constants():
    """The kernels' constants, read from their sources. A constant or a restated statement that
    is not found is an error: the cases below would otherwise stop reaching their branch without
    any test saying so."""
    out, missing = {}, []
    for fname, pats in _CONSTS.items():
        with open(os.path.join(CSRC, fname)) as f:
            src = f.read()
        for name, pat in pats.items():
            m = re.search(pat, src)
            if m is None:
                missing.append(f"{fname}: {name} (/{pat}/)")
            else:
                out[name] = int(m.group(1), 0)
        for name, pat in _SHAPES[fname].items():
            if re.search(pat, src) is None:
                missing.append(f"{fname}: the {name} statement (/{pat}/)")
    if missing:
        raise RuntimeError("tests/f64_run_cases.py restates these from the kernel sources and no "
                           "longer finds them; re-read tile_plan() against the kernels:\n  " +
                           "\n  ".join(missing))
    out["ESUB"] = (out["T"] // 12 + out["EREC"]) // out["EREC"]
    out["WAVES"] = out.pop("X_TPB") // out.pop("X_WAVE")
    out["X_WAVE_BYTES"] = out["SUB"] * out["SPW"]
    out["X_WG_BYTES"] = out["X_WAVE_BYTES"] * out["WAVES"]
    return out


# ---- frames ----------------------------------------------------------------------------------
def id_width(ids):
    """varint bytes of each id (< 2^35)."""
    ids = np.asarray(ids, np.uint64)
    w = np.ones(len(ids), np.int64)
    for t in (7, 14, 21, 28):
        w += ids >= np.uint64(1 << t)
    return w


def safe_values(n, seed):
    """n f64 bit patterns whose eight bytes are all >= 0x20."""
    b = np.random.default_rng(seed).integers(0x20, 0x100, (n, 8), dtype=np.uint8)
    return b.view(">u8").reshape(n).astype(np.uint64)


def frame(ids, vals):
    """The wire bytes of From::Update(id, F64(v)) records: L 04 varint(id) 09 f64be."""
    ids = np.asarray(ids, np.uint64)
    vals = np.asarray(vals, np.uint64)
    n = len(ids)
    assert n == len(vals) and (n == 0 or int(ids.max()) < 1 << 35)
    nb = id_width(ids)
    L = 11 + nb
    start = np.concatenate([[0], np.cumsum(L)])[:n].astype(np.int64)
    w = np.zeros(int(L.sum()), np.uint8)
    w[start] = L
    w[start + 1] = 4
    for j in range(5):
        m = nb > j
        g = ((ids[m] >> np.uint64(7 * j)) & np.uint64(0x7f)).astype(np.uint8)
        g |= np.where(nb[m] > j + 1, 0x80, 0).astype(np.uint8)
        w[start[m] + 2 + j] = g
    w[start + 2 + nb] = 9
    vb = vals.astype(">u8").view(np.uint8).reshape(n, 8)
    for j in range(8):
        w[start + 3 + nb + j] = vb[:, j]
    return w


class Records(NamedTuple):
    start: np.ndarray   # int64
    length: np.ndarray  # int64
    id: np.ndarray      # uint64
    value: np.ndarray   # uint64


def records(wire):
    """An f64 frame parsed record by record: a length byte, 04, a canonical varint id below 2^35,
    09 and eight big-endian value bytes; the length byte must be the record's length. Raises
    ValueError (with the offset) on anything else."""
    b = bytes(wire)
    W, p = len(b), 0
    st, ln, ids, vals = [], [], [], []
    while p < W:
        L = b[p]
        if not 12 <= L <= 16 or p + L > W:
            raise ValueError(f"length byte {L} at {p} of {W}")
        if b[p + 1] != 4:
            raise ValueError(f"variant {b[p + 1]} at {p + 1}")
        q, v, sh = p + 2, 0, 0
        while True:
            c = b[q]
            v |= (c & 0x7f) << sh
            sh += 7
            q += 1
            if not c & 0x80:
                break
            if sh >= 35:
                raise ValueError(f"id varint too long at {p + 2}")
        if q - p - 2 > 1 and c == 0:
            raise ValueError(f"id varint not canonical at {p + 2}")
        if q + 9 != p + L:
            raise ValueError(f"record at {p}: length byte {L}, id of {q - p - 2} bytes")
        if b[q] != 9:
            raise ValueError(f"value tag {b[q]} at {q}")
        st.append(p)
        ln.append(L)
        ids.append(v)
        vals.append(int.from_bytes(b[q + 1:q + 9], "big"))
        p += L
    return Records(np.array(st, np.int64), np.array(ln, np.int64), np.array(ids, np.uint64),
                   np.array(vals, np.uint64))


def candidates(wire):
    """Positions whose byte is in 12..16 and is followed by 04."""
    w = np.asarray(wire, np.uint8)
    if len(w) < 2:
        return np.zeros(0, np.int64)
    return np.flatnonzero((w[:-1] >= 12) & (w[:-1] <= 16) & (w[1:] == 4))


# ---- the tile model ----------------------------------------------------------------------------
def _rec(b, p, W):
    """(L, id) of the valid record at p of the W-byte frame b (bytes past W read as zero), or
    (0, None): rec_check16 + rec_decode16."""
    def at(i):
        return b[i] if i < W else 0
    L = at(p)
    if not 12 <= L <= 16 or at(p + 1) != 4:
        return 0, None
    nb = L - 11
    v = 0
    for j in range(nb):
        c = at(p + 2 + j)
        if bool(c & 0x80) != (j < nb - 1):
            return 0, None
        v |= (c & 0x7f) << (7 * j)
    if at(p + 2 + nb) != 9 or W - p < L:
        return 0, None
    return L, v


class Tile(NamedTuple):
    cls: str
    entry: int
    count: int
    ks: int
    L: int
    L2: int
    x: int


class Plan(NamedTuple):
    tiles: Tuple[Tile, ...]
    n_exact: int     # tiles on the exact walk (DevStatus.diag[0]); 0 after a bail
    bails: bool      # handed to the single-pass decoder (irregular bit 0)
    not_f64: bool    # some 16-byte window holds no record start (irregular bit 1)
    off_model: int   # tiles the probe's one-lane model did not settle (the bail rule's count)


def _ceil(a, b):
    return -(-a // b)


def _run_search(b, W, t0, e, L, lim):
    """run_search: (ks, L2, n, x) of a two-run tile, or None."""
    n1 = _ceil(lim - e, L)
    step = (n1 + 62) // 63
    ki = [n1 - 1 if lane == 63 else min(lane * step, n1 - 1) for lane in range(64)]
    good = [_rec(b, t0 + e + k * L, W)[0] == L for k in ki]
    if all(good):
        return None
    ib = good.index(False)
    khi = ki[ib]
    klo = ki[ib - 1] + 1 if ib else 0
    k2 = [min(klo + lane, khi) for lane in range(64)]
    l2 = [_rec(b, t0 + e + k * L, W)[0] for k in k2]
    j = next(i for i, x in enumerate(l2) if x != L)
    ks, L2 = klo + j, l2[j]
    if L2 == 0 or L2 == L:
        return None
    p2 = e + ks * L
    n2 = _ceil(lim - p2, L2)
    kc = [n2 - 1 if lane == 63 else lane * (n2 - 1) // 63 for lane in range(64)]
    if not all(_rec(b, t0 + p2 + k * L2, W)[0] == L2 for k in kc):
        return None
    return ks, L2, ks + n2, p2 + n2 * L2


def tile_plan(wire, begin=0, end=None, flags=0):
    """The length-run probe's verdict on the records that start in [begin, end) of the frame:
    probe_fast, run_search and the bail rule restated one tile after another (frames of at most
    TPB tiles: one probe workgroup). Exact tiles take entry, count and x from records()."""
    k = constants()
    T = k["T"]
    b = bytes(wire)
    Wf = len(b)
    end = Wf if end is None else end
    assert 0 <= begin <= end <= Wf
    R = end - begin
    nt = _ceil(R, T)
    assert nt <= k["TPB"]
    first = begin == 0
    tiles, states, nof_any, bad0 = [], [], False, False
    for t in range(nt):
        a0 = begin + t * T          # frame position of the tile
        lim = min(R - t * T, T)
        rem0 = Wf - a0
        V = 0
        if rem0 < 16:
            V |= 1 << rem0
        for s in range(16):
            if _rec(b, a0 + s, Wf)[0]:
                V |= 1 << s
        s1 = (V & -V).bit_length() - 1 if V else 32
        L1 = b[a0 + s1] if s1 < 16 and s1 != rem0 else 0
        p2 = s1 + L1
        nof = V == 0 or (t == 0 and first and not V & 1)
        nof_any |= nof
        tile, state = None, 0
        if t == 0 and first and not V & 1:
            bad0 = True
            tile = Tile("exact", 0, 0, 0, 0, 0, 0)
        elif s1 < 16 and (s1 == rem0 or s1 >= lim):
            tile = Tile("end", s1, 0, 0, 12, 12, s1)
        elif s1 < 16 and V == ((1 << s1) | (1 << p2 if p2 < 16 else 0)):
            e, L = s1, L1
            L2 = L
            n = _ceil(lim - e, L)
            ks = n
            id0 = _rec(b, a0 + e, Wf)[1]
            nb = L - 11
            nxt = 1 << (7 * nb)
            if nb < 5 and id0 < nxt and id0 + n > nxt:
                ks = nxt - id0
                L2 = L + 1
                n = ks + _ceil(lim - (e + ks * L), L2)

            def at(i):
                return e + i * L if i < ks else e + ks * L + (i - ks) * L2

            def ln(i):
                return L if i < ks else L2
            m = n - 1
            ke, kf = (ks - 1, ks) if ks < n else (m, m)
            sa, se, sf = (_rec(b, a0 + at(i), Wf) for i in (m, ke, kf))
            lok = sa[0] == ln(m) and se[0] == ln(ke) and sf[0] == ln(kf)
            ok = lok and sa[1] == id0 + m and se[1] == id0 + ke and sf[1] == id0 + kf
            if not ok and lok and ks == n:
                ok = _rec(b, a0 + at(m // 2), Wf)[0] == L
            if ok:
                tile = Tile("one_run" if ks == n else "predicted_two", e, n, ks, L, L2, at(n))
            else:
                state = 1
                tile = (e, L, lim)
        else:
            state = 2
        if flags & F_FORCE_EXACT and not bad0:
            state = 2
        tiles.append(tile)
        states.append(state)
    off_model = sum(s != 0 for s in states)
    bail = not flags & F_NO_BAIL and (nof_any or off_model * k["BAIL"] > nt)
    if bail:
        return Plan(tuple(t if isinstance(t, Tile) else None for t in tiles), 0, not nof_any,
                    nof_any, off_model)
    rec = None
    out = []
    for t in range(nt):
        tile, state = tiles[t], states[t]
        a0, lim = begin + t * T, min(R - t * T, T)
        if state == 1:
            e, L, lim = tile
            r = _run_search(b, Wf, a0, e, L, lim)
            if r is None:
                state = 2
            else:
                tile = Tile("searched_two", e, r[2], r[0], L, r[1], r[3])
        if state == 2:
            if rec is None:
                rec = records(wire)
            S = rec.start
            i0, i1 = np.searchsorted(S, [a0, a0 + lim])
            ent = (int(S[i0]) if i0 < len(S) else Wf) - a0
            ex = (int(S[i1]) if i1 < len(S) else Wf) - a0
            tile = Tile("exact", ent, int(i1 - i0), 0, 0, 0, ex)
        out.append(tile)
    return Plan(tuple(out), sum(t.cls == "exact" for t in out), False, False, off_model)


# ---- id and length builders --------------------------------------------------------------------
def band_ids(nb, n, mul=7, mod=1000):
    """n ids of nb varint bytes, not consecutive, all within `mod` of the band's lowest id, so
    that no tile's first id plus its record count reaches the next width (nb >= 2)."""
    lo = 0 if nb == 1 else 1 << (7 * (nb - 1))
    return (lo + (mul * np.arange(n, dtype=np.int64)) % (min(mod, 128) if nb == 1 else mod)
            ).astype(np.uint64)


def ids_of_lengths(lens):
    """Non-consecutive ids whose records have the given lengths (12..16)."""
    lens = np.asarray(lens, np.int64)
    out = np.zeros(len(lens), np.uint64)
    for L in range(12, 17):
        m = lens == L
        out[m] = band_ids(L - 11, int(m.sum()))
    return out


def false_value(L=12):
    """Eight value bytes whose bytes 1.. read as a complete record header of length L <= 14:
    41 L 04 varint(L - 11 bytes) 09, then bytes >= 0x20 (tests/test_gpu_fullsize.py
    _false_record). The false start is the value's second byte."""
    nb = L - 11
    b = [0x41, L, 0x04] + [0xa5] * (nb - 1) + [0x33, 0x09]
    b += [0x77] * (8 - len(b))
    return int.from_bytes(bytes(b), "big")


def plant(ids, vals, lo):
    """vals with one false record planted so that its false start lies in [lo, lo + 16): returns
    (vals, record index, false start)."""
    nb = id_width(ids)
    L = 11 + nb
    start = np.concatenate([[0], np.cumsum(L)])[:len(ids)]
    fs = start + 3 + nb + 1  # each record's value byte 1
    k = int(np.flatnonzero((fs >= lo) & (fs < lo + 16))[0])
    vals = np.array(vals, np.uint64)
    vals[k] = false_value(12)
    return vals, k, int(fs[k])


def two_run_consecutive(total, L, near_half=True, ks=None):
    """Consecutive ids crossing 2^(7(L-11)): ks records of L bytes, then b of L + 1, `total`
    bytes together. Returns (ids, ks)."""
    B = 1 << (7 * (L - 11))
    b = total % L
    if ks is None:
        q = (total // 2) // (L * (L + 1)) if near_half else 0
        b += L * q
    else:
        while (total - b * (L + 1)) // L > ks:
            b += L
    ks = (total - b * (L + 1)) // L
    assert ks >= 0 and ks * L + b * (L + 1) == total and 0 <= B - ks
    return (B - ks + np.arange(ks + b)).astype(np.uint64), ks


# ---- whole-frame cases -------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    family: str            # W1..W11
    ids: Optional[np.ndarray]
    seed: int
    tile: int              # the tile the case is there for
    cls: str               # ... and the class it must reach
    ks: Optional[int] = None      # the split the model must find there
    count: Optional[int] = None   # the tile's record count the table promises
    wlen: Optional[int] = None    # the frame length the table promises
    ctx: str = "run"
    planted: Optional[int] = None     # lo of the 16-byte window a false start is planted in
    corrupt: Optional[Tuple[int, str]] = None  # (record, kind): W11
    heartbeat: Optional[int] = None   # record index a Heartbeat (02 05) is inserted before
    bail: Optional[bool] = None       # the verdict promised without F_NO_BAIL
    note: str = ""


@functools.lru_cache(maxsize=None)
def _built(name):
    c = BY_NAME[name]
    vals = safe_values(len(c.ids), c.seed)
    info = {}
    if c.planted is not None:
        vals, k, fs = plant(c.ids, vals, c.planted)
        info["false_start"], info["planted_record"] = fs, k
    w = frame(c.ids, vals)
    if c.corrupt is not None:
        r, kind = c.corrupt
        nb = id_width(c.ids)
        p = int((11 + nb)[:r].sum())
        w = w.copy()
        if kind == "tag":
            assert w[p + 2 + nb[r]] == 9
            w[p + 2 + nb[r]] = 8
        elif kind == "variant":
            w[p + 1] = 5
        elif kind == "length":
            assert w[p] == 13
            w[p] = 12
        elif kind == "continuation":
            assert w[p + 2] & 0x80
            w[p + 2] &= 0x7f
        else:
            raise KeyError(kind)
        info["corrupt_at"] = p
    if c.heartbeat is not None:
        p = int((11 + id_width(c.ids))[:c.heartbeat].sum())
        w = np.concatenate([w[:p], np.array([2, 5], np.uint8), w[p:]])
        info["heartbeat_at"] = p
    w.setflags(write=False)
    return w, vals, info


def wire(name):
    return _built(name)[0]


def values(name):
    return _built(name)[1]


def info(name):
    return _built(name)[2]


def _cases():
    k = constants()
    T, EREC = k["T"], k["EREC"]
    out = []

    def add(name, family, ids, tile, cls, seed=None, **kw):
        out.append(Case(name, family, np.asarray(ids, np.uint64), seed or len(out) + 1, tile, cls,
                        **kw))

    # W1 one_run: one length per frame, ids not consecutive and far below the next width
    for L in (13, 14, 15, 16):
        for nt in (1, 2, 3):
            n = (nt * T - 100) // L
            add(f"W1-L{L}-{nt}t", "W1", band_ids(L - 11, n), nt - 1, "one_run")
    add("W1-L12-100", "W1", band_ids(1, 100, mod=20), 0, "one_run", count=100)
    # the companion of decode_bounds_cases: one-byte ids, more than 127 records in the tile
    add("W1-L12-companion", "W1", band_ids(1, 2 * T // 12 - 10), 0, "exact")
    # W2 predicted_two: consecutive ids crossing a width inside a tile
    for nb in (1, 2, 3, 4):
        B, L = 1 << (7 * nb), 11 + nb
        n = 120 if nb == 1 else 1000
        for ks in (1, 2, n // 2, n - 1):
            add(f"W2-x{7 * nb}-t0-ks{ks}", "W2", B - ks + np.arange(n), 0, "predicted_two", ks=ks,
                count=n)
        if nb == 1:
            continue  # (at most 128 records precede 2^7: the crossing cannot be in a later tile)
        f = _ceil(T, L)  # tile 1's first record; its entry is f * L - T != 0
        assert f * L - T != 0
        n = 800
        for ks in (1, 2, n // 2, n - 1):
            add(f"W2-x{7 * nb}-t1-ks{ks}", "W2", B - f - ks + np.arange(f + n), 1,
                "predicted_two", ks=ks, count=n)
    # W3 searched_two: a width change inside tile 0, ids not consecutive; tile 0 is full
    # (lim = T), so n1 and the sample stride depend on L alone
    for L, L2 in ((12, 13), (15, 16), (12, 14), (14, 12), (16, 15)):
        n1 = _ceil(T, L)
        step = (n1 + 62) // 63
        for label, ks in (("1", 1), ("onstep", 10 * step), ("step+1", 10 * step + 1),
                          ("step-1", 10 * step - 1), ("mid", n1 // 2), ("n1-1", n1 - 1)):
            n2 = _ceil(T + 200 - ks * L, L2)
            lens = np.concatenate([np.full(ks, L), np.full(n2, L2)])
            add(f"W3-{L}to{L2}-ks{label}", "W3", ids_of_lengths(lens), 0, "searched_two", ks=ks)
    # W4 exact by shape
    third = T // 3 // 14
    add("W4-three-runs", "W4", ids_of_lengths(np.concatenate(
        [np.full(third, 13), np.full(third, 14), np.full(third + 300, 15)])), 0, "exact")
    add("W4-alternating", "W4", ids_of_lengths(np.tile([13, 14], T // 27 + 50)), 0, "exact")
    # W5 entry phase: j records of 15 bytes, then 16-byte records to the tile edge: tile 1's
    # entry is (-j) mod 16; tile 1 holds 100 records of 12 bytes (two true starts in its window
    # for an entry <= 3)
    for j in range(16):
        m = _ceil(T - 15 * j, 16)
        ent = 15 * j + 16 * m - T
        lens = np.concatenate([np.full(j, 15), np.full(m, 16), np.full(100, 12)])
        ids = ids_of_lengths(lens)
        ids[j + m:] = band_ids(1, 100, mod=20)
        add(f"W5-entry{ent}", "W5", ids, 1, "one_run", count=100, note=str(ent))
    # W6 a false candidate in tile 1's window
    n = (3 * T - 100) // 14
    add("W6-false-start", "W6", band_ids(3, n), 1, "exact", planted=T)
    # W7 frame end
    for r in (0, 1, 11, 12, 15, 16, 17):
        ids, _ = two_run_consecutive(T + r, 13)
        # (T + 12 here: the tail of a record that starts in tile 0; W7-T+12-alone is the other)
        add(f"W7-T+{r}", "W7", ids, 1 if r else 0, "end" if r and r <= 12 else
            ("predicted_two" if r == 0 else "one_run"), wlen=T + r)
    ids, _ = two_run_consecutive(2 * T, 13)
    add("W7-2T", "W7", ids, 1, "one_run", wlen=2 * T)
    add("W7-T+12-alone", "W7", np.concatenate([band_ids(5, T // 16), [5]]), 1, "one_run",
        wlen=T + 12, count=1)
    for L in (12, 13, 14, 15):
        add(f"W7-one-record-{L}", "W7", band_ids(L - 11, 1), 0, "one_run", wlen=L, count=1)
    # W8 emit sub-waves: the last, short tile sets the count; tile 0 holds an odd (14-byte
    # records) or an even (16-byte records) number of rows, which is the short tile's base.
    # A run tile holds at most ceil(T / 13) records (12-byte records have one-byte ids, of which
    # a run tile takes 128), so 10 * EREC - 1 .. 10 * EREC + 1 cannot be reached: 9 * EREC is
    # the last sub-wave boundary a run tile crosses.
    top = 9 * EREC
    assert top + 1 <= (T - 16) // 14 and 10 * EREC - 1 > _ceil(T, 13)
    for L0 in (14, 16):
        n0 = _ceil(T, L0)
        for c in (1, 63, 64, 65, EREC - 1, EREC, EREC + 1, top - 1, top, top + 1):
            lens = np.concatenate([np.full(n0, L0), np.full(c, 14)])
            add(f"W8-base{n0 & 1}-count{c}", "W8", ids_of_lengths(lens), 1, "one_run", count=c,
                note=f"base&1={n0 & 1}")
    add("W8-full-12", "W8", band_ids(1, _ceil(T, 12) + 50), 0, "exact", count=_ceil(T, 12))
    for ks in (EREC - 1, EREC, EREC + 1):
        add(f"W8-split-ks{ks}", "W8", (1 << 14) - ks + np.arange(1000), 0, "predicted_two", ks=ks,
            count=1000)
    # W9 guard: tile 1 full, once the frame's last full tile with fewer than GUARD_AHEAD bytes
    # behind it, once with more
    n = _ceil(2 * T, 14)
    assert n * 14 - 2 * T < k["GUARD_AHEAD"] <= (n + 3) * 14 - 2 * T
    add("W9-guarded", "W9", band_ids(3, n), 1, "one_run", wlen=n * 14, seed=9009)
    add("W9-unguarded", "W9", band_ids(3, n + 3), 1, "one_run", wlen=(n + 3) * 14, seed=9009)
    # W10 bail threshold: one exact tile (a planted false start in tile 1's window) in BAIL
    # tiles is kept, in BAIL - 1 tiles it is not
    for nt in (k["BAIL"], k["BAIL"] - 1):
        n = (nt * T - 100) // 14
        add(f"W10-{nt}-tiles", "W10", band_ids(3, n), 1, "exact", planted=T,
            bail=nt < k["BAIL"])
    # a Heartbeat behind a 16-byte record that ends 14 bytes into tile 1: bytes [T, T + 16) hold
    # no record start
    lens = np.concatenate([[14], np.full(T // 16, 16), np.full(300, 16)])
    add("W10-heartbeat", "W10", ids_of_lengths(lens), 1, "exact", heartbeat=T // 16 + 1,
        bail=True)
    # W11 malformed where the probe does not look: record 7 of a one-run and of a two-run tile
    for kind in ("tag", "variant", "length", "continuation"):
        add(f"W11-one-run-{kind}", "W11", band_ids(2, 1000), 0, "one_run", corrupt=(7, kind))
        add(f"W11-two-run-{kind}", "W11", (1 << 14) - 500 + np.arange(1000), 0, "predicted_two",
            ks=500, corrupt=(7, kind))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def clean(c):
    """The case's frame is a well-formed f64 frame (records() parses it)."""
    return c.corrupt is None and c.heartbeat is None


def pristine(c):
    """The frame of a W11 case before its byte was corrupted (the probe's view of the tile)."""
    return frame(c.ids, safe_values(len(c.ids), c.seed))


# ---- byte-range cases ----------------------------------------------------------------------------
class RCase(NamedTuple):
    name: str
    family: str
    ids: np.ndarray
    seed: int
    cuts: Tuple[Tuple[int, ...], ...]  # each: the inner boundaries of one decode of the frame
    planted: Optional[int] = None
    ctx: str = "default"
    offsets: bool = False   # also with the frame 1 and 8 bytes off its allocation
    heartbeat: Optional[int] = None   # record index a Heartbeat (02 05) is inserted before


@functools.lru_cache(maxsize=None)
def _rbuilt(name):
    c = RBY_NAME[name]
    vals = safe_values(len(c.ids), 1000 + c.seed)
    inf = {}
    if c.planted is not None:
        vals, kk, fs = plant(c.ids, vals, c.planted)
        inf["false_start"] = fs
    w = frame(c.ids, vals)
    if c.heartbeat is not None:
        p = int((11 + id_width(c.ids))[:c.heartbeat].sum())
        w = np.concatenate([w[:p], np.array([2, 5], np.uint8), w[p:]])
        inf["heartbeat_at"] = p
    w.setflags(write=False)
    return w, inf


def rvalues(name):
    c = RBY_NAME[name]
    return safe_values(len(c.ids), 1000 + c.seed)


def rwire(name):
    return _rbuilt(name)[0]


def rinfo(name):
    return _rbuilt(name)[1]


def _windows(W, T, edges):
    """R1 / R5's cut sets, by name."""
    out = {"head": range(1, 81), "middle": range(T + T // 2 - 24, T + T // 2 + 24),
           "tail": range(W - 40, W + 1)}
    for e in edges:
        out[f"edge{e}"] = range(e - 24, e + 25)
    return out


def _rcases():
    k = constants()
    T = k["T"]
    out = []

    def add(name, family, ids, cuts, **kw):
        out.append(RCase(name, family, np.asarray(ids, np.uint64), len(out) + 1,
                         tuple(tuple(c) for c in cuts), **kw))

    def sweep(name, family, ids, edges, ctx="default"):
        W = int((11 + id_width(ids)).sum())
        for wn, cs in _windows(W, T, edges).items():
            add(f"{name}-{wn}", family, ids, [(c,) for c in cs], offsets=True, ctx=ctx)

    # R1: one record length per frame, and a frame with a predicted split in tile 1
    for L in (12, 13, 14, 15, 16):
        sweep(f"R1-L{L}", "R1", band_ids(L - 11, (3 * T + 500) // L), (T,))
    # On the default context a range of at most 5 tiles with one tile off the run model is
    # handed to the single-pass decoder (1 * BAIL > 5), so the 12-byte frame, whose tiles the
    # probe does not settle, never meets the run decoder's exact walk there. The same sweep on
    # the context that never hands over (NXG_F64R_FLAGS=2) does: exact_tile in range mode at
    # every look-behind 1..64, at the tile edge and at the frame end.
    sweep("R1x-L12", "R1", band_ids(1, (3 * T + 500) // 12), (T,), ctx="run")
    f = _ceil(T, 13)
    sweep("R1-split", "R1", (1 << 14) - f - 700 + np.arange((3 * T + 500) // 14 + 100), (T,))
    # R2: three ranges, the middle one tiny: starting one byte behind a record start (no start
    # inside while it is shorter than the record) and on a record start
    for L in (13, 16):
        ids = band_ids(L - 11, (3 * T + 500) // L)
        s = (T + T // 2) // L * L
        cuts = [(a, a + m) for a in (s + 1, s) for m in (0, 1, 11, 12, 15, 16, 17, 31)]
        add(f"R2-L{L}", "R2", ids, cuts)
    # R3: the cut on, one before and one behind the first record of the new width
    n = (3 * T + 500) // 14
    ids, ks = (1 << 14) - 3000 + np.arange(n), 3000
    add("R3-predicted", "R3", ids, [(13 * ks + d,) for d in (-1, 0, 1)])
    lens = np.concatenate([np.full(3000, 16), np.full(n, 15)])
    add("R3-searched", "R3", ids_of_lengths(lens), [(16 * 3000 + d,) for d in (-1, 0, 1)])
    # (the same on the context that never hands over: run_search in a range's tile)
    # (and a cut 5000 bytes before the change, which then lies inside the second range's tile 0)
    add("R3x-searched", "R3", ids_of_lengths(lens),
        [(16 * 3000 + d,) for d in (-1, 0, 1, -5000)], ctx="run")
    # R4: a false record near the cut: the false start in [c, c + 16), in [c - 64, c), and (the
    # first range's view) in the last 16 bytes before its end
    ids = band_ids(3, (3 * T + 500) // 14)
    lo = T + T // 2
    fs = plant(ids, safe_values(len(ids), 0), lo)[2]
    for ctx in ("default", "run"):
        add(f"R4-{ctx}", "R4", ids, [(c,) for c in range(fs - 15, fs + 65)], planted=lo, ctx=ctx)
    # R5: ids of random width (the run probe declines, the single-pass decoder takes the range)
    rng = np.random.default_rng(5)
    n = (5 * T) // 14
    bits = rng.choice([7, 14, 21, 28, 35], n)
    ids = rng.integers(0, 2**62, n, dtype=np.uint64) >> (62 - bits).astype(np.uint64)
    sweep("R5", "R5", ids, (k["SUB"], 2 * k["SUB"], 3 * k["SUB"], k["X_WAVE_BYTES"],
                            k["X_WG_BYTES"]))
    # R6: range ends: [b, e) of a 13-byte-record frame
    ids = band_ids(2, (3 * T + 500) // 13)
    b0 = 1000
    add("R6-middle", "R6", ids, [(b0, b0 + T // 2 + d) for d in range(-16, 16)])
    add("R6-tile-edge", "R6", ids, [(b0, b0 + T + d) for d in range(-16, 17)])
    # R7 (beside the issue's list, for the not-f64 verdict in range mode): a Heartbeat between
    # two records in the middle of tile 1; the f64 decoders decline the range that holds it
    n = (3 * T + 500) // 16
    hb = (T + T // 2) // 16
    a = 16 * hb  # the Heartbeat's position: record starts at a - 16 and a + 2
    add("R7-heartbeat", "R7", band_ids(5, n),
        [(a - 15,), (a - 14,), (a - 40,), (a + 1,), (T, 2 * T)], heartbeat=hb)
    return out


RCASES = _rcases()
RBY_NAME = {c.name: c for c in RCASES}
assert len(RBY_NAME) == len(RCASES)


def ranges_of(W, cuts):
    """[(begin, end)] of a frame of W bytes cut at `cuts`."""
    edges = [0] + [min(c, W) for c in cuts] + [W]
    return list(zip(edges, edges[1:]))


def expect_range(rec, W, begin, end):
    """(entry, exit, first row, rows) of the records that start in [begin, end)."""
    S = rec.start
    i0, i1 = (int(x) for x in np.searchsorted(S, [begin, end]))
    entry = int(S[i0]) if i0 < len(S) else W
    ex = int(S[i1]) if i1 < len(S) else W
    return entry, ex, i0, i1 - i0


CTX_FLAGS = {"default": 0, "run": F_NO_BAIL}  # NXG_F64R_FLAGS of the contexts the R cases name


def class_census(every=1):
    """How many W cases, and how many ranges of the R cases (every `every`-th cut list), reach
    each class on the device, as counted by tile_plan(): {family group: {class: n}}. A W case
    is decoded on the context that never hands over (its tiles' classes) and on the one that
    does (bail, not f64); a range on its case's context only, so a range that the probe hands
    over counts as a bail and its tiles' classes do not count."""
    out = {"W": dict.fromkeys(CLASSES + ("bail", "not_f64"), 0),
           "R": dict.fromkeys(CLASSES + ("bail", "not_f64"), 0)}
    for c in CASES:
        w = pristine(c) if c.corrupt else wire(c.name)
        verdict = tile_plan(w, flags=0)
        out["W"]["bail"] += verdict.bails
        out["W"]["not_f64"] += verdict.not_f64
        if c.heartbeat is None:
            for cls in {t.cls for t in tile_plan(w, flags=F_NO_BAIL).tiles}:
                out["W"][cls] += 1
    for c in RCASES:
        w = rwire(c.name)
        for cut in c.cuts[::every]:
            for b, e in ranges_of(len(w), cut):
                if b == e:
                    continue
                p = tile_plan(w, b, e, 0 if c.heartbeat is not None else CTX_FLAGS[c.ctx])
                out["R"]["bail"] += p.bails
                out["R"]["not_f64"] += p.not_f64
                if not p.bails and not p.not_f64:
                    for cls in {t.cls for t in p.tiles}:
                        out["R"][cls] += 1
    return out
