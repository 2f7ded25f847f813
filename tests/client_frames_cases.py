"""Inputs that sit on the branches of the per-client encode (test infrastructure).

nxg_encode_clients runs a tile encoder over a dispatch's entry list: nxg_enc_f64_gather_kernel
(tiles of TPB * NXG_ENC_RPT entries, NXG_ENC_STGB staging bytes per entry) for F64 columns and
nxg_enc_rows_gather_kernel (tiles of TPB * NXG_ENC_GRPT entries, NXG_ENC_BPR staging bytes per
entry) for mixed ones. A tile whose bytes exceed its staging writes straight to the output; a
client's offset is stored by the tile that holds its first entry. `constants()` reads those
numbers FROM THE KERNEL SOURCES and `plan()` restates the choices, so a retune makes
tests/test_client_frames_cpu.py say which case no longer reaches the branch it is named for.

  constants()            T_F64, T_MIXED, STG_F64, STG_MIXED (staging bytes a tile may hold)
  msg_lens(case)         the message length of every entry (scalar and text rows)
  plan(case, layout)     per tile: bytes, staged or direct, the clients that start in it
  cases(layout)          {name: Case} for "f64" or "mixed"
"""
import functools
import os
import re
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "netidx_amd", "csrc")
_INT = r"(\d+)"
_PATTERNS = {
    "nxg_encode_general.hip": {
        "TPB": r"constexpr\s+int\s+TPB\s*=\s*" + _INT + r"\s*;",
        "GRPT": r"#define\s+NXG_ENC_GRPT\s+" + _INT,
        "BPR": r"#define\s+NXG_ENC_BPR\s+" + _INT,
    },
    "nxg_encode_f64.hip": {
        "RPT": r"#define\s+NXG_ENC_RPT\s+" + _INT,
        "STGB": r"#define\s+NXG_ENC_STGB\s+" + _INT,
    },
    "nxg_internal.h": {
        "F64_TPB": r"namespace f64enc \{[^}]*?constexpr\s+int\s+TPB\s*=\s*" + _INT + r"\s*;",
    },
}
# statements plan() restates
_SHAPES = {
    "nxg_encode_general.hip": {
        "tile": r"constexpr int GTILE = TPB \* GRPT;",
        "staging": r"constexpr int GSTG = GTILE \* NXG_ENC_BPR \+ 32;",
        "staged": r"stage = out && c\.n_ctl == 0 && tot <= \(uint64_t\)\(GSTG - 32\);",
    },
    "nxg_encode_f64.hip": {
        "tile": r"constexpr int ETILE = TPB \* ERPT;",
        "staging": r"constexpr int MAXB_ALL = ETILE \* NXG_ENC_STGB \+ 32;",
        "direct": r"phase \+ tbytes > \(uint32_t\)\(MAXB_ALL - 16\)",
    },
    "nxg_internal.h": {},
}


@functools.lru_cache(maxsize=None)
def constants():
    out, missing = {}, []
    for fname, pats in _PATTERNS.items():
        with open(os.path.join(CSRC, fname)) as f:
            src = f.read()
        for name, pat in pats.items():
            m = re.search(pat, src, flags=re.S)
            if m is None:
                missing.append(f"{fname}: {name} (/{pat}/)")
            else:
                out[name] = int(m.group(1))
        for name, pat in _SHAPES[fname].items():
            if re.search(pat, src) is None:
                missing.append(f"{fname}: the {name} statement (/{pat}/)")
    if missing:
        raise RuntimeError("tests/client_frames_cases.py restates these from the kernel sources "
                           "and no longer finds them; re-read plan() against the kernels:\n  " +
                           "\n  ".join(missing))
    out["T_MIXED"] = out["TPB"] * out["GRPT"]
    out["T_F64"] = out["F64_TPB"] * out["RPT"]
    out["STG_MIXED"] = out["T_MIXED"] * out["BPR"]         # tot <= GSTG - 32
    out["STG_F64"] = out["T_F64"] * out["STGB"] + 16       # phase + tbytes <= MAXB_ALL - 16
    return types.MappingProxyType(out)


def tile_size(layout):
    return constants()["T_F64" if layout == "f64" else "T_MIXED"]


class Case:
    """cols: id / tag / fixed / aux (numpy, rows of scalars and text only); heap; the dispatch
    (chan_off, ent_row). f64: every value is an F64, so the case also runs in the F64 layout."""

    def __init__(self, name, cols, heap, chan_off, ent_row, want=None):
        self.name, self.cols, self.heap = name, cols, heap
        self.chan_off = np.asarray(chan_off, np.uint64)
        self.ent_row = np.asarray(ent_row, np.uint64)
        self.f64 = bool(np.all(cols["tag"] == 9))
        self.want = want or {}
        assert self.chan_off[-1] == len(self.ent_row)

    @property
    def n_clients(self):
        return len(self.chan_off) - 1


def _vl(v):
    v = np.asarray(v, np.uint64)
    n = np.ones(v.shape, np.int64)
    for k in range(1, 10):
        n += (v >= np.uint64(1 << (7 * k))).astype(np.int64)
    return n


def msg_lens(case):
    """Message length of every entry: varint(L) 04 varint(id) Value, L = lw(1 + vl(id) + |Value|),
    for F64 (tag 9) and String / Bytes (12, 13) rows."""
    c = case.cols
    tag, aux = c["tag"].astype(np.int64), c["aux"].astype(np.int64)
    assert np.all((tag == 9) | (tag == 12) | (tag == 13)), "msg_lens knows F64, String and Bytes"
    vlen = np.where(tag == 9, 9, 1 + _vl(aux) + aux)
    body = 1 + _vl(c["id"]) + vlen
    row_len = body + _vl(body + _vl(body))
    return row_len[case.ent_row.astype(np.int64)]


def plan(case, layout):
    """Per tile of the layout's kernel: its bytes, whether it is staged (a tile of the F64 kernel
    at the output phase its base gives it), and the clients whose first entry it holds (the last
    tile: also those that start at the end)."""
    k = constants()
    T = tile_size(layout)
    lens = msg_lens(case)
    E = len(lens)
    ntiles = (E + T - 1) // T
    tiles, base = [], 0
    first = case.chan_off.astype(np.int64)
    for t in range(ntiles):
        b = int(lens[t * T:(t + 1) * T].sum())
        if layout == "f64":
            staged = (base % 16) + b <= k["STG_F64"]
        else:
            staged = b <= k["STG_MIXED"]
        hi = (t + 1) * T if t + 1 < ntiles else E + 1
        cl = np.flatnonzero((first >= t * T) & (first < hi))
        tiles.append(types.SimpleNamespace(bytes=b, base=base, staged=staged, clients=cl))
        base += b
    return types.SimpleNamespace(T=T, E=E, ntiles=ntiles, tiles=tiles, total=base)


def commit_shape(n, n_cl=16, seed=0x5EED0009):
    """bench.py's commit shape at n rows: f64 updates, each Id published once and subscribed by 1
    or 2 of n_cl clients, half the rows UpdateChanged and half of those equal to the current
    value. Returns ids, vals (the f64s' bits), kind, and the table's slot_of_id, off, client, cur."""
    from netidx_amd import synth
    rng = np.random.default_rng(seed)
    ids, vals = synth.f64_columns(n, synth.SEED_F64)
    fan = 1 + (rng.random(n) < 0.5).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(fan)]).astype(np.uint32)
    first = rng.integers(0, n_cl, n)
    second = (first + 1 + rng.integers(0, n_cl - 1, n)) % n_cl
    client = np.empty(int(off[-1]), np.uint32)
    client[off[:-1]] = first
    two = fan == 2
    client[off[:-1][two] + 1] = second[two]
    kind = np.where(np.arange(n) % 2 == 0, 1, 0).astype(np.uint8)
    same = rng.random(n) < 0.5
    cur = np.where(same, vals, vals ^ np.uint64(1)).astype(np.uint64)
    slot_of_id = np.zeros(int(ids.max()) + 1, np.uint32)
    slot_of_id[ids] = np.arange(n, dtype=np.uint32)
    return types.SimpleNamespace(ids=ids, vals=vals, kind=kind, slot_of_id=slot_of_id, off=off,
                                 client=client, cur=cur, n_clients=n_cl)


# ---- the cases ----------------------------------------------------------------------------------
VARINT_IDS = [(1 << (7 * k)) - 1 for k in range(1, 10)] + [1 << (7 * k) for k in range(1, 10)] + \
             [2 ** 64 - 1]
TEXT_LENS = [0, 1, 127, 128, 16383, 16384]
BIG_BYTES = 100_000


def _f64_rows(n, seed, id_bits=20):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 1 << id_bits, n, dtype=np.uint64)
    bits = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    return {"id": ids, "tag": np.full(n, 9, np.uint8), "fixed": bits,
            "aux": np.zeros(n, np.uint32)}


def _split(E, cuts):
    return [0] + sorted(min(c, E) for c in cuts) + [E]


def _text_rows(ids, lens, tag=12, seed=7):
    """Rows of String / Bytes values of the given lengths; the heap holds them back to back."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    heap = rng.integers(97, 123, int(off[-1]) + 1, dtype=np.uint8)  # ASCII: valid UTF-8
    n = len(lens)
    cols = {"id": np.asarray(ids, np.uint64), "tag": np.full(n, tag, np.uint8),
            "fixed": off[:-1].astype(np.uint64), "aux": lens.astype(np.uint32)}
    return cols, heap


def _concat(a, ha, b, hb):
    """Rows a then rows b; b's text offsets move behind a's heap."""
    cols = {k: np.concatenate([a[k], b[k]]) for k in ("id", "tag", "aux")}
    bf = b["fixed"].copy()
    text = np.isin(b["tag"], (12, 13))
    bf[text] += np.uint64(len(ha))
    cols["fixed"] = np.concatenate([a["fixed"], bf])
    return cols, np.concatenate([ha, hb])


@functools.lru_cache(maxsize=None)
def cases(layout):
    T = tile_size(layout)
    none = np.zeros(1, np.uint8)
    out = {}

    def add(c):
        out[c.name] = c

    # entry counts around the tile size; three clients, the middle one empty
    for E in (0, 1, 2, T - 1, T, T + 1, 2 * T + 3):
        cols = _f64_rows(max(E, 1), 100 + E)
        add(Case(f"count_{E}", cols, none, [0, E // 3, E // 3, E], np.arange(E),
                 want={"ntiles": (E + T - 1) // T}))
    E = 2 * T + 3
    # clients that start on the last entry of a tile, on the first of the next, and one further
    add(Case("edges", _f64_rows(E, 1), none, [0, T - 1, T, T + 1, E], np.arange(E),
             want={"first_in_tile": {1: 0, 2: 1, 3: 1}}))
    # runs of three empty clients: at the start, on a tile edge, inside a tile, at the end
    add(Case("empty_runs", _f64_rows(E, 2), none,
             [0, 0, 0, 0, 5, T, T, T, T, T + 7, T + 7, T + 7, T + 7, E, E, E, E], np.arange(E),
             want={"first_in_tile": {0: 0, 3: 0, 5: 1, 8: 1, 9: 1, 12: 1, 13: 2, 16: 2}}))
    add(Case("one_client", _f64_rows(E, 3), none, [0, E], np.arange(E), want={"ntiles": 3}))
    # more clients than entries
    for nc in (1, 2, 1025, 70000):
        rng = np.random.default_rng(nc)
        cuts = np.sort(rng.integers(0, 301, nc - 1)) if nc > 1 else []
        add(Case(f"clients_{nc}", _f64_rows(300, 4), none, _split(300, list(cuts)),
                 np.arange(300), want={"ntiles": 1}))
    # ids of every varint width, over more than one tile
    n = len(VARINT_IDS)
    cols = _f64_rows(n, 5)
    cols["id"] = np.array(VARINT_IDS, np.uint64)
    E = T + 5
    add(Case("varint_ids", cols, none, [0, 7, E], np.arange(E) % n, want={"ntiles": 2}))
    # one row named 3000 times; descending rows; a row named by several clients
    add(Case("one_row_3000", _f64_rows(4, 6), none, [0, 1000, 3000], np.full(3000, 2)))
    add(Case("descending", _f64_rows(T + 9, 8), none, [0, 3, T + 9],
             np.arange(T + 9)[::-1].copy()))
    add(Case("shared_rows", _f64_rows(50, 9), none, [0, 40, 80, 120],
             np.concatenate([np.arange(40), np.arange(10, 50), np.arange(5, 45)])))
    # staging overflow: tile 0 takes the direct path, the tile beside it is staged
    if layout == "f64":
        big, small = _f64_rows(T, 10), _f64_rows(T, 11)
        big["id"] |= np.uint64(1 << 28)  # 16-byte records: more than NXG_ENC_STGB each
        cols = {k: np.concatenate([big[k], small[k]]) for k in big}
        add(Case("overflow", cols, none, [0, T // 2, T + 3, 2 * T], np.arange(2 * T),
                 want={"staged": [False, True]}))
    else:
        a, ha = _text_rows(np.arange(T), np.full(T, 40))
        b = _f64_rows(T, 11)
        cols, heap = _concat(a, ha, b, none)
        add(Case("overflow", cols, heap, [0, T // 2, T + 3, 2 * T], np.arange(2 * T),
                 want={"staged": [False, True]}))
        # long messages: every length-prefix width of a String, and three entries of a 100 KB
        # Bytes value that straddle a tile edge
        a, ha = _text_rows(np.arange(len(TEXT_LENS)) + 200, TEXT_LENS)
        b, hb = _text_rows([9], [BIG_BYTES], tag=13)
        f = _f64_rows(T + 10, 12)
        cols, heap = _concat(a, ha, b, hb)
        cols, heap = _concat(cols, heap, f, none)
        nt = len(TEXT_LENS)
        ent = np.arange(nt + 1, nt + 1 + T + 10)       # the f64 rows
        ent[:nt] = np.arange(nt)                        # the strings first
        ent[T - 1:T + 2] = nt                           # the big value at T - 1, T, T + 1
        add(Case("long_messages", cols, heap, [0, 3, T, T + 10], ent,
                 want={"staged": [False, False]}))
    return types.MappingProxyType(out)
