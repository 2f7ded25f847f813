#!/usr/bin/env python3
"""Hand-built zstd frames for every branch of the decompressor's frame-format code
(netidx_amd/csrc/nxg_zstd.hip: frame_decode, block_compressed), written to
tests/golden/zstd_valid.json.

The committed libzstd fixtures (make_zstd.py) hold the decompressor to whatever libzstd emits for
one data generator. This writer builds frames from explicit blocks instead -- literals, a list of
(literals length, match length, offset value) sequences, the literals type and size format, the
table modes and distributions -- so every header form, table mode, repeat-offset case and match
geometry is reached on purpose. It has
  * an FSE sequence encoder derived from the decode table (the cells of one symbol partition the
    state space, so encoding backwards the cell for a symbol is the one whose [base, base + 2^nbits)
    holds the next state),
  * a Huffman encoder from chosen code lengths (direct 4-bit weights),
  * a formatted dictionary writer (magic, id, tree, OF, ML, LL descriptions, offsets, content).
The intended content of a frame is computed by expand() below straight from the block list. Each
frame is then decoded by libzstd (ctypes) and by the model (tests/zstd_model.py); nothing is
written unless both give the intended bytes, and the model's tags say what the frame reached.
Malformed frames carry the one check of nxg_zstd.hip that rejects them and libzstd's verdict.

Sizes named below come from the kernel's constants: RING 16384 (LDS ring of the latest output),
DRAIN RING/4 = 4096, LSTAGE 1024 (literal stage), kBlockMax 131072, 64 lanes per copy round,
kLLLog 9 / kMLLog 9 / kOFLog 8, kHufMaxBits 12.

Usage: python tests/golden/make_zstd_valid.py   (needs libzstd.so.1)
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import zstd_enc_cases as zc  # noqa: E402
import zstd_model as zm  # noqa: E402

OUT = os.path.join(HERE, "zstd_valid.json")
INLINE_MAX = 4096  # plains above are stored as length + sha256


# ---- bit writers -------------------------------------------------------------------------------
def pack_backward(items):
    """(value, nbits) in the order the decoder reads them -> the backward bitstream's bytes."""
    v = pos = 0
    for val, n in reversed(items):
        assert 0 <= val < (1 << n) or n == 0 and val == 0
        v |= val << pos
        pos += n
    v |= 1 << pos  # the final marker bit
    return v.to_bytes(pos // 8 + 1, "little")


def code_of(bases, bits, v):
    c = max(i for i, b in enumerate(bases) if b <= v)
    assert v - bases[c] < (1 << bits[c])
    return c, v - bases[c], bits[c]


def fse_states(cells, syms):
    """The decode-table state for each symbol, chosen backwards."""
    by = {}
    for u, (s, nb, base) in enumerate(cells):
        by.setdefault(s, []).append((u, nb, base))
    st = [0] * len(syms)
    st[-1] = by[syms[-1]][0][0]
    for i in range(len(syms) - 2, -1, -1):
        nxt = st[i + 1]
        (st[i],) = [u for u, nb, base in by[syms[i]] if base <= nxt < base + (1 << nb)]
    return st


def make_norm(counts, log):
    """{symbol: count or -1} -> the normalized counts list; the first symbol of the largest count
    takes what is left of 2^log."""
    top = max(counts)
    norm = [0] * (top + 1)
    for s, c in counts.items():
        norm[s] = c
    rest = (1 << log) - sum(abs(c) for c in norm)
    big = max(counts, key=lambda s: (counts[s], -s))
    assert rest >= 0 and norm[big] > 0
    norm[big] += rest
    return norm


# ---- Huffman -----------------------------------------------------------------------------------
def code_lengths(n, maxlen=None):
    """n Kraft-complete code lengths: a chain down to `maxlen` first (when given), then the
    shallowest leaf split until there are n."""
    leaves = [0]
    if maxlen:
        while max(leaves) < maxlen:
            d = max(leaves)
            leaves.remove(d)
            leaves += [d + 1, d + 1]
    while len(leaves) < n:
        d = min(leaves)
        leaves.remove(d)
        leaves += [d + 1, d + 1]
    assert len(leaves) == n
    return sorted(leaves)


def huf_tree(lengths_by_symbol):
    """{symbol: code length} -> (direct-weights description bytes, {symbol: (code, nbits)})."""
    mb = max(lengths_by_symbol.values())
    top = max(lengths_by_symbol)
    w = [0] * top  # the last symbol's weight is implied
    for s, n in lengths_by_symbol.items():
        if s != top:
            w[s] = mb + 1 - n
    assert 1 <= len(w) <= 128
    cells, mb2, full = zm.huf_from_weights(w)
    assert mb2 == mb and full[top] == mb + 1 - lengths_by_symbol[top]
    desc = bytearray([127 + len(w)])
    for i in range(0, len(w), 2):
        desc.append((w[i] << 4) | (w[i + 1] if i + 1 < len(w) else 0))
    codes = {}
    for u, (s, n) in enumerate(cells):
        if s not in codes:
            codes[s] = (u >> (mb - n), n)
    return bytes(desc), codes


def huf_stream(codes, data):
    return pack_backward([codes[b] for b in data])


# ---- blocks ------------------------------------------------------------------------------------
class Ctx:
    """What a frame's later blocks may reuse: the last Huffman codes and FSE tables."""

    def __init__(self, huf=None, fse=None):
        self.huf = huf
        self.fse = dict(fse or {})


def literals_section(ctx, lits, kind, sf, tree=None):
    """kind raw | rle | huf | treeless; sf the Size_Format; tree {symbol: length} for huf."""
    rs = len(lits)
    if kind in ("raw", "rle"):
        lt = 0 if kind == "raw" else 1
        if sf in (0, 2):
            assert rs < 32
            h = bytes([lt | (sf << 2) | (rs << 3)])
        elif sf == 1:
            assert rs < 4096
            h = (lt | (1 << 2) | (rs << 4)).to_bytes(2, "little")
        else:
            assert rs < (1 << 20)
            h = (lt | (3 << 2) | (rs << 4)).to_bytes(3, "little")
        if kind == "rle":
            assert lits == lits[:1] * rs and rs
            return h + lits[:1]
        return h + lits
    body = b""
    if kind == "huf":
        desc, ctx.huf = huf_tree(tree)
        body = desc
    codes = ctx.huf
    if sf == 0:
        body += huf_stream(codes, lits)
    else:
        seg = (rs + 3) // 4
        parts = [huf_stream(codes, lits[k * seg:(k + 1) * seg]) for k in range(4)]
        body += b"".join(len(q).to_bytes(2, "little") for q in parts[:3]) + b"".join(parts)
    lhs, nb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    cs = len(body)
    assert rs < (1 << nb) and cs < (1 << nb), (rs, cs, nb)
    lt = 2 if kind == "huf" else 3
    return (lt | (sf << 2) | (rs << 4) | (cs << (4 + nb))).to_bytes(lhs, "little") + body


def sequences_section(ctx, seqs, modes, extra_items=(), drop=0):
    """seqs [(ll, ml, offset value)]; modes {name: 'pre' | 'rle' | ('desc', norm, log) | 'rep'}."""
    n = len(seqs)
    if n == 0:
        return b"\x00"
    if n < 128:
        out = bytes([n])
    elif n < 0x7F00:
        out = bytes([128 + (n >> 8), n & 255])
    else:
        out = bytes([255]) + (n - 0x7F00).to_bytes(2, "little")
    coded = {"ll": [code_of(zm.LL_BASE, zm.LL_BITS, s[0]) for s in seqs],
             "ml": [code_of(zm.ML_BASE, zm.ML_BITS, s[1]) for s in seqs],
             "of": [(s[2].bit_length() - 1, s[2] - (1 << (s[2].bit_length() - 1)),
                     s[2].bit_length() - 1) for s in seqs]}
    mbits, desc = 0, b""
    for name, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        m = modes.get(name, "pre")
        mx, mlog, dflt, dlog = zm.TABLES[name]
        if m == "pre":
            ctx.fse[name] = (zm.build_fse(dflt, dlog), dlog)
        elif m == "rle":
            (sym,) = {c[0] for c in coded[name]}
            ctx.fse[name] = ([(sym, 0, 0)], 0)
            desc += bytes([sym])
            mbits |= 1 << shift
        elif m == "rep":
            mbits |= 3 << shift
        else:
            _, norm, log = m
            assert log <= mlog and len(norm) <= mx + 1
            d = zm.write_ncount(norm, log)
            back, blog, used = zm.read_ncount(d, mx)
            assert back == norm and blog == log and used == len(d)
            ctx.fse[name] = (zm.build_fse(norm, log), log)
            desc += d
            mbits |= 2 << shift
    out += bytes([mbits]) + desc
    st = {k: fse_states(ctx.fse[k][0], [c[0] for c in coded[k]]) for k in ("ll", "of", "ml")}
    items = [(st[k][0], ctx.fse[k][1]) for k in ("ll", "of", "ml")]
    for i in range(n):
        for k in ("of", "ml", "ll"):
            items.append((coded[k][i][1], coded[k][i][2]))
        if i + 1 < n:
            for k in ("ll", "ml", "of"):
                _, nb, base = ctx.fse[k][0][st[k][i]]
                items.append((st[k][i + 1] - base, nb))
    items += list(extra_items)
    if drop:  # (malformed frames: a stream that ends before its last `drop` fields)
        items = items[:-drop]
    return out + pack_backward(items)


def cblock(lits, seqs, kind="raw", sf=None, tree=None, modes=None, extra_items=(), drop=0):
    if sf is None:
        n = len(lits)
        sf = (0 if n < 32 else 1 if n < 4096 else 3) if kind in ("raw", "rle") else \
            (1 if n < 1024 else 2 if n < 16384 else 3)
    return {"t": "c", "lits": bytes(lits), "seqs": list(seqs), "kind": kind, "sf": sf,
            "tree": tree, "modes": modes or {}, "extra": extra_items, "drop": drop}


def raw(data):
    return {"t": "raw", "data": bytes(data)}


def rle(byte, size):
    return {"t": "rle", "byte": byte, "size": size}


def build_frame(blocks, ctx=None, did=(0, 0), fcs_len=None, single=True, checksum=False,
                window_log=20, content=None, last_type=None):
    """blocks -> the frame's bytes. did (bytes, id); fcs_len None: the smallest field."""
    ctx = ctx or Ctx()
    body = b""
    for i, b in enumerate(blocks):
        last = 1 if i + 1 == len(blocks) else 0
        if b["t"] == "raw":
            typ, size, data = 0, len(b["data"]), b["data"]
        elif b["t"] == "rle":
            typ, size, data = 1, b["size"], bytes([b["byte"]])
        else:
            data = literals_section(ctx, b["lits"], b["kind"], b["sf"], b["tree"]) + \
                sequences_section(ctx, b["seqs"], b["modes"], b["extra"], b["drop"])
            typ, size = 2, len(data)
            assert size <= zm.BLOCK_MAX
        if last and last_type is not None:
            typ = last_type
        body += ((size << 3) | (typ << 1) | last).to_bytes(3, "little") + data
    n = len(content)
    if fcs_len is None:
        fcs_len = 1 if n < 256 else 2 if n < 65536 + 256 else 4
    if not single and fcs_len == 1:
        fcs_len = 2 if n >= 256 else 4
    dl, dv = did
    fhd = ({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_len] << 6) | ((1 if single else 0) << 5) | \
        ((1 if checksum else 0) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[dl]
    h = zm.MAGIC.to_bytes(4, "little") + bytes([fhd])
    if not single:
        h += bytes([(window_log - 10) << 3])
    h += dv.to_bytes(dl, "little")
    if fcs_len:
        h += (n - 256 if fcs_len == 2 else n).to_bytes(fcs_len, "little")
    f = h + body
    if checksum:
        f += (zm.xxh64(content) & 0xFFFFFFFF).to_bytes(4, "little")
    return f


def expand(blocks, hist=b"", rep=(1, 4, 8)):
    """The content the block list means: a direct reading of each (ll, ml, offset value)."""
    out = bytearray()
    rep = list(rep)
    for b in blocks:
        if b["t"] == "raw":
            out += b["data"]
        elif b["t"] == "rle":
            out += bytes([b["byte"]]) * b["size"]
        else:
            lp = 0
            for ll, ml, ofv in b["seqs"]:
                out += b["lits"][lp:lp + ll]
                lp += ll
                if ofv > 3:
                    rep = [ofv - 3, rep[0], rep[1]]
                else:
                    k = ofv - 1 + (ll == 0)
                    if k == 1:
                        rep = [rep[1], rep[0], rep[2]]
                    elif k == 2:
                        rep = [rep[2], rep[0], rep[1]]
                    elif k == 3:
                        rep = [rep[0] - 1, rep[0], rep[1]]
                for _ in range(ml):
                    q = len(out) - rep[0]
                    out.append(out[q] if q >= 0 else hist[len(hist) + q])
            out += b["lits"][lp:]
    return bytes(out)


def dictionary(did, tree, norms, rep, content):
    """A formatted dictionary (RFC 8878 5). norms {name: (norm, log)}."""
    desc, codes = huf_tree(tree)
    d = zm.DICT_MAGIC.to_bytes(4, "little") + did.to_bytes(4, "little") + desc
    fse = {}
    for name in ("of", "ml", "ll"):
        norm, log = norms[name]
        d += zm.write_ncount(norm, log)
        fse[name] = (zm.build_fse(norm, log), log)
    d += b"".join(r.to_bytes(4, "little") for r in rep) + content
    return d, Ctx(codes, fse)


# ---- the cases ---------------------------------------------------------------------------------
def rbytes(seed, n, symbols):
    r = random.Random(seed)
    return bytes(r.choice(symbols) for _ in range(n))


SYM16 = list(range(0x61, 0x71))
TREE16 = {s: 4 for s in SYM16}
TREE2 = {0x30: 1, 0x31: 1}


def dicts():
    """name -> (bytes, writer context or None). Two formatted dictionaries of about 300 bytes
    (1- and 2-byte ids) and a raw-content one."""
    content = rbytes(11, 300, SYM16)
    tree = {s: n for s, n in zip(SYM16, code_lengths(16, 7))}
    norms = {"of": (make_norm({0: 2, 1: 2, 2: 4, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4, 8: 2, 9: 2}, 5), 5),
             "ml": (make_norm({0: 8, 1: 4, 2: 4, 3: 4, 5: 4, 13: 2, 30: -1, 36: 2}, 6), 6),
             "ll": (make_norm({0: 8, 1: 4, 2: 4, 3: 4, 4: 4, 5: 4, 8: 4, 16: -1, 20: 2}, 6), 6)}
    out = {}
    for name, did in (("fmt1", 0x5A), ("fmt2", 0x1234)):
        d, ctx = dictionary(did, tree, norms, (7, 33, 120), content)
        out[name] = (d, ctx, did)
    out["raw"] = (rbytes(12, 500, SYM16), None, 0)
    return out


def valid_cases(D):
    """[(name, dict name or None, blocks, frame options)]"""
    C = []

    def add(name, blocks, dname=None, **kw):
        C.append((name, dname, blocks, kw))

    mid = lambda n: [(n // 2, 5, 4 + 3)] if n >= 8 else [(n - 1, 5, 2 + 3)]  # noqa: E731
    # literal header sizes at their edges (raw / RLE: 5, 12, 20 bits of size)
    for n in (31, 32, 4095, 4096):
        add("lit_raw_%d" % n, [cblock(rbytes(n, n, SYM16), mid(n))])
        add("lit_rle_%d" % n, [cblock(b"\x77" * n, [(n // 2, 7, 1)], kind="rle")])
    add("lit_rle_sf2", [cblock(b"\x55" * 9, [(4, 4, 1)], kind="rle", sf=2)])
    # Huffman literals: one stream with a fresh tree; four streams at every rs % 4, at the ends of
    # the 10-, 14- and 18-bit size formats (compressed sizes stay within: 4-bit codes)
    add("lit_huf1_fresh", [cblock(rbytes(1, 200, SYM16), mid(200), kind="huf", sf=0, tree=TREE16)])
    for n in (6, 7, 8, 9, 1023, 1024, 16383, 16384):
        syms, tree = (SYM16, TREE16) if n < 16383 else (SYM16[:4], {s: 2 for s in SYM16[:4]})
        add("lit_huf4_%d" % n, [cblock(rbytes(n, n, syms), mid(n), kind="huf", tree=tree)])
    # trees: 2 symbols; 128 symbols as direct weights (127 listed) and the longest direct
    # description (128 listed); code length 11, and 12 (kHufMaxBits; libzstd's verdict decides)
    add("huf_2sym", [cblock(rbytes(2, 100, [0, 1]), mid(100), kind="huf", sf=0,
                            tree={0: 1, 1: 1})])
    t128 = {s: n for s, n in zip(range(128), code_lengths(128))}
    add("huf_direct_128", [cblock(rbytes(3, 600, list(range(128))), mid(600), kind="huf",
                                  tree=t128)])
    t129 = {s: n for s, n in zip(range(129), code_lengths(129, 9))}
    add("huf_direct_129", [cblock(rbytes(4, 600, list(range(129))), mid(600), kind="huf",
                                  tree=t129)])
    for mbits in (11, 12):
        t = {s: n for s, n in zip(range(40, 60), code_lengths(20, mbits))}
        data = bytes(range(40, 60)) * 3 + rbytes(5, 300, list(range(40, 60)))
        add("huf_maxbits%d" % mbits, [cblock(data, mid(len(data)), kind="huf", tree=t)])
    # sequence counts at the ends of the 1-, 2- and 3-byte forms. 0x7EFF and 0x7F00: RLE literals
    # and all three tables in RLE mode (ll 1, ml 3, offset value 1), so the stream is its marker
    lit = rbytes(6, 300, SYM16)
    add("nseq_1", [cblock(lit[:20], [(10, 4, 6)])])
    for n in (127, 128):
        add("nseq_%d" % n, [cblock(lit, [(2, 3 + i % 5, 4 + i % 7) for i in range(n)])])
    allrle = {"ll": "rle", "of": "rle", "ml": "rle"}
    for n in (0x7EFF, 0x7F00):
        add("nseq_0x%X" % n, [cblock(b"\x42" * n, [(1, 3, 1)] * n, kind="rle", modes=allrle)])
    # RLE mode for each table on its own
    for k in ("ll", "of", "ml"):
        seqs = [(3 if k == "ll" else 13 if i == 0 else 1 + i % 4, 6 if k == "ml" else 3 + i % 9,
                 (8 + 3) if k == "of" else 5 + i % 30) for i in range(40)]
        add("seq_rle_%s" % k, [cblock(rbytes(7, 200, SYM16), seqs, modes={k: "rle"})])
    # described tables: accuracy 5; the largest (kLLLog 9, kMLLog 9, kOFLog 8) with low-probability
    # symbols and zero runs above 3 (gaps in the used codes)
    seqs = [(2, 3, 4)] + [(i % 3, 3 + i % 3, 4 + i % 4) for i in range(30)]
    d5 = {"ll": ("desc", make_norm({0: 8, 1: 8, 2: 8}, 5), 5),
          "of": ("desc", make_norm({2: 16, 1: 8}, 5), 5),
          "ml": ("desc", make_norm({0: 8, 1: 8, 2: 8}, 5), 5)}
    add("desc_log5", [cblock(rbytes(8, 100, SYM16), seqs, modes=d5)])
    seqs = [(40, 200, 4)] + [((0, 1, 9, 18, 40)[i % 5], (3, 4, 20, 55, 150)[i % 5],
                              (4, 5, 259, 9, 70)[i % 5]) for i in range(50)]
    big = {"ll": ("desc", make_norm({0: 200, 1: 100, 9: 50, 17: -1, 23: 3, 35: -1}, 9), 9),
           "of": ("desc", make_norm({2: 100, 3: 20, 6: -1, 8: 40, 20: -1}, 8), 8),
           "ml": ("desc", make_norm({0: 150, 1: 100, 17: 60, 38: -1, 43: 7, 52: -1}, 9), 9)}
    add("desc_max_logs", [cblock(rbytes(9, 800, SYM16), seqs, modes=big)])
    # repeat offsets: every (offset value 1, 2, 3) x (ll 0, > 0), chained so that a wrong rotation
    # changes which bytes later matches copy; distinct starting offsets 5, 11, 23
    chain = [(30, 4, 5 + 3), (3, 4, 11 + 3), (3, 4, 23 + 3)]
    for i, (ofv, ll) in enumerate([(1, 2), (2, 2), (3, 2), (1, 0), (2, 0), (3, 0), (2, 1), (1, 0),
                                   (3, 3), (3, 0), (1, 1), (2, 0), (2, 0), (3, 0), (1, 5)]):
        chain.append((ll, 4 + i % 3, ofv))
    add("rep_chain", [cblock(rbytes(10, 120, SYM16), chain)])
    for dn in ("fmt1", "fmt2"):
        # straight from the dictionary's three offsets (7, 33, 120), then the same chain
        add("rep_chain_" + dn, [cblock(rbytes(10, 120, SYM16), [(0, 5, 1), (2, 5, 3), (0, 6, 2)]
                                       + chain[3:], kind="treeless", sf=0,
                                       modes={"ll": "rep", "of": "rep", "ml": "rep"})], dn)
    # matches from the dictionary's content: wholly inside, running into the output with a period
    # of at least 64 lanes and below
    for dn in ("raw", "fmt1"):
        n = len(D[dn][0]) if dn == "raw" else 300
        add("match_dict_inside_" + dn, [cblock(lit[:40], [(10, 50, n + 10 + 3), (5, 20, 200 + 3)])],
            dn)
        add("match_dict_cross64_" + dn, [cblock(lit[:40], [(10, 300, 100 + 10 + 3), (5, 9, 7)])],
            dn)
        add("match_dict_cross_short_" + dn, [cblock(lit[:40], [(10, 200, 30 + 10 + 3),
                                                               (0, 150, 5 + 3)])], dn)
        add("match_dict_whole_" + dn, [cblock(lit[:9], [(0, n, n + 3), (9, 3, 2 * n + 9 + 3)])], dn)
    # short and lane-count offsets (64 lanes per copy round) x lengths around one and three rounds
    for off in (1, 2, 3, 63, 64, 65):
        seqs = [(70 if i == 0 else 7, ml, off + 3) for i, ml in enumerate((3, 64, 65, 200))]
        add("match_off%d" % off, [cblock(rbytes(off, 100, SYM16), seqs)])
    # distances around RING (16384) with a copy longer than DRAIN (4096), so a drain falls inside
    # the copy: 24 KiB of two-symbol literals (1 bit each), then the match
    # twice (the second time through repeat offset 1)
    for dist in (16383, 16384, 16385, 20480):
        n = dist + 300
        far = rbytes(13, n, [0x30, 0x31])
        add("match_dist%d" % dist, [cblock(far + b"01", [(n, 5000, dist + 3), (1, 4097, 1)],
                                           kind="huf", tree=TREE2)])
    # the largest codes: ml 52 with extra bits, ll 35 (a literal run past 65536: 69 refills of the
    # 1 KiB stage), an offset code of 20 (a match from more than 1 MiB back, through global memory)
    add("ml_code52", [cblock(rbytes(14, 50, SYM16), [(40, 65539 + 1234, 37 + 3)])])
    long_lits = rbytes(15, 65536 + 5000, [0x30, 0x31])
    add("ll_code35", [cblock(long_lits, [(65536 + 4990, 10, 999 + 3)], kind="huf", tree=TREE2)])
    add("of_code20", [rle(0x41 + i, 131072) for i in range(9)] +
        [cblock(lit[:30], [(10, 300, (1 << 20) + 70000 + 3), (5, 5000, 2 * 131072 - 50 + 3)])],
        single=False, window_log=21, fcs_len=4)
    # literal runs against the 1 KiB stage (LSTAGE): ending at 1023, 1024, 1025; starting 64
    # before the edge (961)
    sl = rbytes(16, 2300, SYM16)
    for end in (1023, 1024, 1025):
        add("lit_run_end%d" % end, [cblock(sl, [(end, 4, 9), (100, 4, 77 + 3), (1000, 5, 8)],
                                           kind="huf", tree=TREE16)])
    add("lit_run_start961", [cblock(sl, [(961, 4, 9), (100, 4, 77 + 3), (63, 3, 5), (64, 3, 6),
                                         (1024, 5, 8)], kind="huf", tree=TREE16)])
    # blocks: one regenerating exactly kBlockMax; four blocks (fresh tables; treeless + repeat;
    # RLE; predefined then repeat of predefined); no sequences after sequences; empty raw and RLE
    add("block_131072", [cblock(rbytes(17, 1000, SYM16), [(900, 65036, 777 + 3),
                                                          (50, 65036, 4000 + 3)])])
    fresh = {"ll": ("desc", make_norm({0: 8, 1: 8, 2: 8, 5: 4}, 5), 5),
             "of": ("desc", make_norm({2: 16, 3: 8, 4: 4}, 5), 5),
             "ml": ("desc", make_norm({0: 8, 1: 8, 4: 8}, 5), 5)}
    rep3 = {"ll": "rep", "of": "rep", "ml": "rep"}
    s4 = [((2, 1, 0, 5)[i % 4], (3, 4, 7)[i % 3], (4, 5, 9, 17)[i % 4]) for i in range(20)]
    add("four_blocks", [cblock(rbytes(18, 90, SYM16), s4, kind="huf", sf=0, tree=TREE16,
                               modes=fresh),
                        cblock(rbytes(19, 70, SYM16), s4[3:], kind="treeless", sf=1, modes=rep3),
                        rle(0x2E, 100),
                        cblock(rbytes(20, 60, SYM16), s4[:9]),
                        cblock(rbytes(21, 60, SYM16), s4[2:], kind="treeless", sf=0, modes=rep3)],
        checksum=True)
    add("treeless1_after_rle_modes", [cblock(rbytes(22, 50, SYM16), [(5, 4, 7)] * 4, kind="huf",
                                             tree=TREE16, modes=allrle),
                                      cblock(rbytes(23, 50, SYM16), [(5, 4, 7)] * 6,
                                             kind="treeless", sf=0, modes=rep3),
                                      cblock(rbytes(24, 50, SYM16), [(5, 4, 7)] * 3,
                                             kind="treeless", sf=1, modes=rep3)])
    add("nseq0_after_seq", [cblock(lit[:50], [(10, 30, 7)]), cblock(lit[50:90], []),
                            cblock(lit[90:130], [(0, 9, 2), (3, 9, 100 + 3)])])
    add("empty_raw_rle", [cblock(lit[:50], [(10, 30, 7)]), raw(b""), rle(0x99, 0), raw(b"tail")],
        checksum=True)
    # frame headers: a window descriptor and no content size; content size 255 (1 byte) and 256
    # (2 bytes, the +256 form), 4 and 8 bytes; 1- and 2-byte dictionary ids are the fmt frames
    add("hdr_window_nofcs", [cblock(lit[:60], [(20, 30, 7)]), raw(b"xyz")], single=False,
        fcs_len=0)
    add("hdr_fcs255", [raw(rbytes(25, 255, SYM16))])
    add("hdr_fcs256", [raw(rbytes(26, 256, SYM16))])
    add("hdr_fcs4", [cblock(lit[:60], [(20, 30, 7)])], fcs_len=4)
    add("hdr_fcs8", [cblock(lit[:60], [(20, 30, 7)])], fcs_len=8)
    return C


def malformed_cases(D):
    """[(name, dict name, frame bytes, record length, check)] -- `check` is the one test of
    nxg_zstd.hip that refuses the frame, read to precede any use of the bad field."""
    lit = rbytes(6, 300, SYM16)
    M = []

    def add(name, blocks, check, dname=None, cap=None, content=None, **kw):
        # the writer needs tables to encode with where the frame claims earlier ones
        ctx = Ctx(huf_tree(TREE16)[1], {k: (zm.build_fse(v[2], v[3]), v[3])
                                        for k, v in zm.TABLES.items()})
        if dname and D[dname][1]:
            ctx = Ctx(D[dname][1].huf, D[dname][1].fse)
        content = content if content is not None else b"\0" * 64
        did = (0, 0) if not dname or not D[dname][2] else (1 if D[dname][2] < 256 else 2,
                                                           D[dname][2])
        f = build_frame(blocks, ctx, did=did, single=False, fcs_len=0, content=content, **kw)
        M.append((name, dname, f, cap if cap is not None else 4096, check))

    hip = "netidx_amd/csrc/nxg_zstd.hip:"
    past = hip + "526 `off == 0 || off > f.op + hist` before emit_match"
    add("offset_past_history", [cblock(lit[:40], [(10, 5, 11 + 3)])], past)
    add("offset_past_history_dict", [cblock(lit[:40], [(10, 5, 500 + 11 + 3)])], past, "raw")
    add("literals_overrun", [cblock(lit[:20], [(10, 4, 5), (11, 4, 5)])],
        hip + "523 `l.pos + ll > l.total` before emit_lits")
    add("leftover_sequence_bits", [cblock(lit[:20], [(10, 4, 5)], extra_items=[(0, 8)])],
        hip + "532 `b.bp != 0` after the last sequence")
    # the stream ends 8 fields early, inside the third of five sequences: the rest reads as zeros
    add("sequence_bits_overrun", [cblock(lit[:40], [(3, 4, 5), (2, 5, 6), (9, 3, 7), (1, 4, 5),
                                                    (1, 4, 4)], drop=8)],
        hip + "532 `b.bp != 0` after the last sequence")
    add("repeat_mode_first_block", [cblock(lit[:20], [(10, 4, 5)],
                                           modes={"ll": "pre", "of": "rep", "ml": "pre"})],
        hip + "241 `!ok` in seq_table mode 3")
    add("treeless_first_block", [cblock(lit[:20], [(10, 4, 5)], kind="treeless", sf=0)],
        hip + "415 `!f.huf_ok`")
    add("reserved_block_type", [raw(b"abcdef")], hip + "605 `return Z_CORRUPT;  // reserved block type`", last_type=3)
    add("rep0_minus_1_is_zero", [raw(b"0123456789"), cblock(lit[:20], [(0, 4, 3)])],
        hip + "526 `off == 0` before emit_match")
    add("block_131073", [cblock(rbytes(17, 1000, SYM16), [(900, 65037, 777 + 3),
                                                          (50, 65036, 4000 + 3)])],
        hip + "602 `f.op - o0 > kBlockMax` after the block (its writes held to the slot by 524)", cap=131073 + 64)
    good = [cblock(lit[:60], [(20, 30, 7)]), raw(b"xyz")]
    n = len(expand(good))
    add("output_one_over", good, hip + "588 `f.op + bs > f.cap` before the raw block's copy",
        cap=n - 1)
    return M


def libzstd_cases(z):
    """libzstd-made frames for what the writer has no encoder for: a Huffman tree of all 256
    symbols, FSE-coded. Skewed bytes, so the literals compress."""
    import ctypes as C
    r = random.Random(27)
    data = bytes(range(256)) + bytes(min(255, int(r.expovariate(0.03))) for _ in range(1500))
    Z = z.z
    Z.ZSTD_compressBound.restype = C.c_size_t
    Z.ZSTD_compress.restype = C.c_size_t
    Z.ZSTD_compress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    out = C.create_string_buffer(4096)
    n = Z.ZSTD_compress(out, 4096, data, len(data), 19)
    assert not Z.ZSTD_isError(n)
    return [("libzstd_huf_fse_256", None, out.raw[:n], data, "huf:fse:nsym>=255")]


def build_cases(z):
    """The JSON document. z: zstd_enc_cases.Libzstd."""
    D = dicts()
    models = {k: zm.Dict(v[0]) for k, v in D.items()}
    doc = {"libzstd": int(z.z.ZSTD_versionNumber()),
           "dicts": {k: v[0].hex() for k, v in D.items()}, "valid": [], "malformed": []}

    def verify(name, dname, f, want):
        dz = D[dname][0] if dname else None
        got = z.decompress(f, len(want), dz)
        out, tags = zm.decode(f, models[dname] if dname else None, len(want))
        return got, out, tags

    def entry(name, dname, f, want, tags):
        e = {"name": name, "dict": dname, "frame": f.hex(), "plain_len": len(want),
             "tags": sorted(tags)}
        if len(want) <= INLINE_MAX:
            e["plain"] = want.hex()
        else:
            e["sha256"] = hashlib.sha256(want).hexdigest()
        return e

    for name, dname, blocks, kw in valid_cases(D):
        hist = models[dname].content if dname else b""
        rep = models[dname].rep if dname else (1, 4, 8)
        want = expand(blocks, hist, rep)
        ctx = None
        did = (0, 0)
        if dname and D[dname][1]:
            ctx = Ctx(D[dname][1].huf, D[dname][1].fse)
            did = (1 if D[dname][2] < 256 else 2, D[dname][2])
        f = build_frame(blocks, ctx, did=did, content=want, **kw)
        got, out, tags = verify(name, dname, f, want)
        if name == "huf_maxbits12":
            # follow libzstd on 12-bit codes
            doc["huf_maxbits12_libzstd"] = "accepted" if got == want else "rejected"
            if got is None:  # then neither the model (HUF_MAX_BITS) nor the kernel should take it
                continue
        assert got == want, (name, "libzstd", None if got is None else len(got))
        assert out == want, (name, "model", out if not isinstance(out, bytes) else len(out))
        doc["valid"].append(entry(name, dname, f, want, tags))
    for name, dname, f, want, tag in libzstd_cases(z):
        got, out, tags = verify(name, dname, f, want)
        assert got == want and out == want and tag in tags, name
        doc["valid"].append(entry(name, dname, f, want, tags))
    for name, dname, f, cap, check in malformed_cases(D):
        # (Libzstd.decompress offers one byte more than asked: the case about the record's own
        # length gives libzstd exactly that length)
        got = z.decompress(f, cap - 1 if name == "output_one_over" else cap,
                           D[dname][0] if dname else None)
        out, _ = zm.decode(f, models[dname] if dname else None, cap)
        assert isinstance(out, zm.ZstdError), (name, "the model accepts it")
        e = {"name": name, "dict": dname, "frame": f.hex(), "rec_len": cap, "check": check,
             "model": str(out), "libzstd": "rejected" if got is None else "accepted"}
        if got is not None:
            e["libzstd_plain"] = got.hex() if len(got) <= INLINE_MAX else None
            e["libzstd_sha256"] = hashlib.sha256(got).hexdigest()
        doc["malformed"].append(e)
    return doc


def dumps(doc):
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


def main():
    z = zc.Libzstd.load()
    if z is None:
        raise SystemExit("libzstd.so.1 is needed to check the frames")
    doc = build_cases(z)
    s = dumps(doc)
    assert len(s) < 200 * 1024, len(s)
    open(OUT, "w").write(s)
    print("%d valid, %d malformed, %d bytes" % (len(doc["valid"]), len(doc["malformed"]), len(s)))
    for e in doc["malformed"]:
        print(" ", e["name"], "libzstd:", e["libzstd"], "| model:", e["model"])


if __name__ == "__main__":
    main()
