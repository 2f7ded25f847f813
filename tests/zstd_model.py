"""A plain-Python zstd frame decoder written from RFC 8878, instrumented: besides the frame's
content it returns the set of feature tags the frame exercised (which literal header, which table
modes, which repeat-offset case, which match geometry ...). The tests hold the GPU decompressor
(netidx_amd/csrc/nxg_zstd.hip) to it on frames built branch by branch
(tests/golden/make_zstd_valid.py), and the tag census (tests/test_zstd_model_cpu.py) records which
committed frame reaches which part of the format.

The FSE table description reader and table builder are those of tests/golden/make_zstd_crafted.py
(imported, not copied). Everything else is restated here from the RFC: frame and block headers
(3.1.1.1, 3.1.1.2), literals (3.1.1.3.1), sequences and repeat offsets (3.1.1.3.2, 3.1.1.5),
Huffman (4.2), dictionaries (5).

decode(frame, dictionary=None, cap=None) -> (bytes, tags) or (ZstdError, tags)
"""
import importlib.util
import os

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mzc():
    spec = importlib.util.spec_from_file_location("mzc", os.path.join(G, "make_zstd_crafted.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mzc = _mzc()
read_ncount, build_fse, write_ncount = mzc.read_ncount, mzc.build_fse, mzc.write_ncount

MAGIC = 0xFD2FB528
DICT_MAGIC = 0xEC30A437
BLOCK_MAX = 128 * 1024

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                             4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1,
              1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
# per table: (largest code, largest accuracy log, predefined distribution, its log)
TABLES = {"ll": (35, 9, LL_DEFAULT, 6), "of": (31, 8, OF_DEFAULT, 5), "ml": (52, 9, ML_DEFAULT, 6)}
# RFC 8878 4.2.1 gives Max_Number_of_Bits 11 for what encoders write; libzstd's reader takes 12
# (HUF_TABLELOG_MAX), and tests/golden/zstd_valid.json records its verdict on such a tree
HUF_MAX_BITS = 12


class ZstdError(Exception):
    """A frame the format forbids; str() names the rule."""


# ---- XXH64, seed 0 (the content checksum is its low 4 bytes) -----------------------------------
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161,
                           9650029242287828579, 2870177450012600261)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(b):
    n, i = len(b), 0
    if n >= 32:
        v = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _round(v[k], int.from_bytes(b[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _round(0, v[k])) * _P1 + _P4) & _M
    else:
        h = _P5
    h = (h + n) & _M
    while i + 8 <= n:
        h ^= _round(0, int.from_bytes(b[i:i + 8], "little"))
        h = (_rotl(h, 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h ^= (int.from_bytes(b[i:i + 4], "little") * _P1) & _M
        h = (_rotl(h, 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h ^= (b[i] * _P5) & _M
        h = (_rotl(h, 11) * _P1) & _M
        i += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    h ^= h >> 32
    return h


# ---- backward bitstream (4.1): one big integer, read from the bit under the final marker -------
class Bits:
    def __init__(self, stream):
        if not stream or stream[-1] == 0:
            raise ZstdError("bitstream: no final marker bit")
        self.v = int.from_bytes(stream, "little")
        self.bp = self.v.bit_length() - 1  # unread bits: [0, bp)

    def read(self, k):
        """k bits; bits below the stream's start read as 0 and leave bp negative."""
        self.bp -= k
        if self.bp >= 0:
            return (self.v >> self.bp) & ((1 << k) - 1)
        return (self.v << -self.bp) & ((1 << k) - 1)


# ---- Huffman (4.2) -----------------------------------------------------------------------------
def huf_from_weights(w):
    """Weights of the listed symbols (the last one implied) -> (decode cells, max bits, weights)."""
    total = sum(1 << (x - 1) for x in w if x)
    if total == 0:
        raise ZstdError("huffman: all weights zero")
    mb = total.bit_length()
    rest = (1 << mb) - total
    if rest & (rest - 1):
        raise ZstdError("huffman: weights do not complete a power of two")
    w = list(w) + [rest.bit_length()]
    if len(w) > 256:
        raise ZstdError("huffman: more than 256 symbols")
    if mb > HUF_MAX_BITS:
        raise ZstdError("huffman: code longer than 12 bits")
    cells = [None] * (1 << mb)
    pos = 0
    for wt in range(1, mb + 1):  # weight 1 = the longest codes, from cell 0, symbols in order
        for s, x in enumerate(w):
            if x == wt:
                n = 1 << (wt - 1)
                cells[pos:pos + n] = [(s, mb + 1 - wt)] * n
                pos += n
    assert pos == 1 << mb
    return cells, mb, w


def read_huf_tree(p, tags):
    """A Huffman tree description at p -> (cells, max bits, bytes used)."""
    if not p:
        raise ZstdError("huffman: no tree description")
    hb = p[0]
    if hb >= 128:
        n = hb - 127
        used = 1 + (n + 1) // 2
        if used > len(p):
            raise ZstdError("huffman: direct weights past the section")
        w = []
        for i in range(n):
            b = p[1 + i // 2]
            w.append(b >> 4 if i % 2 == 0 else b & 15)
        tags.add("huf:direct")
        kind = "direct"
    else:
        used = 1 + hb
        if hb < 2 or used > len(p):
            raise ZstdError("huffman: compressed weights past the section")
        try:
            norm, log, u = read_ncount(bytes(p[1:1 + hb]), 12)
        except (AssertionError, IndexError):
            raise ZstdError("huffman: bad FSE description of the weights")
        if log > 6 or u >= hb:
            raise ZstdError("huffman: weight table accuracy above 6 / no stream")
        stream = bytes(p[1 + u:1 + hb])
        if stream[-1] == 0:
            raise ZstdError("bitstream: no final marker bit")
        w = mzc.fse_weights(stream, build_fse(norm, log), log, 255)
        if len(w) > 255:
            raise ZstdError("huffman: more than 255 listed weights")
        tags.add("huf:fse")
        kind = "fse"
    if any(x > HUF_MAX_BITS for x in w):
        raise ZstdError("huffman: weight above the maximum")
    cells, mb, w = huf_from_weights(w)
    if sum(1 for x in w if x == 1) < 2:
        raise ZstdError("huffman: fewer than two weight-1 symbols")
    tags.add("huf:maxbits%d" % mb)
    nsym = sum(1 for x in w if x)
    if nsym == 2:
        tags.add("huf:nsym=2")
    if len(w) >= 255:
        tags.add("huf:%s:nsym>=255" % kind)
    if kind == "direct" and len(w) == 128:
        tags.add("huf:direct:nsym=128")
    return cells, mb, used


def huf_decode(stream, cells, mb, count):
    b = Bits(stream)
    v, bp, mask = b.v, b.bp, (1 << mb) - 1
    out = bytearray(count)
    for i in range(count):
        idx = (v >> (bp - mb)) & mask if bp >= mb else (v << (mb - bp)) & mask
        s, n = cells[idx]
        out[i] = s
        bp -= n
    if bp != 0:
        raise ZstdError("huffman: stream not consumed exactly")
    return out


# ---- dictionary (5) ----------------------------------------------------------------------------
class Dict:
    def __init__(self, d, tags=None):
        tags = set() if tags is None else tags
        self.id, self.huf, self.fse = 0, None, {}
        self.rep = [1, 4, 8]
        self.formatted = len(d) >= 8 and int.from_bytes(d[:4], "little") == DICT_MAGIC
        if not self.formatted:
            self.content = bytes(d)
            return
        self.id = int.from_bytes(d[4:8], "little")
        cells, mb, used = read_huf_tree(d[8:], tags)
        self.huf = (cells, mb)
        p = 8 + used
        for name in ("of", "ml", "ll"):
            mx, mlog = TABLES[name][:2]
            norm, log, u = read_ncount(bytes(d[p:p + 2 * mx + 16]), mx)
            if log > mlog:
                raise ZstdError("dictionary: table accuracy too large")
            self.fse[name] = (build_fse(norm, log), log)
            p += u
        self.rep = [int.from_bytes(d[p + 4 * k:p + 4 * k + 4], "little") for k in range(3)]
        p += 12
        self.content = bytes(d[p:])
        if any(r == 0 or r > len(self.content) for r in self.rep):
            raise ZstdError("dictionary: repeat offset outside the content")


# ---- the frame ---------------------------------------------------------------------------------
class _State:
    pass


def decode(frame, dictionary=None, cap=None):
    """(content, tags), or (ZstdError, tags) when the frame breaks a rule. `cap`: the most output
    the caller accepts (a record's uncompressed length)."""
    tags = set()
    try:
        return bytes(_decode(bytes(frame), dictionary, cap, tags)), tags
    except ZstdError as e:
        return e, tags


def _decode(f, dictionary, cap, tags):
    if len(f) < 6 or int.from_bytes(f[:4], "little") != MAGIC:
        raise ZstdError("frame: magic")
    fhd = f[4]
    fcs_flag, single, cksum, did_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    if fhd & 8:
        raise ZstdError("frame: reserved bit")
    p = 5
    window = None
    if not single:
        wd = f[p]
        base = 1 << (10 + (wd >> 3))
        window = base + (base >> 3) * (wd & 7)
        p += 1
        tags.add("fhd:window")
    dl = (0, 1, 2, 4)[did_flag]
    fl = (1 if single else 0, 2, 4, 8)[fcs_flag]
    if p + dl + fl > len(f):
        raise ZstdError("frame: header past the input")
    did = int.from_bytes(f[p:p + dl], "little")
    p += dl
    fcs = None
    if fl:
        fcs = int.from_bytes(f[p:p + fl], "little") + (256 if fl == 2 else 0)
        p += fl
    tags.add("fhd:did%d" % dl)
    tags.add("fhd:fcs%d" % fl)
    if fl == 2 and fcs in (256, 511):
        tags.add("fhd:fcs2=%d" % fcs)
    if fl == 1 and fcs == 255:
        tags.add("fhd:fcs1=255")
    if fl == 0:
        tags.add("fhd:no-content-size")
    if cksum:
        tags.add("fhd:checksum")
    d = dictionary if isinstance(dictionary, (Dict, type(None))) else Dict(dictionary)
    if did and (d is None or d.id != did):
        raise ZstdError("frame: dictionary id")
    if fcs is not None and cap is not None and fcs > cap:
        raise ZstdError("output: content size above the capacity")
    st = _State()
    st.tags = tags
    st.cap = cap
    st.hist = d.content if d else b""
    st.out = bytearray()
    st.rep = list(d.rep) if d else [1, 4, 8]
    st.rep_dict = [bool(d and d.formatted)] * 3  # which slots still hold the dictionary's values
    st.huf = d.huf if d else None
    st.huf_src = "dict" if st.huf else None
    st.fse = dict(d.fse) if d else {}
    st.fse_src = {k: "dict" for k in st.fse}
    st.had_seq = False
    nblocks = 0
    while True:
        if p + 3 > len(f):
            raise ZstdError("block: header past the input")
        bh = int.from_bytes(f[p:p + 3], "little")
        p += 3
        last, typ, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        nblocks += 1
        st.first = nblocks == 1
        if typ == 3:
            raise ZstdError("block: reserved type")
        if bs > BLOCK_MAX:
            raise ZstdError("block: size above 128 KiB")
        if typ == 0:
            if p + bs > len(f):
                raise ZstdError("block: raw past the input")
            _room(st, bs)
            st.out += f[p:p + bs]
            p += bs
            tags.add("blk:raw")
            if bs == 0:
                tags.add("blk:raw:size0")
        elif typ == 1:
            if p + 1 > len(f):
                raise ZstdError("block: RLE past the input")
            _room(st, bs)
            st.out += f[p:p + 1] * bs
            p += 1
            tags.add("blk:rle")
            if bs == 0:
                tags.add("blk:rle:size0")
        else:
            if p + bs > len(f):
                raise ZstdError("block: compressed past the input")
            o0 = len(st.out)
            _compressed(st, f[p:p + bs])
            if len(st.out) - o0 > BLOCK_MAX:
                raise ZstdError("block: regenerates more than 128 KiB")
            if len(st.out) - o0 == BLOCK_MAX:
                tags.add("blk:regen=131072")
            p += bs
            tags.add("blk:compressed")
        if last:
            break
    if nblocks >= 2:
        tags.add("blocks>=2")
    if nblocks >= 3:
        tags.add("blocks>=3")
    if cksum:
        if p + 4 > len(f):
            raise ZstdError("frame: checksum past the input")
        if int.from_bytes(f[p:p + 4], "little") != xxh64(st.out) & 0xFFFFFFFF:
            raise ZstdError("frame: checksum mismatch")
        p += 4
        if nblocks >= 2:
            tags.add("fhd:checksum:multiblock")
    if p != len(f):
        raise ZstdError("frame: trailing bytes")
    if fcs is not None and fcs != len(st.out):
        raise ZstdError("frame: content size differs from the output")
    return st.out


def _room(st, n):
    if st.cap is not None and len(st.out) + n > st.cap:
        raise ZstdError("output: above the capacity")


def _literals(st, b):
    """The literals section of block body b -> (literals, section length)."""
    tags = st.tags
    if not b:
        raise ZstdError("literals: empty block")
    lt, sf = b[0] & 3, (b[0] >> 2) & 3
    if lt <= 1:
        lhs = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        if lhs > len(b):
            raise ZstdError("literals: header past the block")
        rs = int.from_bytes(b[:lhs], "little") >> (3 if lhs == 1 else 4)
        if rs > BLOCK_MAX:
            raise ZstdError("literals: above 128 KiB")
        name = "raw" if lt == 0 else "rle"
        tags.add("lit:%s:lhs%d" % (name, lhs))
        if rs in (0, 31, 32, 4095, 4096):
            tags.add("lit:%s:rs=%d" % (name, rs))
        if lt == 0:
            if lhs + rs > len(b):
                raise ZstdError("literals: raw past the block")
            return b[lhs:lhs + rs], lhs + rs
        if lhs + 1 > len(b):
            raise ZstdError("literals: RLE byte past the block")
        return b[lhs:lhs + 1] * rs, lhs + 1
    lhs, nb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    if lhs > len(b):
        raise ZstdError("literals: header past the block")
    h = int.from_bytes(b[:lhs], "little")
    rs = (h >> 4) & ((1 << nb) - 1)
    cs = (h >> (4 + nb)) & ((1 << nb) - 1)
    if rs > BLOCK_MAX or lhs + cs > len(b):
        raise ZstdError("literals: compressed size past the block")
    body = b[lhs:lhs + cs]
    if lt == 2:
        cells, mb, used = read_huf_tree(body, tags)
        st.huf = (cells, mb)
        st.huf_src = "block"
        body = body[used:]
        name = "huf"
    else:
        if st.huf is None:
            raise ZstdError("literals: treeless with no previous tree")
        tags.add("lit:treeless:" + ("dict" if st.huf_src == "dict" else "prev-block"))
        name = "treeless"
    cells, mb = st.huf
    if sf == 0:
        tags.add("lit:%s:1stream" % name)
        lits = huf_decode(body, cells, mb, rs)
    else:
        tags.add("lit:%s4:sf%d" % (name, sf))
        tags.add("lit:4stream:rs%%4=%d" % (rs % 4))
        if rs in (6, 7, 8, 9, 1023, 1024, 16383, 16384):
            tags.add("lit:4stream:rs=%d" % rs)
        if len(body) < 10:
            raise ZstdError("literals: four streams need a jump table and 4 bytes")
        s = [int.from_bytes(body[2 * k:2 * k + 2], "little") for k in range(3)]
        if 6 + sum(s) >= len(body):
            raise ZstdError("literals: jump table past the section")
        seg = (rs + 3) // 4
        if 3 * seg > rs:
            raise ZstdError("literals: too few literals for four streams")
        lits = bytearray()
        q = 6
        for k in range(4):
            n = s[k] if k < 3 else len(body) - q
            lits += huf_decode(body[q:q + n], cells, mb, seg if k < 3 else rs - 3 * seg)
            q += n
    return bytes(lits), lhs + cs


def _seq_table(st, name, mode, b, p):
    tags = st.tags
    mx, mlog, dflt, dlog = TABLES[name]
    if mode == 0:
        st.fse[name] = (build_fse(dflt, dlog), dlog)
        st.fse_src[name] = "predefined"
        tags.add("seq:%s:predefined" % name)
    elif mode == 1:
        if p >= len(b) or b[p] > mx:
            raise ZstdError("sequences: RLE symbol")
        st.fse[name] = ([(b[p], 0, 0)], 0)
        st.fse_src[name] = "rle"
        tags.add("seq:%s:rle" % name)
        p += 1
    elif mode == 2:
        try:
            norm, log, u = read_ncount(bytes(b[p:]), mx)
        except (AssertionError, IndexError):
            raise ZstdError("sequences: bad table description")
        if log > mlog or p + u > len(b) or len(norm) > mx + 1:
            raise ZstdError("sequences: table description out of range")
        st.fse[name] = (build_fse(norm, log), log)
        st.fse_src[name] = "described"
        tags.add("seq:%s:described" % name)
        tags.add("seq:%s:log%d" % (name, log))
        if -1 in norm:
            tags.add("fse:lowprob")
        run = best = 0
        for c in norm:
            run = run + 1 if c == 0 else 0
            best = max(best, run)
        if best >= 5:  # a zero count, then a repeat field of more than 3 further zeros
            tags.add("fse:zero-run>3")
        p += u
    else:
        if name not in st.fse:
            raise ZstdError("sequences: repeat mode with no previous table")
        tags.add("seq:%s:repeat" % name)
        tags.add("seq:%s:repeat:after-%s" % (name, st.fse_src[name]))
    return p


def _compressed(st, b):
    tags = st.tags
    lits, p = _literals(st, b)
    if p >= len(b):
        raise ZstdError("sequences: no section")
    nseq = b[p]
    if nseq == 0:
        if p + 1 != len(b):
            raise ZstdError("sequences: bytes after a zero count")
        _room(st, len(lits))
        st.out += lits
        tags.add("nseq:0")
        if st.had_seq:
            tags.add("blk:nseq0:after-seq")
        return
    if nseq < 128:
        p += 1
        tags.add("nseq:form1")
    elif nseq < 255:
        if p + 2 > len(b):
            raise ZstdError("sequences: count past the block")
        nseq = ((nseq - 128) << 8) + b[p + 1]
        p += 2
        tags.add("nseq:form2")
    else:
        if p + 3 > len(b):
            raise ZstdError("sequences: count past the block")
        nseq = b[p + 1] + (b[p + 2] << 8) + 0x7F00
        p += 3
        tags.add("nseq:form3")
    if nseq in (1, 127, 128, 0x7EFF, 0x7F00):
        tags.add("nseq=%d" % nseq)
    if p >= len(b):
        raise ZstdError("sequences: no modes byte")
    modes = b[p]
    p += 1
    if modes & 3:
        raise ZstdError("sequences: reserved mode bits")
    p = _seq_table(st, "ll", modes >> 6, b, p)
    p = _seq_table(st, "of", (modes >> 4) & 3, b, p)
    p = _seq_table(st, "ml", (modes >> 2) & 3, b, p)
    if p >= len(b):
        raise ZstdError("sequences: no bitstream")
    bits = Bits(b[p:])
    (llt, lll), (oft, ofl), (mlt, mll) = st.fse["ll"], st.fse["of"], st.fse["ml"]
    sll, sof, sml = bits.read(lll), bits.read(ofl), bits.read(mll)
    out, hist, rep = st.out, st.hist, st.rep
    lp = 0
    o0 = len(out)
    st.had_seq = True
    for i in range(nseq):
        llc, lnb, lbase = llt[sll]
        ofc, onb, obase = oft[sof]
        mlc, mnb, mbase = mlt[sml]
        if ofc > 31:
            raise ZstdError("sequences: offset code above 31")
        ofx = bits.read(ofc)
        ofv = (1 << ofc) + ofx
        mlx = bits.read(ML_BITS[mlc])
        ml = ML_BASE[mlc] + mlx
        ll = LL_BASE[llc] + bits.read(LL_BITS[llc])
        if i + 1 < nseq:
            sll = lbase + bits.read(lnb)
            sml = mbase + bits.read(mnb)
            sof = obase + bits.read(onb)
        if bits.bp < 0:
            raise ZstdError("sequences: bitstream overrun")
        if llc == 35:
            tags.add("ll:code35")
        if mlc == 52:
            tags.add("ml:code52")
            if mlx:
                tags.add("ml:code52:extra")
        if ofc >= 20:
            tags.add("of:code>=20")
        if ofv > 3:
            off = ofv - 3
            rep[2], rep[1], rep[0] = rep[1], rep[0], off
            st.rep_dict[2], st.rep_dict[1], st.rep_dict[0] = st.rep_dict[1], st.rep_dict[0], False
        else:
            idx = ofv - 1 + (1 if ll == 0 else 0)
            tags.add("rep:idx%d" % idx)
            tags.add("rep:of%d:%s" % (ofv, "ll0" if ll == 0 else "ll>0"))
            if ll == 0:
                tags.add("rep:ll0")
            if st.rep_dict[0 if idx == 3 else idx]:
                tags.add("rep:from-dict")
            if idx == 0:
                off = rep[0]
            elif idx == 3:
                off = rep[0] - 1
                if off == 0:
                    raise ZstdError("sequences: repeat offset 1 minus 1 is zero")
                rep[2], rep[1], rep[0] = rep[1], rep[0], off
                st.rep_dict[2], st.rep_dict[1], st.rep_dict[0] = (st.rep_dict[1], st.rep_dict[0],
                                                                  False)
            elif idx == 1:
                off = rep[1]
                rep[1], rep[0] = rep[0], off
                st.rep_dict[1], st.rep_dict[0] = st.rep_dict[0], st.rep_dict[1]
            else:
                off = rep[2]
                rep[2], rep[1], rep[0] = rep[1], rep[0], off
                st.rep_dict[2], st.rep_dict[1], st.rep_dict[0] = (st.rep_dict[1], st.rep_dict[0],
                                                                  st.rep_dict[2])
        if lp + ll > len(lits):
            raise ZstdError("sequences: literals overrun")
        _room(st, ll + ml)
        if ll:
            if ll >= 64 and lp % 1024 == 961:
                tags.add("lit:run-start@961")
            out += lits[lp:lp + ll]
            lp += ll
            if lp in (1023, 1024, 1025):
                tags.add("lit:run-end@%d" % lp)
        n = len(out)
        if off > n + len(hist):
            raise ZstdError("sequences: offset past the history")
        _tag_match(tags, off, ml, n)
        if off > n:  # starts in the dictionary's content
            k = off - n
            take = min(k, ml)
            out += hist[len(hist) - k:len(hist) - k + take]
            rem = ml - take
        else:
            rem = ml
        if rem:
            s = len(out) - off
            if off >= rem:
                out += out[s:s + rem]
            else:
                piece = bytes(out[s:])
                out += (piece * (rem // off + 1))[:rem]
    if bits.bp != 0:
        raise ZstdError("sequences: bits left over")
    _room(st, len(lits) - lp)
    out += lits[lp:]


def _tag_match(tags, off, ml, n):
    if off > n:
        if off - n >= ml:
            tags.add("match:dict")
        else:
            tags.add("match:dict-into-output")
            tags.add("match:dict-into-output:period%s64" % (">=" if off >= 64 else "<"))
    if off < 64 and ml > 64:
        tags.add("match:period<64:len>64")
    if off in (16383, 16384, 16385, 20480):
        tags.add("match:dist=%d" % off)
        if ml > 4096:
            tags.add("match:dist=%d:len>4096" % off)
    if off in (1, 2, 3, 63, 64, 65) and ml in (3, 64, 65, 200):
        tags.add("match:off%d:len%d" % (off, ml))
