"""Inputs and format readers shared by the zstd compressor's tests (tests/test_gpu_zstd_compress.py,
tests/test_zstd_gpu_golden_cpu.py) and the generator of its golden pin (tests/golden/make_zstd_gpu.py):
the fixture payloads as uncompressed archive records, the crafted payloads whose compressed size has a
derivable bound, the fixture dictionary's Huffman code lengths (decoded with the independent Python
restatement in tests/golden/make_zstd_crafted.py), a frame header reader (RFC 8878 3.1.1.1) and
libzstd through ctypes where it loads."""
import ctypes as C
import importlib.util
import json
import os
import random

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 128 * 1024


def _mzc():
    spec = importlib.util.spec_from_file_location("mzc", os.path.join(G, "make_zstd_crafted.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def load_fixtures():
    """(manifest entries, fixture records, plain bytes, dictionary)"""
    m = json.load(open(os.path.join(G, "zstd_manifest.json")))["records"]
    rec = open(os.path.join(G, "zstd_records.bin"), "rb").read()
    plain = open(os.path.join(G, "zstd_plain.bin"), "rb").read()
    d = open(os.path.join(G, "zstd_dict.bin"), "rb").read()
    return m, rec, plain, d


def fixture_record(e, rec, plain):
    """The uncompressed archive record of fixture entry e (after its RecordHeader): the index
    bytes of the fixture's compressed record, then the plain batch. Returns (index, batch)."""
    idx = rec[e["rec_off"] + 4:e["rec_off"] + 4 + e["index_len"]]
    return idx, plain[e["plain_off"]:e["plain_off"] + e["plain_len"]]


def worst_case(index_len, batch_len):
    """The issue's per-record bound."""
    return 4 + index_len + 17 + batch_len + 3 * max(1, -(-batch_len // BLOCK))


def dict_parts(d):
    """(dictionary id, code length per byte value (0: no code), content) of a zstd-format
    dictionary (RFC 8878 5): magic, id, Huffman tree, three FSE tables, three offsets, content."""
    mzc = _mzc()
    assert d[:4] == bytes.fromhex("37a430ec")
    did = int.from_bytes(d[4:8], "little")
    hb = d[8]
    assert hb < 128  # FSE-compressed weights
    norm, log, used = mzc.read_ncount(d[9:9 + hb], 15)
    cells = mzc.build_fse(norm, log)
    w = mzc.fse_weights(d[9 + used:9 + hb], cells, log, 255)
    total = sum(1 << (x - 1) for x in w if x)
    mb = total.bit_length()
    rest = (1 << mb) - total
    assert rest & (rest - 1) == 0
    w.append(rest.bit_length())
    nbits = [(mb + 1 - x) if x else 0 for x in w] + [0] * (256 - len(w))
    p = 9 + hb
    for max_sym in (31, 52, 35):  # offsets, match lengths, literals lengths
        _, _, u = mzc.read_ncount(d[p:p + 16 + 2 * max_sym], max_sym)
        p += u
    p += 12
    return did, nbits, d[p:]


def no_repeat_payload(symbols, length, content, seed):
    """Up to `length` bytes over `symbols` with no 3-byte substring that occurs earlier in the
    payload or anywhere in `content`: no match exists. Greedy; stops early at a dead end."""
    seen = {content[i:i + 3] for i in range(len(content) - 2)}
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < length:
        order = list(symbols)
        rng.shuffle(order)
        for s in order:
            if len(out) < 2:
                out.append(s)
                break
            t = bytes(out[-2:]) + bytes([s])
            if t not in seen:
                seen.add(t)
                out.append(s)
                break
        else:
            break
    return bytes(out)


def crafted(d):
    """name -> payload: the payloads of the issue's items 3 and 4."""
    _, nbits, content = dict_parts(d)
    rng = random.Random(8878)
    pat = bytes(rng.getrandbits(8) for _ in range(64))
    s6 = [s for s in range(256) if 0 < nbits[s] <= 6]
    s7 = [s for s in range(256) if 0 < nbits[s] <= 7]
    return {
        "dict_slice": content[1000:1000 + 4096],
        "pattern64": pat * 512,
        "one_byte": b"\x2a" * 4096,
        "random70000": bytes(rng.getrandbits(8) for _ in range(70000)),
        "huf1": no_repeat_payload(s6, 150, content, 1),
        "huf4": no_repeat_payload(s7, 2000, content, 2),
        # a match that starts in the dictionary's last bytes and runs on into the record itself
        "dict_cross": content[-100:] + content[-100:-50] + bytes(rng.getrandbits(8) for _ in range(20)),
        # a match longer than its offset
        "period2": b"ab" * 3000 + bytes(rng.getrandbits(8) for _ in range(9)),
    }


def frame_header(f):
    """Fields of a frame header: dict(single, checksum, did_flag, did, fcs_flag, fcs, size)."""
    assert f[:4] == bytes.fromhex("28b52ffd")
    fhd = f[4]
    h = {"single": (fhd >> 5) & 1, "checksum": (fhd >> 2) & 1, "did_flag": fhd & 3,
         "fcs_flag": fhd >> 6, "reserved": (fhd >> 3) & 1}
    p = 5 + (0 if h["single"] else 1)
    dl = (0, 1, 2, 4)[h["did_flag"]]
    h["did"] = int.from_bytes(f[p:p + dl], "little")
    p += dl
    fl = (1 if h["single"] else 0, 2, 4, 8)[h["fcs_flag"]]
    h["fcs"] = int.from_bytes(f[p:p + fl], "little") + (256 if fl == 2 else 0) if fl else None
    h["size"] = p + fl
    return h


def check_frame_header(f, batch_len, did):
    """The header nxg_archive_compress promises: Single_Segment with the content size in the
    smallest field, no checksum, `did` (0: none) in its smallest field."""
    h = frame_header(f)
    assert h["single"] == 1 and h["checksum"] == 0 and h["reserved"] == 0
    assert h["fcs"] == batch_len
    assert h["fcs_flag"] == (batch_len >= 256) + (batch_len >= 65536 + 256)
    assert h["did_flag"] == (did > 0) + (did >= 256) + (did >= 65536) and h["did"] == did
    return h


def blocks(f):
    """[(type, last, size, body offset)] of a frame's blocks."""
    p = frame_header(f)["size"]
    out = []
    while True:
        bh = int.from_bytes(f[p:p + 3], "little")
        last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
        out.append((typ, last, size, p + 3))
        p += 3 + (1 if typ == 1 else size)
        if last:
            break
    assert p == len(f)
    return out


class Libzstd:
    """libzstd's one-shot decompression through ctypes (None from load() when it is absent)."""

    def __init__(self, z):
        self.z = z
        z.ZSTD_isError.argtypes = [C.c_size_t]
        z.ZSTD_createDCtx.restype = C.c_void_p
        z.ZSTD_freeDCtx.argtypes = [C.c_void_p]
        z.ZSTD_createDDict.restype = C.c_void_p
        z.ZSTD_createDDict.argtypes = [C.c_char_p, C.c_size_t]
        z.ZSTD_freeDDict.argtypes = [C.c_void_p]
        z.ZSTD_decompress_usingDDict.restype = C.c_size_t
        z.ZSTD_decompress_usingDDict.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                                 C.c_size_t, C.c_void_p]
        z.ZSTD_decompressDCtx.restype = C.c_size_t
        z.ZSTD_decompressDCtx.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                          C.c_size_t]
        self.dctx = z.ZSTD_createDCtx()
        self.ddicts = {}

    @staticmethod
    def load():
        try:
            return Libzstd(C.CDLL("libzstd.so.1"))
        except OSError:
            return None

    def decompress(self, frame, size, d=None):
        """The frame's content (`size` bytes expected), or None when libzstd refuses it."""
        frame = bytes(frame)
        out = C.create_string_buffer(size + 1)
        if d is not None:
            if d not in self.ddicts:
                self.ddicts[d] = self.z.ZSTD_createDDict(d, len(d))
            r = self.z.ZSTD_decompress_usingDDict(self.dctx, out, size + 1, frame, len(frame),
                                                  self.ddicts[d])
        else:
            r = self.z.ZSTD_decompressDCtx(self.dctx, out, size + 1, frame, len(frame))
        if self.z.ZSTD_isError(r):
            return None
        return out.raw[:r]
