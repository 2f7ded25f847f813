"""GPU zstd compression of archive batch records (nxg_archive_compress, nxg_zstd_enc.hip).

The compressor's bytes are its own (no two encoders agree), so it is checked by what its frames
are: every fixture payload round-trips through this project's decompressor and through libzstd,
the record layout and frame headers are as compress_task writes them, matches and the
dictionary's Huffman tree are really used (size bounds that follow from the format, computed
here), a record's failure is its own, the output is deterministic, and today's output equals the
committed pin (tests/golden/zstd_gpu_records.bin, made by tests/golden/make_zstd_gpu.py), whose
frames libzstd decodes on the CPU in tests/test_zstd_gpu_golden_cpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import zstd_enc_cases as zc

pytestmark = pytest.mark.gpu
G = zc.G


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return zc.load_fixtures()


@pytest.fixture(scope="module")
def zd(codec, fx):
    d = codec.zstd_dict(fx[3])
    yield d
    d.close()


@pytest.fixture(scope="module")
def parts(fx):
    return zc.dict_parts(fx[3])  # (id, code lengths, content)


@pytest.fixture(scope="module")
def crafted(fx):
    return zc.crafted(fx[3])


def compress(codec, zdict, records, indexed=False):
    """records: [(index bytes, batch bytes)] -> [compressed record bytes], raw results"""
    src, offs, o = [], [], 0
    for idx, b in records:
        r = bytes(idx) + bytes(b)
        src.append(r)
        offs.append((o, len(r)))
        o += len(r)
    out, res = codec.archive_compress(np.frombuffer(b"".join(src) + b"\0", np.uint8), offs,
                                      indexed, zdict)
    return [bytes(out[oo:oo + ol]) for oo, ol, _ in res], res


@pytest.fixture(scope="module")
def fixture_out(codec, zd, fx):
    """Every fixture payload compressed once, shared by the tests: entry index -> (index bytes,
    batch, compressed record)."""
    ents, rec, plain, d = fx
    groups = {}
    for k, e in enumerate(ents):
        groups.setdefault((e["dict"], e["indexed"]), []).append(k)
    out = {}
    for (use_dict, indexed), ks in groups.items():
        recs = [zc.fixture_record(ents[k], rec, plain) for k in ks]
        comp, res = compress(codec, zd if use_dict else None, recs, indexed)
        slots = sorted((oo, ol) for oo, ol, _ in res)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(slots, slots[1:]))  # disjoint, in order
        for k, (idx, b), cr, (oo, ol, er) in zip(ks, recs, comp, res):
            assert er == 0, ents[k]["kind"]
            assert ol <= zc.worst_case(len(idx), len(b))
            out[k] = (idx, b, cr)
    assert len(out) == len(ents) == 48
    return out


def test_round_trip_every_fixture(codec, zd, fx, fixture_out, parts):
    ents, rec, plain, d = fx
    did = parts[0]
    sizes = set()
    for indexed in (False, True):
        for use_dict in (False, True):
            ks = [k for k, e in enumerate(ents) if e["indexed"] == indexed and e["dict"] == use_dict]
            if not ks:
                continue
            blob, offs, o = [], [], 0
            for k in ks:
                idx, b, cr = fixture_out[k]
                # u32 BE record_length (the uncompressed record), the index verbatim, the frame
                assert int.from_bytes(cr[:4], "big") == len(idx) + len(b)
                assert cr[4:4 + len(idx)] == idx
                zc.check_frame_header(cr[4 + len(idx):], len(b), did if use_dict else 0)
                if len(b) == 0:  # one empty raw last block
                    f = cr[4 + len(idx):]
                    assert f[zc.frame_header(f)["size"]:] == b"\x01\x00\x00"
                sizes.add(len(b))
                blob.append(cr)
                offs.append((o, len(cr)))
                o += len(cr)
            out, res = codec.archive_decompress(np.frombuffer(b"".join(blob), np.uint8), offs,
                                                indexed, zd if use_dict else None)
            host = out.cpu().numpy()
            for k, (oo, ol, er) in zip(ks, res):
                assert er == 0, ents[k]["kind"]
                assert host[oo:oo + ol].tobytes() == fixture_out[k][1], ents[k]["kind"]
    assert 0 in sizes and min(s for s in sizes if s) < 16 and 207484 in sizes


def test_compressed_batch_decodes_on_the_gpu(codec, zd, fx, fixture_out):
    """One dictionary batch: compressed, decompressed and decoded on the device, against the
    oracle's decode of the plain bytes."""
    import nxo
    import netidx_amd
    from netidx_amd.codec import Columns
    ents = fx[0]
    k = [k for k, e in enumerate(ents) if e["dict"] and e["batch"] and not e["indexed"]
         and e["plain_len"] > 2000][0]
    idx, b, cr = fixture_out[k]
    out, res = codec.archive_decompress(np.frombuffer(cr, np.uint8), [(0, len(cr))], False, zd)
    oo, ol, er = res[0]
    assert er == 0 and ol == len(b)
    cols = Columns(ol + 1, ol + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    st, used = codec.decode_archive(out[oo:oo + ol], ol, cols)
    o, used_o = nxo.decode_archive(np.frombuffer(b, np.uint8))
    o = o.trim()
    assert used == used_o == ol and st.n_rows == len(o["id"])
    g = cols.numpy()
    for key in ("id", "tag", "aux", "ctag", "cfixed", "caux", "fixed"):
        assert np.array_equal(g[key], o[key]), key


def test_libzstd_decodes_every_frame(fx, fixture_out, crafted_out):
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here; tests/test_zstd_gpu_golden_cpu.py pins it")
    ents, _, _, d = fx
    for k, (idx, b, cr) in fixture_out.items():
        got = z.decompress(cr[4 + len(idx):], len(b), d if ents[k]["dict"] else None)
        assert got == b, ents[k]["kind"]
    for name, (b, cr) in crafted_out.items():
        assert z.decompress(cr[4:], len(b), d) == b, name


@pytest.fixture(scope="module")
def crafted_out(codec, zd, crafted):
    """name -> (payload, compressed record), all with the dictionary, one call"""
    names = list(crafted)
    comp, res = compress(codec, zd, [(b"", crafted[n]) for n in names])
    assert all(r[2] == 0 for r in res)
    return {n: (crafted[n], c) for n, c in zip(names, comp)}


def test_matches_are_found_and_coded(codec, zd, crafted_out):
    # (a) 4096 consecutive bytes of the dictionary's content: one or a few sequences
    b, cr = crafted_out["dict_slice"]
    assert len(cr) - 4 <= 512, len(cr) - 4
    # (b) a 64-byte pattern, 512 times
    b, cr = crafted_out["pattern64"]
    assert (len(cr) - 4) * 8 <= len(b), len(cr) - 4
    # (c) one byte, 4096 times
    b, cr = crafted_out["one_byte"]
    assert len(cr) - 4 <= 64, len(cr) - 4
    # (d) random bytes: within the worst case, every block at most raw
    b, cr = crafted_out["random70000"]
    assert len(cr) <= zc.worst_case(0, len(b))
    assert len(cr) - 4 <= len(b) + 17 + 3 * len(zc.blocks(cr[4:]))
    # and they come back
    names = list(crafted_out)
    blob, offs, o = [], [], 0
    for n in names:
        c = crafted_out[n][1]
        blob.append(c)
        offs.append((o, len(c)))
        o += len(c)
    out, res = codec.archive_decompress(np.frombuffer(b"".join(blob), np.uint8), offs, False, zd)
    host = out.cpu().numpy()
    for n, (oo, ol, er) in zip(names, res):
        assert er == 0 and host[oo:oo + ol].tobytes() == crafted_out[n][0], n


def test_raw_content_dictionary(codec, parts):
    """A dictionary without the magic is raw content: history only, no Dictionary_ID in the
    frame, no Huffman tree to reuse; matches still reach into it."""
    content = parts[2]
    raw = codec.zstd_dict(content)
    b = content[5000:9000] + b"tail"
    comp, res = compress(codec, raw, [(b"", b), (b"", b"")])
    assert [r[2] for r in res] == [0, 0]
    f = comp[0][4:]
    zc.check_frame_header(f, len(b), 0)
    assert len(f) <= 512
    body = f[zc.blocks(f)[0][3]:]
    assert body[0] & 3 != 3  # no tree to reuse: the literals are not Huffman-coded
    out, r2 = codec.archive_decompress(np.frombuffer(comp[0], np.uint8), [(0, len(comp[0]))],
                                       False, raw)
    oo, ol, er = r2[0]
    assert er == 0 and out.cpu().numpy()[oo:oo + ol].tobytes() == b
    z = zc.Libzstd.load()
    if z is not None:
        assert z.decompress(f, len(b), content) == b
    raw.close()


def test_the_dictionary_tree_is_used(crafted_out, parts):
    did, nbits, content = parts
    assert [s for s in range(256) if 0 < nbits[s] <= 5] == [0, 6, 9, 255]
    assert [s for s in range(256) if nbits[s] == 6] == [12, 19, 65, 193]
    assert sum(1 for s in range(256) if nbits[s] == 7) == 36 and max(nbits) == 9
    for name, streams in (("huf1", 1), ("huf4", 4)):
        b, cr = crafted_out[name]
        assert len(b) >= (100 if streams == 1 else 1500)  # the greedy builder got far enough
        tri = [b[i:i + 3] for i in range(len(b) - 2)]
        assert len(set(tri)) == len(tri) and not any(t in content for t in tri)  # no match exists
        f = cr[4:]
        bl = zc.blocks(f)
        assert len(bl) == 1 and bl[0][0] == 2  # one compressed block
        body = f[bl[0][3]:bl[0][3] + bl[0][2]]
        assert body[0] & 3 == 3  # Treeless_Literals_Block: the dictionary's tree
        sf = (body[0] >> 2) & 3
        assert (sf == 0) == (streams == 1)
        h = int.from_bytes(body[:5], "little")
        nb = (10, 10, 14, 18)[sf]
        lhs = (3, 3, 4, 5)[sf]
        regen, csize = (h >> 4) & ((1 << nb) - 1), (h >> (4 + nb)) & ((1 << nb) - 1)
        assert regen == len(b)
        assert body[lhs + csize:] == b"\x00"  # no sequences: literals only
        bits = sum(nbits[x] for x in b)
        bound = 17 + 3 + 3 + -(-bits // 8) + 1 + 1
        if streams == 4:
            bound += 6 + 4 + 2
        assert len(f) <= bound, (len(f), bound)


def test_per_record_behaviour(codec, zd, fx):
    from netidx_amd.codec import lib, NxgArchiveRecord, NetidxError
    ents, rec, plain, d = fx
    ks = [k for k, e in enumerate(ents) if e["indexed"] and e["dict"]][:3]
    recs = [zc.fixture_record(ents[k], rec, plain) for k in ks]
    bad = (b"\x7f", b"\x01\x02\x03")  # an index varint of 127 in a record of 4 bytes
    comp, res = compress(codec, zd, [recs[0], bad, recs[1], (b"\x85", b""), recs[2]], True)
    assert [r[2] for r in res] == [0, 7, 0, 7, 0]
    alone, _ = compress(codec, zd, recs, True)
    assert [comp[0], comp[2], comp[4]] == alone
    # out = NULL: the worst case, computed on the host; cap = need - 1 is refused
    src = np.frombuffer(b"".join(i + b for i, b in recs), np.uint8)
    n = len(recs)
    cr = (NxgArchiveRecord * n)()
    o = 0
    for i, (idx, b) in enumerate(recs):
        cr[i].off, cr[i].len = o, len(idx) + len(b)
        o += len(idx) + len(b)
    need, err = C.c_uint64(0), NetidxError()
    assert lib().nxg_archive_compress(codec.ctx, zd.h, C.c_void_p(src.ctypes.data), len(src), cr, n,
                                      True, None, 0, C.byref(need), C.byref(err))
    assert need.value == sum(zc.worst_case(len(i), len(b)) for i, b in recs)
    buf = np.full(need.value, 0xAB, np.uint8)
    ok = lib().nxg_archive_compress(codec.ctx, zd.h, C.c_void_p(src.ctypes.data), len(src), cr, n,
                                    True, C.c_void_p(buf.ctypes.data), need.value - 1,
                                    C.byref(need), C.byref(err))
    assert not ok and err.msg
    lib().nxg_error_free(C.byref(err))
    assert (buf == 0xAB).all()


def test_deterministic_whatever_else_is_in_the_call(codec, zd, fx):
    ents, rec, plain, d = fx
    es = [e for e in ents if e["dict"] and not e["indexed"]]
    eight = [zc.fixture_record(e, rec, plain) for e in es[:16:2]]
    others = [zc.fixture_record(e, rec, plain) for e in es[1:16:2]] * 5
    assert len(eight) == 8 and len(others) == 40
    a, _ = compress(codec, zd, eight)
    mixed = []
    for i in range(8):
        mixed += others[5 * i:5 * i + 5] + [eight[i]]
    b, _ = compress(codec, zd, mixed)
    assert [b[6 * i + 5] for i in range(8)] == a
    c, _ = compress(codec, zd, eight)
    assert c == a


def test_golden_pin(codec, zd, fx, crafted):
    """Today's output equals the committed bytes (tests/golden/make_zstd_gpu.py regenerates them
    after any change to the encoder)."""
    ents, rec, plain, d = fx
    m = json.load(open(os.path.join(G, "zstd_gpu_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_records.bin"), "rb").read()
    own = open(os.path.join(G, "zstd_gpu_plain.bin"), "rb").read()
    assert {e["name"] for e in m} >= {"empty", "tiny", "indexed", "two_blocks", "no_dict", "huf1",
                                       "huf4", "dict_slice", "pattern64", "one_byte"}
    for dict_used in (True, False):
        for indexed in (True, False):
            part = [e for e in m if e["dict"] == dict_used and e["indexed"] == indexed]
            if not part:
                continue
            recs = []
            for e in part:
                src = plain if e["plain_src"] == "fixture" else own
                b = src[e["plain_off"]:e["plain_off"] + e["plain_len"]]
                if e["name"] in crafted:
                    assert b == crafted[e["name"]]
                recs.append((bytes.fromhex(e["index"]), b))
            comp, res = compress(codec, zd if dict_used else None, recs, indexed)
            for e, c in zip(part, comp):
                assert c == blob[e["rec_off"]:e["rec_off"] + e["rec_len"]], e["name"]
