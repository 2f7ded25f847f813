"""GPU zstd compression with block trees (nxg_archive_compress_opts, literals = 1: a block may
build a Huffman tree from its own literals and describe it; nxg_zstd_enc.hip).

As in tests/test_gpu_zstd_compress.py the frames are checked by what they are: they come back
through nxg_archive_decompress, tests/zstd_model.py and libzstd; the model's tags show that the
one- and four-stream forms, both header sizes, both description forms, the length limit and a tree
carried from one block to the next are all reached; sizes are held to what the candidates' order
implies and to a bound derived from a flat code; a wave's state does not leak from one record to
the next; literals = 0 is nxg_archive_compress byte for byte; and today's bytes equal the pin
tests/golden/zstd_gpu_tree_records.bin (tests/golden/make_zstd_gpu_trees.py), which
tests/test_zstd_gpu_trees_golden_cpu.py decodes on the CPU."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import zstd_enc_cases as zc
import zstd_model as zm
import zstd_tree_cases as tc

pytestmark = pytest.mark.gpu
G = zc.G
MODEL_MAX = zc.BLOCK  # fixtures above one block go through the model with their own dictionary only


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
def dicts(codec, fx):
    """name -> (dictionary bytes or None, handle or None)"""
    out = {}
    for name, dd in tc.dictionaries(fx[3]):
        out[name] = (dd, codec.zstd_dict(dd) if dd is not None else None)
    yield out
    for dd, h in out.values():
        if h is not None:
            h.close()


@pytest.fixture(scope="module")
def crafted(fx):
    return tc.tree_records(fx[3])


def compress(codec, zdict, records, indexed=False, literals=tc.BLOCK_TREES):
    """records: [(index bytes, batch bytes)] -> [compressed record bytes], raw results"""
    src, offs, o = [], [], 0
    for idx, b in records:
        r = bytes(idx) + bytes(b)
        src.append(r)
        offs.append((o, len(r)))
        o += len(r)
    out, res = codec.archive_compress(np.frombuffer(b"".join(src) + b"\0", np.uint8), offs,
                                      indexed, zdict, literals)
    return [bytes(out[oo:oo + ol]) for oo, ol, _ in res], res


def the_records(fx, crafted):
    """[(name, indexed, index bytes, batch)]: every fixture, every crafted record, two of the
    crafted ones behind an index as well"""
    ents, rec, plain, d = fx
    out = []
    for k, e in enumerate(ents):
        idx, b = zc.fixture_record(e, rec, plain)
        out.append(("fixture%d:%s" % (k, e["kind"]), e["indexed"], idx, b))
    for name, b in crafted.items():
        out.append((name, False, b"", b))
    for name in ("low64", "two_blocks_reuse"):
        out.append((name + ":indexed", True, b"\x05abcd", crafted[name]))
    return out


@pytest.fixture(scope="module")
def outputs(codec, fx, crafted, dicts):
    """(dictionary name, literals) -> [(name, indexed, index, batch, compressed record)]: every
    record compressed with each dictionary in both modes, four calls per dictionary"""
    recs = the_records(fx, crafted)
    out = {}
    for dname, (dd, h) in dicts.items():
        for literals in (0, 1):
            got = {}
            for indexed in (False, True):
                part = [r for r in recs if r[1] == indexed]
                comp, res = compress(codec, h, [(r[2], r[3]) for r in part], indexed, literals)
                for r, c, (oo, ol, er) in zip(part, comp, res):
                    assert er == 0, r[0]
                    assert ol <= zc.worst_case(len(r[2]), len(r[3])), r[0]
                    got[r[0]] = r + (c,)
            out[dname, literals] = [got[r[0]] for r in recs]
    return out


@pytest.mark.parametrize("dname", ["dict", "raw-content", "none"])
def test_round_trip(codec, fx, dicts, outputs, dname):
    dd, h = dicts[dname]
    did = zc.dict_parts(fx[3])[0] if dname == "dict" else 0
    z = zc.Libzstd.load()
    mdict = zm.Dict(dd) if dd is not None else None
    recs = outputs[dname, 1]
    for indexed in (False, True):
        part = [r for r in recs if r[1] == indexed]
        blob, offs, o = [], [], 0
        for name, _, idx, b, cr in part:
            assert int.from_bytes(cr[:4], "big") == len(idx) + len(b), name
            assert cr[4:4 + len(idx)] == idx, name
            zc.check_frame_header(cr[4 + len(idx):], len(b), did)
            blob.append(cr)
            offs.append((o, len(cr)))
            o += len(cr)
        out, res = codec.archive_decompress(np.frombuffer(b"".join(blob), np.uint8), offs, indexed,
                                            h)
        host = out.cpu().numpy()
        for (name, _, idx, b, cr), (oo, ol, er) in zip(part, res):
            assert er == 0 and host[oo:oo + ol].tobytes() == b, name
            f = cr[4 + len(idx):]
            if z is not None:
                assert z.decompress(f, len(b), dd) == b, name
            if len(b) <= MODEL_MAX or not name.startswith("fixture"):
                got, _ = zm.decode(f, mdict, len(b))
                assert got == b, (name, got if isinstance(got, Exception) else "differs")


def test_model_decodes_the_multi_block_fixtures(fx, outputs):
    mdict = zm.Dict(fx[3])
    big = [r for r in outputs["dict", 1] if r[0].startswith("fixture") and len(r[3]) > MODEL_MAX]
    assert len(big) >= 2
    for name, _, idx, b, cr in big:
        got, tags = zm.decode(cr[4 + len(idx):], mdict, len(b))
        assert got == b and "blocks>=2" in tags, name


def test_every_form_is_reached(fx, outputs):
    """The model's tags over the crafted records and the small fixtures."""
    tags = set()
    by = {}
    for dname, dd in tc.dictionaries(fx[3]):
        mdict = zm.Dict(dd) if dd is not None else None
        for name, _, idx, b, cr in outputs[dname, 1]:
            if name.startswith("fixture") and len(b) > 3000:
                continue
            got, t = zm.decode(cr[4 + len(idx):], mdict, len(b))
            assert got == b, name
            tags |= t
            by[dname, name] = t
    assert tags >= {"lit:huf:1stream", "lit:huf4:sf2", "lit:huf4:sf3", "lit:treeless:prev-block",
                    "lit:treeless:dict", "huf:direct", "huf:fse", "huf:maxbits11"}, sorted(tags)
    for dname in ("dict", "raw-content", "none"):
        # 1 and 4 streams; the 4- and the 5-byte header
        assert "lit:huf:1stream" in by[dname, "lits1023"]
        assert "lit:4stream:rs=1024" in by[dname, "lits1024"]
        assert {"lit:4stream:rs=16383", "lit:huf4:sf2"} <= by[dname, "lits16383"]
        assert {"lit:4stream:rs=16384", "lit:huf4:sf3"} <= by[dname, "lits16384"]
        # the second block takes the first block's tree, or must write its own
        f = {r[0]: r[4][4:] for r in outputs[dname, 1]}
        assert tc.first_lit_types(f["two_blocks_reuse"]) == [2, 3], dname
        assert "lit:treeless:prev-block" in by[dname, "two_blocks_reuse"]
        assert tc.first_lit_types(f["two_blocks_new_tree"]) == [2, 2], dname


def test_a_literal_the_dictionary_tree_lacks(codec):
    sd, syms = tc.small_dict_missing_codes()
    lacking = [s for s in range(256) if s not in syms][0]
    rng = random.Random(1)
    a = bytes(rng.choice(syms) for _ in range(300))
    b = a + bytes([lacking]) + bytes(rng.choice(syms) for _ in range(50)) + a  # `a` again: a match
    h = codec.zstd_dict(sd)
    try:
        c0, r0 = compress(codec, h, [(b"", b)], False, 0)
        c1, r1 = compress(codec, h, [(b"", b)], False, 1)
        assert r0[0][2] == 0 and r1[0][2] == 0
        # literals = 0: one literal without a code and the block's literals are raw;
        # literals = 1: the block's own tree
        assert tc.first_lit_types(c0[0][4:]) == [0]
        assert tc.first_lit_types(c1[0][4:]) == [2]
        assert len(c1[0]) < len(c0[0])
        got, tags = zm.decode(c1[0][4:], zm.Dict(sd), len(b))
        assert got == b
        out, res = codec.archive_decompress(np.frombuffer(c1[0], np.uint8), [(0, len(c1[0]))],
                                            False, h)
        oo, ol, er = res[0]
        assert er == 0 and out.cpu().numpy()[oo:oo + ol].tobytes() == b
    finally:
        h.close()


def test_never_larger_than_the_dictionary_tree_mode(outputs):
    """By the candidates' order a block's literals section with block trees is never larger when
    the tree the reader has is the same in both modes: every block of a frame without a
    zstd-format dictionary (there is none in mode 0), the first block with one."""
    gained = 0
    for dname in ("dict", "raw-content", "none"):
        for r0, r1 in zip(outputs[dname, 0], outputs[dname, 1]):
            name, _, idx, b, c0 = r0
            c1 = r1[4]
            if dname != "dict" or len(b) <= zc.BLOCK:
                assert len(c1) <= len(c0), (dname, name, len(c0), len(c1))
                gained += len(c1) < len(c0)
            else:  # the live tree makes the later blocks' choice greedy: reported
                print("%s with the dictionary: %d bytes, %d with block trees"
                      % (name, len(c0), len(c1)))
    assert gained > 60


def test_flat_code_bound(codec, crafted, outputs):
    """3000 bytes drawn uniformly from 0..63, no dictionary: an optimal code is no longer than the
    flat 6-bit one, and the direct description of 64 symbols takes 33 bytes."""
    b = crafted["low64"]
    assert set(b) == set(range(64))
    cr = {r[0]: r[4] for r in outputs["none", 1]}["low64"]
    f = cr[4:]
    bl = zc.blocks(f)
    assert len(bl) == 1 and bl[0][0] == 2
    body = f[bl[0][3]:bl[0][3] + bl[0][2]]
    st = zm._State()
    st.tags, st.huf, st.huf_src = set(), None, None
    lits, section = zm._literals(st, body)  # the model's parse of the section
    n = len(lits)
    assert 2900 <= n <= 3000  # few matches
    seg = (n + 3) // 4
    bound = 5 + 6 + 33 + sum(-(-6 * s // 8) + 1 for s in (seg, seg, seg, n - 3 * seg))
    print("literals section: %d bytes for %d literals, bound %d" % (section, n, bound))
    assert section <= bound, (section, bound)
    assert tc.lit_section(body)[3] == section


def test_a_waves_state_does_not_leak(codec, fx, dicts):
    """More than 4 x CU-count small records, so every wave compresses several: records that write
    their own tree alternate with records that take the dictionary's tree treeless."""
    import torch
    ents, rec, plain, d = fx
    h = dicts["dict"][1]
    treeless = [zc.fixture_record(e, rec, plain) for e in ents
                if e["dict"] and not e["indexed"] and 500 < e["plain_len"] < 3000]
    assert len(treeless) >= 4
    eight = []
    for i in range(4):
        eight += [(b"", tc.uniform(300, 100 + i)), (b"", treeless[i][1])]
    a, _ = compress(codec, h, eight)
    assert [tc.first_lit_types(c[4:]) for c in a] == [[2], [3]] * 4
    n = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 72
    others = [(b"", tc.uniform(200 + 7 * (i % 30), 1000 + i % 50)) if i % 2
              else (b"", treeless[i % 4][1][:400 + i % 100]) for i in range(n)]
    step = n // 8
    mixed = []
    for i in range(8):
        mixed += others[step * i:step * (i + 1)] + [eight[i]]
    b, res = compress(codec, h, mixed)
    assert all(r[2] == 0 for r in res)
    assert [b[(step + 1) * i + step] for i in range(8)] == a
    c, _ = compress(codec, h, eight)
    assert c == a
    # and the crowd comes back
    blob, offs, o = [], [], 0
    for cr in b:
        blob.append(cr)
        offs.append((o, len(cr)))
        o += len(cr)
    out, r2 = codec.archive_decompress(np.frombuffer(b"".join(blob), np.uint8), offs, False, h)
    host = out.cpu().numpy()
    for (idx, p), (oo, ol, er) in zip(mixed, r2):
        assert er == 0 and host[oo:oo + ol].tobytes() == p


def raw_call(codec, h, recs, indexed, opts, out, cap):
    """nxg_archive_compress_opts as C sees it -> (ok, need, error text, the records)"""
    from netidx_amd.codec import lib, NxgArchiveRecord, NetidxError
    src = np.frombuffer(b"".join(i + b for i, b in recs) + b"\0", np.uint8)
    n = len(recs)
    cr = (NxgArchiveRecord * n)()
    o = 0
    for i, (idx, b) in enumerate(recs):
        cr[i].off, cr[i].len = o, len(idx) + len(b)
        o += len(idx) + len(b)
    need, err = C.c_uint64(0), NetidxError()
    ok = lib().nxg_archive_compress_opts(codec.ctx, h.h if h else None, C.c_void_p(src.ctypes.data),
                                         len(src) - 1, cr, n, indexed,
                                         C.byref(opts) if opts is not None else None,
                                         C.c_void_p(out.ctypes.data) if out is not None else None,
                                         cap, C.byref(need), C.byref(err))
    msg = err.msg.decode() if err.msg else ""
    if err.msg:
        lib().nxg_error_free(C.byref(err))
    return ok, need.value, msg, cr


def test_per_record_errors_sizing_and_misuse(codec, fx, dicts):
    from netidx_amd.codec import NxgZstdCompressOpts
    ents, rec, plain, d = fx
    h = dicts["dict"][1]
    ks = [k for k, e in enumerate(ents) if e["indexed"] and e["dict"]][:3]
    recs = [zc.fixture_record(ents[k], rec, plain) for k in ks]
    bad = (b"\x7f", b"\x01\x02\x03")  # an index varint of 127 in a record of 4 bytes
    comp, res = compress(codec, h, [recs[0], bad, recs[1], (b"\x85", b""), recs[2]], True)
    assert [r[2] for r in res] == [0, 7, 0, 7, 0]
    alone, _ = compress(codec, h, recs, True)
    assert [comp[0], comp[2], comp[4]] == alone
    opts = NxgZstdCompressOpts(literals=1)
    ok, need, msg, _ = raw_call(codec, h, recs, True, opts, None, 0)
    assert ok and need == sum(zc.worst_case(len(i), len(b)) for i, b in recs)  # the slots of mode 0
    buf = np.full(need, 0xAB, np.uint8)
    ok, _, msg, _ = raw_call(codec, h, recs, True, opts, buf, need - 1)
    assert not ok and msg and (buf == 0xAB).all()
    ok, _, msg, cr = raw_call(codec, h, recs, True, opts, buf, need)
    assert ok and [bytes(buf[r.out_off:r.out_off + r.out_len]) for r in cr] == alone
    # misuse fails the call by name, before anything is written
    buf[:] = 0xAB
    ok, _, msg, _ = raw_call(codec, h, recs, True, NxgZstdCompressOpts(literals=2), buf, need)
    assert not ok and "literals" in msg and (buf == 0xAB).all()
    bad_opts = NxgZstdCompressOpts(literals=1)
    bad_opts.reserved[1] = 1
    ok, _, msg, _ = raw_call(codec, h, recs, True, bad_opts, buf, need)
    assert not ok and "reserved" in msg and (buf == 0xAB).all()
    ok, _, msg, _ = raw_call(codec, h, recs, True, NxgZstdCompressOpts(literals=2), None, 0)
    assert not ok and "literals" in msg


def test_mode_0_is_nxg_archive_compress(codec, fx, dicts):
    """literals = 0 and opts = NULL through nxg_archive_compress_opts against nxg_archive_compress,
    on the records of the dictionary-tree golden pin, and against the pin itself."""
    from netidx_amd.codec import lib, NxgArchiveRecord, NetidxError, NxgZstdCompressOpts
    ents, rec, plain, d = fx
    m = json.load(open(os.path.join(G, "zstd_gpu_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_records.bin"), "rb").read()
    own = open(os.path.join(G, "zstd_gpu_plain.bin"), "rb").read()
    for dict_used in (True, False):
        for indexed in (True, False):
            part = [e for e in m if e["dict"] == dict_used and e["indexed"] == indexed]
            if not part:
                continue
            recs = []
            for e in part:
                src = plain if e["plain_src"] == "fixture" else own
                recs.append((bytes.fromhex(e["index"]),
                             src[e["plain_off"]:e["plain_off"] + e["plain_len"]]))
            h = dicts["dict"][1] if dict_used else None
            want = [blob[e["rec_off"]:e["rec_off"] + e["rec_len"]] for e in part]
            # nxg_archive_compress itself
            src = np.frombuffer(b"".join(i + b for i, b in recs) + b"\0", np.uint8)
            n = len(recs)
            cr = (NxgArchiveRecord * n)()
            o = 0
            for i, (idx, b) in enumerate(recs):
                cr[i].off, cr[i].len = o, len(idx) + len(b)
                o += len(idx) + len(b)
            need, err = C.c_uint64(0), NetidxError()
            f = lib().nxg_archive_compress
            assert f(codec.ctx, h.h if h else None, C.c_void_p(src.ctypes.data), len(src) - 1, cr,
                     n, indexed, None, 0, C.byref(need), C.byref(err))
            buf = np.zeros(need.value, np.uint8)
            assert f(codec.ctx, h.h if h else None, C.c_void_p(src.ctypes.data), len(src) - 1, cr,
                     n, indexed, C.c_void_p(buf.ctypes.data), need.value, C.byref(need),
                     C.byref(err))
            plain_call = [bytes(buf[r.out_off:r.out_off + r.out_len]) for r in cr]
            assert plain_call == want
            for opts in (None, NxgZstdCompressOpts(literals=0)):
                buf2 = np.zeros(need.value, np.uint8)
                ok, need2, msg, cr2 = raw_call(codec, h, recs, indexed, opts, buf2, need.value)
                assert ok and need2 == need.value, msg
                assert [bytes(buf2[r.out_off:r.out_off + r.out_len]) for r in cr2] == want


def test_golden_pin(codec, fx, crafted, dicts):
    """Today's output equals the committed bytes (tests/golden/make_zstd_gpu_trees.py regenerates
    them after any change to the encoder)."""
    ents, rec, plain, d = fx
    m = json.load(open(os.path.join(G, "zstd_gpu_tree_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_tree_records.bin"), "rb").read()
    assert {e["name"] for e in m} >= {"low64", "skewed", "lits1023", "lits1024", "two_blocks_reuse",
                                       "two_blocks_new_tree", "huf1:dict", "fixture_tree",
                                       "fixture_treeless"}
    for e in m:
        if e["source"] == "fixture":
            idx, b = zc.fixture_record(ents[e["fixture"]], rec, plain)
        else:
            idx, b = b"", crafted[e["source"]]
        assert idx.hex() == e["index"] and hashlib.sha256(b).hexdigest() == e["plain_sha256"]
        comp, res = compress(codec, dicts["dict"][1] if e["dict"] else None, [(idx, b)],
                             e["indexed"])
        assert res[0][2] == 0
        assert comp[0] == blob[e["rec_off"]:e["rec_off"] + e["rec_len"]], e["name"]
