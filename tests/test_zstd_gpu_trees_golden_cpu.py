"""The golden pin of the GPU zstd compressor with block trees (tests/golden/zstd_gpu_tree_records.bin,
written on the MI355X by tests/golden/make_zstd_gpu_trees.py) checked on the CPU: the independent
decoder tests/zstd_model.py and libzstd turn every committed frame into its plain bytes (which
tests/zstd_tree_cases.py regenerates; the manifest holds their hashes), and the frames hold what
they were picked for. tests/test_gpu_zstd_compress_trees.py asserts the GPU still produces exactly
these bytes. Only the libzstd test skips, where libzstd is absent."""
import hashlib
import json
import os

import pytest

import zstd_enc_cases as zc
import zstd_model as zm
import zstd_tree_cases as tc

G = zc.G


def load():
    ents, rec, plain, d = zc.load_fixtures()
    crafted = tc.tree_records(d)
    m = json.load(open(os.path.join(G, "zstd_gpu_tree_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_tree_records.bin"), "rb").read()
    out = []
    for e in m:
        if e["source"] == "fixture":
            idx, b = zc.fixture_record(ents[e["fixture"]], rec, plain)
        else:
            idx, b = b"", crafted[e["source"]]
        assert idx.hex() == e["index"] and len(b) == e["plain_len"]
        assert hashlib.sha256(b).hexdigest() == e["plain_sha256"], e["name"]
        out.append((e, blob[e["rec_off"]:e["rec_off"] + e["rec_len"]], idx, b))
    return out, d, len(blob)


_loaded = []


def pin():
    if not _loaded:
        _loaded.append(load())
    return _loaded[0]


def test_layout_and_size():
    recs, d, size = pin()
    assert size < os.path.getsize(os.path.join(G, "zstd_gpu_records.bin"))
    assert len(recs) <= 12
    did = zc.dict_parts(d)[0]
    for e, cr, idx, b in recs:
        assert int.from_bytes(cr[:4], "big") == len(idx) + len(b), e["name"]
        assert cr[4:4 + len(idx)] == idx
        assert len(cr) <= zc.worst_case(len(idx), len(b))
        zc.check_frame_header(cr[4 + len(idx):], len(b), did if e["dict"] else 0)


def test_the_model_decodes_every_committed_frame():
    recs, d, _ = pin()
    md = zm.Dict(d)
    by = {}
    for e, cr, idx, b in recs:
        f = cr[4 + len(idx):]
        got, tags = zm.decode(f, md if e["dict"] else None, len(b))
        assert got == b, (e["name"], got if isinstance(got, Exception) else "differs")
        by[e["name"]] = (tags, tc.first_lit_types(f))
    assert {"huf:direct", "lit:huf4:sf2"} <= by["low64"][0]
    assert {"huf:fse", "huf:maxbits11"} <= by["skewed"][0]
    assert "lit:huf:1stream" in by["lits1023"][0] and "lit:4stream:rs=1024" in by["lits1024"][0]
    assert by["two_blocks_reuse"][1] == [2, 3] and by["two_blocks_new_tree"][1] == [2, 2]
    assert "lit:treeless:prev-block" in by["two_blocks_reuse"][0]
    assert by["fixture_tree"][1] == [2] and by["fixture_treeless"][1] == [3]
    assert "lit:treeless:dict" in by["fixture_treeless"][0]


def test_libzstd_decompresses_every_committed_frame():
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here")
    recs, d, _ = pin()
    for e, cr, idx, b in recs:
        assert z.decompress(cr[4 + len(idx):], len(b), d if e["dict"] else None) == b, e["name"]
