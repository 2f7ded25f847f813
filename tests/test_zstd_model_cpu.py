"""The zstd decoder model (tests/zstd_model.py) and the hand-built frames it vouches for
(tests/golden/zstd_valid.json, written by tests/golden/make_zstd_valid.py), on the CPU:
  * the model decodes the 58 libzstd-checked frames committed earlier (zstd_records.bin with
    zstd_dict.bin, zstd_gpu_records.bin) to their committed plain bytes, which pins the model;
  * it decodes every hand-built valid frame to its plain bytes (or hash) and refuses every
    malformed one;
  * REQUIRED lists the parts of RFC 8878 the GPU decompressor's tests must reach, and every one
    of them is reached by a committed frame (the census names the frame);
  * libzstd, where it loads, agrees on every case;
  * the generator's case builder reproduces the committed JSON.
tests/test_gpu_zstd_format.py runs the same frames through nxg_zstd.hip."""
import hashlib
import importlib.util
import json
import os
import re

import pytest

import zstd_enc_cases as zc
import zstd_model as zm

G = zc.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = [
    # literals section: every type and header size, the size formats' ends
    "lit:raw:lhs1", "lit:raw:lhs2", "lit:raw:lhs3", "lit:rle:lhs1", "lit:rle:lhs2", "lit:rle:lhs3",
    "lit:raw:rs=31", "lit:raw:rs=32", "lit:raw:rs=4095", "lit:raw:rs=4096",
    "lit:rle:rs=31", "lit:rle:rs=32", "lit:rle:rs=4095", "lit:rle:rs=4096",
    "lit:huf:1stream", "lit:treeless:1stream", "lit:huf4:sf1", "lit:huf4:sf2", "lit:huf4:sf3",
    "lit:treeless4:sf1", "lit:treeless4:sf2", "lit:treeless:dict", "lit:treeless:prev-block",
    "lit:4stream:rs%4=0", "lit:4stream:rs%4=1", "lit:4stream:rs%4=2", "lit:4stream:rs%4=3",
    "lit:4stream:rs=6", "lit:4stream:rs=7", "lit:4stream:rs=8", "lit:4stream:rs=9",
    "lit:4stream:rs=1023", "lit:4stream:rs=1024", "lit:4stream:rs=16383", "lit:4stream:rs=16384",
    "lit:run-end@1023", "lit:run-end@1024", "lit:run-end@1025", "lit:run-start@961",
    # Huffman trees
    "huf:direct", "huf:fse", "huf:nsym=2", "huf:direct:nsym=128", "huf:fse:nsym>=255",
    "huf:maxbits1", "huf:maxbits11",
    # sequence tables: every mode of every table, what a repeat mode repeats, the table sizes
    "seq:ll:predefined", "seq:of:predefined", "seq:ml:predefined",
    "seq:ll:rle", "seq:of:rle", "seq:ml:rle",
    "seq:ll:described", "seq:of:described", "seq:ml:described",
    "seq:ll:repeat", "seq:of:repeat", "seq:ml:repeat",
    "seq:ll:repeat:after-dict", "seq:of:repeat:after-dict", "seq:ml:repeat:after-dict",
    "seq:ll:repeat:after-rle", "seq:of:repeat:after-rle", "seq:ml:repeat:after-rle",
    "seq:ll:repeat:after-predefined", "seq:of:repeat:after-predefined",
    "seq:ml:repeat:after-predefined",
    "seq:ll:repeat:after-described", "seq:of:repeat:after-described",
    "seq:ml:repeat:after-described",
    "seq:ll:log5", "seq:of:log5", "seq:ml:log5", "seq:ll:log9", "seq:ml:log9", "seq:of:log8",
    "fse:lowprob", "fse:zero-run>3",
    "nseq:0", "nseq:form1", "nseq:form2", "nseq:form3",
    "nseq=1", "nseq=127", "nseq=128", "nseq=32511", "nseq=32512",
    # repeat offsets
    "rep:idx0", "rep:idx1", "rep:idx2", "rep:idx3", "rep:ll0", "rep:from-dict",
    "rep:of1:ll>0", "rep:of2:ll>0", "rep:of3:ll>0", "rep:of1:ll0", "rep:of2:ll0", "rep:of3:ll0",
    # matches
    "match:dict", "match:dict-into-output", "match:dict-into-output:period>=64",
    "match:dict-into-output:period<64", "match:period<64:len>64",
    "match:dist=16383:len>4096", "match:dist=16384:len>4096", "match:dist=16385:len>4096",
    "match:dist=20480:len>4096", "match:dist=16384", "match:dist=16385",
] + ["match:off%d:len%d" % (o, n) for o in (1, 2, 3, 63, 64, 65) for n in (3, 64, 65, 200)] + [
    "ll:code35", "ml:code52", "ml:code52:extra", "of:code>=20",
    # blocks and frame headers
    "blk:raw", "blk:rle", "blk:compressed", "blk:raw:size0", "blk:rle:size0", "blk:regen=131072",
    "blk:nseq0:after-seq", "blocks>=2", "blocks>=3",
    "fhd:did0", "fhd:did1", "fhd:did2", "fhd:did4", "fhd:fcs0", "fhd:fcs1", "fhd:fcs2", "fhd:fcs4",
    "fhd:fcs8", "fhd:fcs1=255", "fhd:fcs2=256", "fhd:window", "fhd:no-content-size",
    "fhd:checksum", "fhd:checksum:multiblock",
]


def load_valid():
    return json.load(open(os.path.join(G, "zstd_valid.json")))


def model_dicts(doc):
    raw = {k: bytes.fromhex(v) for k, v in doc["dicts"].items()}
    return raw, {k: zm.Dict(v) for k, v in raw.items()}


def plain_matches(e, out):
    if len(out) != e["plain_len"]:
        return False
    if "plain" in e:
        return out == bytes.fromhex(e["plain"])
    return hashlib.sha256(out).hexdigest() == e["sha256"]


def old_fixture_frames():
    """(name, frame, plain, uses the dictionary) of the libzstd-checked frames committed before."""
    ents, rec, plain, d = zc.load_fixtures()
    out = []
    for e in ents:
        f = rec[e["rec_off"] + 4 + e["index_len"]:e["rec_off"] + e["rec_len"]]
        out.append(("records:" + e["kind"], f,
                    plain[e["plain_off"]:e["plain_off"] + e["plain_len"]], e["dict"]))
    m = json.load(open(os.path.join(G, "zstd_gpu_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_records.bin"), "rb").read()
    own = open(os.path.join(G, "zstd_gpu_plain.bin"), "rb").read()
    for e in m:
        src = plain if e["plain_src"] == "fixture" else own
        cr = blob[e["rec_off"]:e["rec_off"] + e["rec_len"]]
        out.append(("gpu_records:" + e["name"], cr[4 + len(e["index"]) // 2:],
                    src[e["plain_off"]:e["plain_off"] + e["plain_len"]], e["dict"]))
    return out, d


@pytest.fixture(scope="module")
def census():
    """tag -> the first committed frame that reaches it; every frame's decode is checked on the
    way (the old fixtures and the hand-built ones)."""
    where = {}
    frames, d = old_fixture_frames()
    assert len(frames) == 58
    D = zm.Dict(d)
    for name, f, want, use_dict in frames:
        out, tags = zm.decode(f, D if use_dict else None, len(want))
        assert out == want, (name, out if isinstance(out, zm.ZstdError) else len(out))
        for t in tags:
            where.setdefault(t, name)
    doc = load_valid()
    _, md = model_dicts(doc)
    for e in doc["valid"]:
        out, tags = zm.decode(bytes.fromhex(e["frame"]), md.get(e["dict"]), e["plain_len"])
        assert not isinstance(out, zm.ZstdError), (e["name"], str(out))
        assert plain_matches(e, out), e["name"]
        assert sorted(tags) == e["tags"], e["name"]
        for t in tags:
            where.setdefault(t, "valid:" + e["name"])
    return where


def test_model_decodes_every_committed_frame(census):
    assert census


def test_model_refuses_every_malformed_frame():
    doc = load_valid()
    _, md = model_dicts(doc)
    assert len(doc["malformed"]) >= 10
    for e in doc["malformed"]:
        out, _ = zm.decode(bytes.fromhex(e["frame"]), md.get(e["dict"]), e["rec_len"])
        assert isinstance(out, zm.ZstdError), e["name"]
        assert str(out) == e["model"], e["name"]
        # the check it names: file:line `text`, and that text stands on that line
        m = re.match(r"(netidx_amd/csrc/nxg_zstd\.hip):(\d+) `([^`]+)`", e["check"])
        assert m, e["name"]
        line = open(os.path.join(ROOT, m.group(1))).read().split("\n")[int(m.group(2)) - 1]
        assert m.group(3) in line, (e["name"], line)


def test_every_required_tag_is_reached(census):
    missing = [t for t in REQUIRED if t not in census]
    assert not missing, "no committed frame reaches: " + ", ".join(missing)


def test_libzstd_agrees_on_every_case():
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here")
    doc = load_valid()
    raw, _ = model_dicts(doc)
    for e in doc["valid"]:
        got = z.decompress(bytes.fromhex(e["frame"]), e["plain_len"], raw.get(e["dict"]))
        assert got is not None and plain_matches(e, got), e["name"]
    for e in doc["malformed"]:
        cap = e["rec_len"] - 1 if e["name"] == "output_one_over" else e["rec_len"]
        got = z.decompress(bytes.fromhex(e["frame"]), cap, raw.get(e["dict"]))
        assert ("rejected" if got is None else "accepted") == e["libzstd"], e["name"]
        if got is not None:
            assert hashlib.sha256(got).hexdigest() == e["libzstd_sha256"], e["name"]


def test_the_generator_reproduces_the_committed_json():
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here (the generator records its verdicts)")
    spec = importlib.util.spec_from_file_location("mzv", os.path.join(G, "make_zstd_valid.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    text = open(os.path.join(G, "zstd_valid.json")).read()
    assert len(text) < 200 * 1024
    doc = m.build_cases(z)
    doc["libzstd"] = json.loads(text)["libzstd"]  # (the version that wrote it: not a case)
    assert m.dumps(doc) == text
