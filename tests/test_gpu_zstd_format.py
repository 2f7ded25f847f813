"""GPU zstd decompression (nxg_archive_decompress, nxg_zstd.hip) on hand-built frames that reach
every branch of its frame-format code (tests/golden/zstd_valid.json, made and checked against
libzstd by tests/golden/make_zstd_valid.py; tests/test_zstd_model_cpu.py lists what each frame
reaches). The expected bytes are the committed plains; those stored as a hash are regenerated
once with the decoder model (tests/zstd_model.py) and checked against the hash.

  * every valid frame, one call per dictionary: no error, the length and every byte;
  * the malformed frames in one call with two valid ones: each reports an error (where libzstd
    accepts the frame the GPU is the stricter one and errors too -- see each assertion), the valid
    ones are intact and nothing outside any record's slot is written;
  * 8192 small records in shuffled orders, many more than the persistent grid has waves, so every
    wave decodes record after record with its LDS tables, ring and literal buffer reused."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import zstd_model as zm

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xA5


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
    """(document, dictionaries' bytes, name -> plain) -- the plains computed once."""
    doc = json.load(open(os.path.join(G, "zstd_valid.json")))
    dicts = {k: bytes.fromhex(v) for k, v in doc["dicts"].items()}
    md = {k: zm.Dict(v) for k, v in dicts.items()}
    plains = {}
    for e in doc["valid"]:
        if "plain" in e:
            plains[e["name"]] = bytes.fromhex(e["plain"])
        else:
            out, _ = zm.decode(bytes.fromhex(e["frame"]), md.get(e["dict"]), e["plain_len"])
            assert hashlib.sha256(out).hexdigest() == e["sha256"], e["name"]
            plains[e["name"]] = out
        assert len(plains[e["name"]]) == e["plain_len"]
    return doc, dicts, plains


def pack(items):
    """[(record length, frame)] -> (source bytes, [(off, len)]): u32 BE length, then the frame."""
    parts, recs, off = [], [], 0
    for n, f in items:
        r = n.to_bytes(4, "big") + f
        parts.append(r)
        recs.append((off, len(r)))
        off += len(r)
    return np.frombuffer(b"".join(parts), np.uint8), recs


def by_dict(entries):
    groups = {}
    for e in entries:
        groups.setdefault(e["dict"], []).append(e)
    return groups


def test_every_valid_frame(codec, fx):
    doc, dicts, plains = fx
    seen = 0
    for dname, es in by_dict(doc["valid"]).items():
        zd = codec.zstd_dict(dicts[dname]) if dname else None
        src, recs = pack([(e["plain_len"], bytes.fromhex(e["frame"])) for e in es])
        out, res = codec.archive_decompress(src, recs, False, zd)
        host = out.cpu().numpy()
        for e, (oo, ol, er) in zip(es, res):
            want = plains[e["name"]]
            assert er == 0, (e["name"], er)
            assert ol == len(want), (e["name"], ol, len(want))
            got = host[oo:oo + ol].tobytes()
            if got != want:
                k = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError("%s: first wrong byte at %d of %d: got %s, want %s" % (
                    e["name"], k, len(want), got[k:k + 16].hex(), want[k:k + 16].hex()))
            seen += 1
        if zd:
            zd.close()
    assert seen == len(doc["valid"])


def test_malformed_frames_fail_alone(codec, fx):
    """Each malformed record reports an error. libzstd 1.4.8 accepts three of them (bits left over
    after the last sequence, repeat offset 1 minus 1 being zero, a block regenerating 131073
    bytes: `libzstd` in the JSON); RFC 8878 forbids all three and the GPU refuses them, so the
    assertion is an error there too, not libzstd's bytes. The valid records decoded by the same
    call are intact, and no byte outside a record's slot is touched."""
    import torch
    doc, dicts, plains = fx
    valid = {e["name"]: e for e in doc["valid"]}
    for dname, bad in by_dict(doc["malformed"]).items():
        good = [e for e in doc["valid"] if e["dict"] == dname and e["plain_len"] <= 4096][:2]
        assert len(good) == 2
        zd = codec.zstd_dict(dicts[dname]) if dname else None
        items = [(good[0]["plain_len"], bytes.fromhex(good[0]["frame"]))]
        items += [(e["rec_len"], bytes.fromhex(e["frame"])) for e in bad]
        items += [(good[1]["plain_len"], bytes.fromhex(good[1]["frame"]))]
        src, recs = pack(items)
        total = sum(n for n, _ in items)
        out = torch.full((total + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        out, res = codec.archive_decompress(src, recs, False, zd, out=out)
        host = out.cpu().numpy()
        for e, (oo, ol, er) in zip(bad, res[1:-1]):
            assert er != 0, (e["name"], "libzstd: " + e["libzstd"])
            assert ol == 0, e["name"]
        for e, (oo, ol, er) in ((good[0], res[0]), (good[1], res[-1])):
            assert er == 0 and host[oo:oo + ol].tobytes() == plains[e["name"]], e["name"]
        # the slots are contiguous, each its record's length: a failed record may have written
        # inside its own slot only
        off = 0
        for (n, _), (oo, ol, er) in zip(items, res):
            assert oo == off
            off += n
            if er == 0:
                assert ol == n
        assert off == total
        assert (host[total:] == SENTINEL).all()
        assert valid[good[0]["name"]]["plain_len"] == res[0][1]
        if zd:
            zd.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_many_records_per_wave(codec, fx, seed):
    """8192 records over a persistent grid of at most occupancy x CUs waves (about 29 KB of LDS a
    wave: under 6 a CU, 256 CUs): every wave takes several records in turn, in an order the seed
    shuffles, and each record must still equal its own plain -- nothing of the tables, the ring
    or the literal buffer of the record before may show."""
    doc, dicts, plains = fx
    small = [e for e in doc["valid"] if e["plain_len"] <= 4096]
    for dname, es in by_dict(small).items():
        n = 8192 if dname is None else 1024
        rng = random.Random(seed * 1000 + len(es))
        order = [es[i % len(es)] for i in range(n)]
        rng.shuffle(order)
        zd = codec.zstd_dict(dicts[dname]) if dname else None
        src, recs = pack([(e["plain_len"], bytes.fromhex(e["frame"])) for e in order])
        out, res = codec.archive_decompress(src, recs, False, zd)
        host = out.cpu().numpy()
        want = b"".join(plains[e["name"]] for e in order)
        assert all(er == 0 for _, _, er in res), [(e["name"], r[2]) for e, r in zip(order, res)
                                                  if r[2]][:5]
        if host[:len(want)].tobytes() != want:
            for e, (oo, ol, er) in zip(order, res):
                assert host[oo:oo + ol].tobytes() == plains[e["name"]], (e["name"], oo)
        if zd:
            zd.close()
