"""GPU decode of archive batches (nxg_decode_archive_batch, include/nxg_codec.h) against the
oracle (nxo_decode_archive, a restatement of <Vec<BatchItem> as Pack>::decode,
netidx-archive/src/logfile/mod.rs:150-205 and netidx/src/subscriber/mod.rs:154-177) and the
committed fixtures (tests/golden/make_golden.py, an independent twin): every row, every child,
the bytes consumed, and the first error's (kind, offset). Bit-exact.

Items carry no length, so the decoder finds boundaries by walking value tags from guessed
starts; the cases below stress that: long strings and arrays that span many 1 KiB chunks, bytes
that look like items, trailing bytes after the batch, a count larger than the items present."""
import json
import os
import zlib

import numpy as np
import pytest

import guards
import nxo

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
COLS = ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux")


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def gpu_decode(codec, buf, cap_rows=None, cap_children=None, spare=None):
    """spare: the columns carry a band of that many sentinel elements behind each capacity
    (tests/guards.py), checked after the decode."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    buf = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else buf
    n = len(buf)
    d = torch.from_numpy(buf.copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8).cuda()
    caps = (cap_rows if cap_rows is not None else n // 2 + 1,
            cap_children if cap_children is not None else n + 1, 1)
    if spare:
        cols = guards.guarded_columns(*caps, netidx_amd.LAYOUT_MIXED, "cuda", spare)
    else:
        cols = Columns(*caps, netidx_amd.LAYOUT_MIXED, "cuda")
    st, used = codec.decode_archive(d, n, cols, check=False)
    if spare:
        guards.assert_guards(cols)
    return cols, st, used


def assert_matches_oracle(codec, buf, spare=None, **caps):
    cols, st, used = gpu_decode(codec, buf, spare=spare, **caps)
    d, r = nxo.decode_archive(buf, caps.get("cap_rows"), caps.get("cap_children"))
    o = d.trim()
    assert (st.err_kind, st.err_offset) == (o["err_kind"], o["err_offset"])
    assert st.path in (3, 5)  # the exact decoder, the fast path
    if o["err_kind"]:
        return st
    assert used == r and st.n_rows == len(o["id"]) and st.n_children == len(o["ctag"])
    g = cols.numpy()
    for k in COLS:
        assert np.array_equal(g[k], o[k]), k
    return st


@pytest.mark.parametrize("b", MANIFEST["archive"], ids=lambda b: b["name"])
def test_archive_golden(codec, b):
    wire = open(os.path.join(GOLD, b["file"]), "rb").read()
    cols, st, used = gpu_decode(codec, wire)
    assert st.err_kind == 0 and used == b["consumed"]
    g = cols.numpy()
    rows = [list(map(int, r)) for r in zip(g["id"], g["tag"], g["fixed"], g["aux"])]
    assert rows == b["expect"]["rows"]
    ch = [list(map(int, r)) for r in zip(g["ctag"], g["cfixed"], g["caux"])]
    assert ch == b["expect"]["children"]


@pytest.mark.parametrize("c", MANIFEST["archive_errors"], ids=lambda c: c["name"])
def test_archive_golden_errors(codec, c):
    cols, st, used = gpu_decode(codec, bytes.fromhex(c["hex"]))
    assert (st.err_kind, st.err_offset) == (c["kind"], c["offset"])


@pytest.mark.parametrize("c", MANIFEST["archive_edge_ok"], ids=lambda c: c["name"])
def test_archive_golden_edge_ok(codec, c):
    cols, st, used = gpu_decode(codec, bytes.fromhex(c["hex"]))
    assert st.err_kind == 0 and used == c["consumed"]
    g = cols.numpy()
    assert [list(map(int, r)) for r in zip(g["id"], g["tag"], g["fixed"], g["aux"])] == c["rows"]


def archive_bytes(m):
    d = nxo.Decoded(len(m.id), len(m.ctag) + 1, 1)
    for k in ("id", "tag", "fixed", "aux"):
        getattr(d, k)[:len(m.id)] = getattr(m, k)
    d.ctag[:len(m.ctag)] = m.ctag
    d.cfixed[:len(m.ctag)] = m.cfixed
    d.caux[:len(m.ctag)] = m.caux
    d.s.n_rows, d.s.n_children = len(m.id), len(m.ctag)
    return np.frombuffer(nxo.encode_archive(d, m.heap), np.uint8)


@pytest.mark.parametrize("n", [1, 100, 50_000, 1_000_000])
def test_archive_mixed_vs_oracle(codec, n):
    from netidx_amd import synth
    buf = archive_bytes(synth.archive_columns(n, seed=100 + n % 97))
    st = assert_matches_oracle(codec, buf)
    assert st.n_rows == n and st.path == 5  # the fast path


def test_archive_trailing_bytes_not_read(codec):
    """The uncompressed reader decodes from the record to the end of the mmap (reader.rs:449):
    whatever follows the batch -- here 1 MiB of random bytes -- is neither decoded nor
    reported."""
    from netidx_amd import synth
    buf = archive_bytes(synth.archive_columns(20_000, seed=7))
    junk = np.random.default_rng(8).integers(0, 256, 1 << 20, dtype=np.uint8)
    st = assert_matches_oracle(codec, np.concatenate([buf, junk]))
    assert st.n_rows == 20_000 and st.path == 5


def test_archive_long_values_across_chunks(codec):
    """Strings, bytes and arrays spanning many 1 KiB chunks, mixed with short items; bytes
    payloads full of byte patterns that decode as plausible items."""
    rng = np.random.default_rng(9)
    parts = []
    items = 0
    for i in range(3000):
        u = rng.random()
        parts.append(nxo_varint(int(rng.integers(0, 2**32))))
        if u < 0.02:
            s = bytes(rng.integers(0x61, 0x7B, int(rng.integers(2000, 70000)), dtype=np.uint8))
            parts.append(b"\x0c" + nxo_varint(len(s)) + s)
        elif u < 0.04:  # Bytes that look like items: runs of 09 <8 bytes> and 00 <4 bytes>
            pat = (b"\x01\x09" + bytes(8) + b"\x02\x00" + bytes(4)) * int(rng.integers(50, 3000))
            parts.append(b"\x0d" + nxo_varint(len(pat)) + pat)
        elif u < 0.06:
            k = int(rng.integers(100, 3000))
            parts.append(b"\x13" + nxo_varint(k) + (b"\x09" + bytes(8)) * k)
        elif u < 0.1:
            parts.append(b"\x40")
        else:
            parts.append(b"\x09" + rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
        items += 1
    buf = np.frombuffer(nxo_varint(items) + b"".join(parts), np.uint8)
    st = assert_matches_oracle(codec, buf)
    assert st.n_rows == items


def nxo_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def test_archive_errors_deep_in_the_batch(codec):
    """The first error in stream order, far from the start: an unknown tag, invalid UTF-8 and a
    count larger than the items present (BufferShort at the end)."""
    from netidx_amd import synth
    m = synth.archive_columns(200_000, seed=11)
    buf = archive_bytes(m)
    d, _ = nxo.decode_archive(buf)
    # find item starts through the oracle's rows: corrupt the tag of a late F64 row
    rows = np.nonzero(m.tag == 9)[0]
    r = int(rows[len(rows) * 3 // 4])
    enc = buf.copy()
    # the F64 row's tag byte: search its 9-byte payload after its id varint
    val = int(m.fixed[r]).to_bytes(8, "big")
    pos = bytes(enc).find(b"\x09" + val)
    assert pos > 0
    enc[pos] = 0x1c
    assert_matches_oracle(codec, enc)
    # a bad UTF-8 byte inside a late string
    strs = np.nonzero(m.tag == 12)[0]
    s = int(strs[len(strs) * 2 // 3])
    if m.aux[s] >= 2:
        body = bytes(m.heap[int(m.fixed[s]):int(m.fixed[s]) + int(m.aux[s])])
        p = bytes(buf).find(b"\x0c" + bytes([len(body)]) + body)
        if p > 0:
            enc = buf.copy()
            enc[p + 2] = 0xFF
            assert_matches_oracle(codec, enc)
    # count larger than the items
    hdr = nxo_varint(len(m.id) + 3)
    n0 = len(nxo_varint(len(m.id)))
    enc = np.frombuffer(hdr + bytes(buf[n0:]), np.uint8)
    st = assert_matches_oracle(codec, enc)
    assert st.err_kind == 4 and st.err_offset == len(enc)


def test_archive_capacity(codec):
    from netidx_amd import synth
    buf = archive_bytes(synth.archive_columns(10_000, seed=12))
    # (a band as long as the batch's rows: whatever a decoder wrote behind the 5000th row is seen)
    st = assert_matches_oracle(codec, buf, spare=10_512, cap_rows=5000)
    assert st.err_kind == 7
    cols, st, used = gpu_decode(codec, buf, cap_rows=10_000, spare=10_512)
    assert st.err_kind == 0 and st.n_rows == 10_000


@pytest.mark.parametrize("n", [0, 1, 1000, 1_000_000])
def test_archive_encode_vs_oracle(codec, n):
    """nxg_encode_archive_batch (<Vec<BatchItem> as Pack>::encode, pack.rs:941-952) byte-identical
    to the oracle's encoder, and decoded back to the same columns."""
    import torch
    import netidx_amd
    from netidx_amd import synth
    m = synth.archive_columns(max(n, 1), seed=200 + n % 89)
    if n == 0:
        m = type(m)(m.id[:0], m.tag[:0], m.fixed[:0], m.aux[:0], m.ctag[:0], m.cfixed[:0],
                    m.caux[:0], m.heap)
    ref = archive_bytes(m)
    cols = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
    heap = torch.from_numpy(m.heap.copy()).cuda()
    got = codec.encode_archive(cols, heap).cpu().numpy()
    assert np.array_equal(got, ref)
    if n:
        st = assert_matches_oracle(codec, got)
        assert st.n_rows == n


def _exact_codec():
    import netidx_amd
    os.environ["NXG_ARCH_PATH"] = "exact"
    try:
        return netidx_amd.Codec(0)
    finally:
        del os.environ["NXG_ARCH_PATH"]


def test_archive_fast_equals_exact_every_column(codec):
    """The fast path (nxg_archive_fast.hip) and the exact decoder give the same columns, children,
    consumed bytes on the config-3 mix, on Bytes payloads full of item-like patterns and around
    every tile edge; trailing bytes that parse as items, as garbage, or as nothing at all."""
    from netidx_amd import synth
    ex = _exact_codec()
    try:
        rng = np.random.default_rng(21)
        bufs = [archive_bytes(synth.archive_columns(n, seed=300 + n)) for n in (1, 2, 63, 4000, 300_000)]
        base = bufs[3]
        bufs.append(np.concatenate([base, base]))  # a second batch after the first
        bufs.append(np.concatenate([base, np.zeros(5000, np.uint8)]))
        bufs.append(np.concatenate([base, rng.integers(0, 256, 9000, dtype=np.uint8)]))
        for b in bufs:
            a, sa, ua = gpu_decode(codec, b)
            e, se, ue = gpu_decode(ex, b)
            assert (sa.path, se.path) == (5, 3)
            assert (sa.err_kind, sa.n_rows, sa.n_children, ua) == (se.err_kind, se.n_rows,
                                                                   se.n_children, ue)
            ga, ge = a.numpy(), e.numpy()
            for k in COLS:
                assert np.array_equal(ga[k], ge[k]), k
    finally:
        ex.close()


@pytest.mark.parametrize("case", ["every_tag", "unsub_runs", "long_text", "long_text_4000",
                                  "long_text_20000", "tile_edges", "wide_ids", "arrays"])
def test_archive_fast_cases_vs_oracle(codec, case):
    """Batches built item by item: every leaf tag, runs of Unsubscribed, text of 100 .. 20000
    bytes (past a tile's image: checked from global memory), items of every length around the
    4 KiB tile edges, 1..5-byte Ids and ids wider than u32, arrays of every element kind."""
    import random
    import importlib.util
    spec = importlib.util.spec_from_file_location("mg", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    rng = random.Random(zlib.crc32(case.encode()))  # (hash() of a str varies per process)
    items = []
    for i in range(6000):
        idb = rng.choice([7, 14, 21, 28, 32]) if case != "wide_ids" else rng.choice([33, 35, 40])
        iid = rng.getrandbits(idb)
        if case == "unsub_runs" and (i // 50) % 2:
            items.append(nxo_varint(iid) + b"\x40")
            continue
        if case.startswith("long_text") and rng.random() < 0.05:
            sizes = {"long_text": [100, 300, 4000, 20000], "long_text_4000": [4000],
                     "long_text_20000": [20000]}[case]
            s = bytes(rng.randrange(0x61, 0x7b) for _ in range(rng.choice(sizes)))
            if rng.random() < 0.5:
                s = s[:50] + "é".encode() + s[52:]
            v = (12, s)
        elif case == "tile_edges":
            v = (12, b"e" * rng.randrange(0, 120))
        elif case == "arrays":
            def leaf():
                e = mg.rand_value(rng, 1)
                while e[0] in (19, 21, 22):
                    e = mg.rand_value(rng, 1)
                return e
            v = (19, [leaf() for _ in range(rng.randrange(0, 20))])
        else:
            v = mg.rand_value(rng)
            while v[0] in (19, 21, 22):
                v = mg.rand_value(rng)
        items.append(nxo_varint(iid) + mg.enc_value(v))
    buf = np.frombuffer(nxo_varint(len(items)) + b"".join(items), np.uint8)
    st = assert_matches_oracle(codec, buf)
    if case != "wide_ids":
        assert st.path == 5, (case, st.path)
