"""The encode-side zstd format code (netidx_amd/csrc/nxg_zstd_enc.h: code tables, FSE encoding
tables, Huffman codes from the dictionary's weights, literals and sequences sections, frame
headers) on the CPU: the library's host-only encoder (nxg_debug_zstd_compress_host, the device's
format code behind a serial matcher) compresses every fixture payload and the crafted ones, and
libzstd turns each frame back into the input. The GPU compressor is checked in
tests/test_gpu_zstd_compress.py."""
import ctypes as C
import random

import pytest

import zstd_enc_cases as zc


def host_compress(b, d):
    from netidx_amd.codec import lib
    f = lib().nxg_debug_zstd_compress_host
    f.restype = C.c_uint64
    f.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
    cap = zc.worst_case(0, len(b)) - 4
    out = C.create_string_buffer(cap)
    assert f(d, len(d) if d else 0, b, len(b), out, cap - 1) == 0  # below the bound: refused
    n = f(d, len(d) if d else 0, b, len(b), out, cap)
    assert 0 < n <= cap
    return out.raw[:n]


def payloads():
    ents, rec, plain, d = zc.load_fixtures()
    for e in ents:
        yield e["kind"], plain[e["plain_off"]:e["plain_off"] + e["plain_len"]], e["dict"]
    for name, b in zc.crafted(d).items():
        yield name, b, True
    rng = random.Random(5)
    words = [bytes(rng.getrandbits(8) for _ in range(5)) for _ in range(50)]
    for k in (100, 200, 40000):  # the sequence count's 1-, 2- and 3-byte forms
        yield "seqs%d" % k, b"".join(words[rng.randrange(50)] + bytes([rng.getrandbits(8)])
                                     for _ in range(k)), True
    for n in (1, 2, 31, 32, 1023, 1024, 4095, 4096, 16384, 131073):  # literals header forms
        yield "lits%d" % n, bytes(rng.choice(b"\x00\x06\x09\xff\x0c\x13A\xc1") for _ in range(n)), True


def test_host_encoder_frames_are_libzstd_frames():
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here")
    d = zc.load_fixtures()[3]
    did = zc.dict_parts(d)[0]
    for name, b, use_dict in payloads():
        f = host_compress(b, d if use_dict else None)
        zc.check_frame_header(f, len(b), did if use_dict else 0)
        assert z.decompress(f, len(b), d if use_dict else None) == b, name


def test_sequence_count_forms_and_bounds():
    d = zc.load_fixtures()[3]
    c = zc.crafted(d)
    assert len(host_compress(c["dict_slice"], d)) <= 512
    assert len(host_compress(c["pattern64"], d)) * 8 <= len(c["pattern64"])
    assert len(host_compress(c["one_byte"], d)) <= 64
    f = host_compress(c["random70000"], d)
    assert [t for t, _, _, _ in zc.blocks(f)] == [0]  # incompressible: a raw block
    assert host_compress(b"", d)[-3:] == b"\x01\x00\x00"


def test_sequence_section_count_forms_against_libzstd():
    """Number_of_Sequences in its 1-, 2- and 3-byte forms (below 128, below 0x7F00, above) and the
    predefined-table bitstream for each: a block of given literals and sequences encoded by
    encode_sequences (nxg_debug_zstd_encode_seqs), decoded by libzstd, against the bytes the
    sequences mean."""
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here")
    from netidx_amd.codec import lib
    f = lib().nxg_debug_zstd_encode_seqs
    f.restype = C.c_uint64
    U32 = C.POINTER(C.c_uint32)
    f.argtypes = [C.c_char_p, C.c_uint32, U32, U32, U32, C.c_uint32, C.c_uint64, C.c_char_p,
                  C.c_uint64]
    for nseq in (1, 127, 128, 0x7EFF, 0x7F00, 33000):
        rng = random.Random(nseq)
        lits, plain = bytearray(), bytearray()
        off, ll, ml = [], [], []
        for i in range(nseq):
            n = 8 if i == 0 else rng.choice((0, 0, 0, 1))
            new = bytes(rng.getrandbits(8) for _ in range(n))
            lits += new
            plain += new
            o = rng.randint(1, min(13, len(plain)))
            m = rng.choice((3, 3, 3, 4)) if nseq > 1000 else rng.choice((3, 7, 40, 300))
            for _ in range(m):
                plain.append(plain[-o])
            off.append(o)
            ll.append(n)
            ml.append(m)
        tail = bytes(rng.getrandbits(8) for _ in range(5))  # literals after the last sequence
        lits += tail
        plain += tail
        assert len(plain) <= 128 * 1024
        A = C.c_uint32 * nseq
        out = C.create_string_buffer(len(plain) + 64)
        n = f(bytes(lits), len(lits), A(*off), A(*ll), A(*ml), nseq, len(plain), out, len(out))
        assert n, nseq
        frame = out.raw[:n]
        body = frame[zc.blocks(frame)[0][3]:]
        sec = body[zc_raw_lit_section(body):]
        want = (bytes([nseq]) if nseq < 128 else
                bytes([(nseq >> 8) + 128, nseq & 255]) if nseq < 0x7F00 else
                bytes([255]) + (nseq - 0x7F00).to_bytes(2, "little"))
        assert sec[:len(want)] == want and sec[len(want)] == 0  # the count, predefined modes
        assert z.decompress(frame, len(plain)) == bytes(plain), nseq


def zc_raw_lit_section(body):
    """bytes of a raw literals section at body[0:]"""
    sf = (body[0] >> 2) & 3
    assert body[0] & 3 == 0
    if sf in (0, 2):
        return 1 + (body[0] >> 3)
    if sf == 1:
        return 2 + ((body[0] >> 4) | (body[1] << 4))
    return 3 + ((body[0] >> 4) | (body[1] << 4) | (body[2] << 12))
