"""The sequential-id f64 decoder's uniform-width body (nxg_decode_f64_seq.hip,
emit_full_pairs_uniform) against the CPU oracle.

A full wave whose ids all have one varint width checks each record's header by equality with the
one header it may have (L, 04, the canonical varint of the expected id, 09) and writes the expected
id; a wave with a width change inside keeps the generic body, the frame's last wave the edge body.
Frames here are 1,300 records: with 4 records per lane (256 per wave) five full waves and a
20-record edge wave. These tests pin:
  - bit-exact columns, on the sequential-id kernel, for frames whose full waves are all uniform
    (id widths 2..5), frames with a width change inside a full wave, and record counts around the
    wave and frame-end boundaries;
  - that the equality accepts nothing the generic checks reject: every single-byte corruption of
    a record header (length, variant, each id byte's low and continuation bit, value tag), in pair
    slot a and b of lanes 0, 31 and 63, in the first and last batch of the first and last full
    wave, gives the oracle's result for those bytes and is not reported as decoded by the
    sequential-id kernel;
  - value bytes pass through bit-exactly, header look-alikes included.
Reference rules: netidx-core/src/pack.rs:504-555, netidx-value/src/lib.rs:404-407, 470-506.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1300
UNIFORM_I0 = [200, 20_000, 2**21 + 5, 2**28 + 5]  # id widths 2, 3, 4, 5 for all 1,300 ids
CROSSING_I0 = [0, 16384 - 700, 2**21 - 700]       # a width change inside a full wave


def _wire(n, i0, seed):
    import nxo
    from netidx_amd import synth
    ids, vals = synth.f64_columns(n, seed, id_offset=i0)
    return ids, vals, nxo.encode_f64(ids, vals)


def _oracle(b):
    import nxo
    return nxo.decode(np.ascontiguousarray(b), cap_rows=len(b) + 1, cap_children=len(b) + 1,
                      cap_ctl=len(b) + 1).trim()


def _decode_mixed(codec, b):
    """Decode into mixed-capable columns (a corrupted frame may hold any message)."""
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns
    cols = Columns(len(b) + 1, len(b) + 1, len(b) + 1, netidx_amd.LAYOUT_MIXED, "cuda")
    dw = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    st = codec.decode_into(dw, dw.numel(), cols, 0, check=False)
    return cols, st, codec.last_diag()


def _same_as_oracle(cols, st, o, what):
    assert st.err_kind == o["err_kind"], (what, st.err_kind, o["err_kind"])
    if o["err_kind"]:
        assert st.err_offset == o["err_offset"], (what, st.err_offset, o["err_offset"])
        return
    n = len(o["id"])
    assert st.n_rows == n, (what, st.n_rows, n)
    g = cols.numpy()
    assert np.array_equal(g["id"][:n], o["id"]), what
    assert np.array_equal(g["fixed"][:n], o["fixed"]), what


@pytest.fixture(scope="module")
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


@pytest.mark.parametrize("i0", UNIFORM_I0 + CROSSING_I0)
def test_valid_frames_decode_on_the_sequential_id_kernel(codec, i0):
    for n in (256, 257, 1024, 1279, 1280, 1281, N):
        ids, vals, wire = _wire(n, i0, n)
        cols, st, diag = _decode_mixed(codec, wire)
        assert st.err_kind == 0 and st.n_rows == n
        g = cols.numpy()
        o = _oracle(wire)
        assert np.array_equal(g["id"][:n], o["id"]) and np.array_equal(g["fixed"][:n], o["fixed"])
        assert np.array_equal(g["id"][:n], ids) and np.array_equal(g["fixed"][:n], vals)
        assert st.path == 1 and diag[1] == 1, (i0, n, st.path, diag)


def _corruptions(nb):
    """(name, byte offset in the record, xor mask or signed delta)"""
    out = [("len+1", 0, "+"), ("len-1", 0, "-"), ("variant", 1, 0x04 ^ 0x05)]
    for j in range(nb):
        out.append((f"id{j}.low", 2 + j, 0x01))
        out.append((f"id{j}.cont", 2 + j, 0x80))
    out.append(("tag", 2 + nb, 0x09 ^ 0x0a))
    return out


def _records():
    """Pair slots a and b of lanes 0, 31, 63, in the first and last batch of waves 0 and 4: a
    wave holds 256 records, a batch 128 (lane j of batch r takes 128 r + 2 j and the next)."""
    return [256 * wave + 128 * batch + 2 * lane + slot
            for wave in (0, 4) for batch in (0, 1) for lane in (0, 31, 63) for slot in (0, 1)]


@pytest.mark.parametrize("i0", UNIFORM_I0)
def test_single_byte_header_corruptions_are_never_accepted(i0):
    import netidx_amd
    ids, vals, wire = _wire(N, i0, 77)
    nb = {200: 2, 20_000: 3, 2**21 + 5: 4, 2**28 + 5: 5}[i0]
    L = 11 + nb
    assert len(wire) == N * L
    clean = np.frombuffer(bytes(wire), np.uint8)
    cases = 0
    for rec in _records():
        for name, off, how in _corruptions(nb):
            b = clean.copy()
            p = rec * L + off
            if how == "+":
                b[p] += 1
            elif how == "-":
                b[p] -= 1
            else:
                b[p] ^= how
            o = _oracle(b)
            c = netidx_amd.Codec(0)  # fresh: the skip after a hand-over must not mask a case
            try:
                cols, st, diag = _decode_mixed(c, b)
                _same_as_oracle(cols, st, o, (i0, rec, name))
                assert diag[1] != 1, (i0, rec, name, diag)
            finally:
                c.close()
            cases += 1
    assert cases == 24 * (4 + 2 * nb)


def test_value_bytes_pass_through(codec):
    """f64 bit patterns that are zero, all ones, NaNs or look like a record header."""
    import nxo
    special = np.array([0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 0xFFF8000000000001,
                        0x7FF0000000000001, 0x0C04C80109000000, 0x0D04A09C01090000,
                        0x0F0485808001090C, 0x0409090909090909, 0x0E04858080010900,
                        0x8080808080808080, 0x090C04C801090C04], np.uint64)
    for i0 in UNIFORM_I0:
        ids = np.arange(i0, i0 + N, dtype=np.uint64)
        vals = special[(np.arange(N) * 5 + i0) % len(special)]
        wire = nxo.encode_f64(ids, vals)
        cols, st, diag = _decode_mixed(codec, wire)
        assert st.err_kind == 0 and st.n_rows == N and diag[1] == 1
        g = cols.numpy()
        o = _oracle(wire)
        assert np.array_equal(g["id"][:N], o["id"]) and np.array_equal(g["fixed"][:N], o["fixed"])
        assert np.array_equal(g["id"][:N], ids) and np.array_equal(g["fixed"][:N], vals)
