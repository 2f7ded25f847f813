"""Records for the zstd compressor's block trees (NxgZstdCompressOpts.literals = 1), shared by
tests/test_gpu_zstd_compress_trees.py, tests/test_zstd_gpu_trees_golden_cpu.py and the generator of
their golden pin (tests/golden/make_zstd_gpu_trees.py). Small on purpose: the format's block is
128 KiB, so the two-block records are the smallest that carry a tree from one block to the next,
and they are filled with one long match so that few literals are coded."""
import random

import zstd_enc_cases as zc

BLOCK_TREES = 1


def uniform(n, seed, lo=0, span=64):
    """n bytes drawn uniformly from [lo, lo + span): 4-byte repeats are rare, a flat code fits"""
    rng = random.Random(seed)
    return bytes(lo + rng.randrange(span) for _ in range(n))


def skewed(n, seed):
    """n bytes over 40 byte values of geometrically falling frequency: a deep tree"""
    rng = random.Random(seed)
    syms = rng.sample(range(256), 40)
    return bytes(syms[min(int(rng.expovariate(0.25)), 39)] for _ in range(n))


def no_match(n, seed):
    """exactly n literals: n bytes over 64 values (a few above 128) with no repeated 3 bytes"""
    syms = list(range(20, 80)) + [130, 140, 200, 255]
    b = zc.no_repeat_payload(syms, n, b"", seed)
    assert len(b) == n
    return b


def two_blocks(second_lo):
    """A first block of 3000 uniform bytes below 64 and one long match (a 64-byte pattern of the
    same values), a second block of 400 uniform bytes from [second_lo, second_lo + 64): with
    second_lo = 0 the second block's literals all have codes in the first block's tree and a
    description would cost more than it saves, with 64 none has a code."""
    head = uniform(3000, 21)
    pat = list(range(64))
    random.Random(23).shuffle(pat)
    fill = bytes(pat) * ((zc.BLOCK - len(head)) // 64 + 1)
    return (head + fill)[:zc.BLOCK] + uniform(400, 22, second_lo)


def tree_records(d):
    """name -> payload"""
    c = zc.crafted(d)
    out = {
        "huf1": c["huf1"],          # the dictionary's tree fits: treeless with a dictionary
        "huf4": c["huf4"],
        "dict_slice": c["dict_slice"],
        "one_byte": c["one_byte"],
        "low64": uniform(3000, 64),  # the derivable bound; direct weights
        "skewed": skewed(6000, 7),   # FSE-compressed weights, the length limit
        "tiny8": uniform(8, 8, 0, 2),
        "two_blocks_reuse": two_blocks(0),
        "two_blocks_new_tree": two_blocks(64),
    }
    for n in (1023, 1024, 16383, 16384):
        out["lits%d" % n] = no_match(n, n)
    return out


def dictionaries(d):
    """[(name, dictionary bytes or None)]: zstd format, raw content, none"""
    return [("dict", d), ("raw-content", zc.dict_parts(d)[2]), ("none", None)]


def lit_section(body):
    """(Literals_Block_Type, Size_Format, regenerated size, section bytes) of a compressed block's
    literals section"""
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    if lt <= 1:
        lhs = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        rs = int.from_bytes(body[:lhs], "little") >> (3 if lhs == 1 else 4)
        return lt, sf, rs, lhs + (rs if lt == 0 else 1)
    lhs, nb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    h = int.from_bytes(body[:lhs], "little")
    return lt, sf, (h >> 4) & ((1 << nb) - 1), lhs + ((h >> (4 + nb)) & ((1 << nb) - 1))


def small_dict_missing_codes():
    """(a zstd-format dictionary whose tree codes 16 byte values only, those values): the `fmt1`
    dictionary of tests/golden/make_zstd_valid.py"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("mzv", os.path.join(zc.G, "make_zstd_valid.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.dicts()["fmt1"][0], list(m.SYM16)


def first_lit_types(frame):
    """Literals_Block_Type of every compressed block of a frame (None for raw / RLE blocks)"""
    return [lit_section(frame[o:o + size])[0] if typ == 2 else None
            for typ, _, size, o in zc.blocks(frame)]
