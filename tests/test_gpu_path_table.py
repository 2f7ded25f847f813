"""GPU tests of the device-resident by_path (nxg_path_table_*): every answer against a Python dict
holding the same paths. The lookup call is the seam: what was inserted is found with its Id, what
was not (near misses of the same length, prefixes, removed paths) is NXG_NO_ID."""
import random

import pytest

pytestmark = pytest.mark.gpu

NO_ID = 2**64 - 1
BLOCK = 256  # paths per workgroup of the table's kernels (nxg_internal.h kRwBlock)
M64 = 2**64 - 1


@pytest.fixture
def codec():
    import torch
    import netidx_amd
    assert torch.cuda.is_available()
    c = netidx_amd.Codec(0)
    yield c
    c.close()


def table(codec, cap_paths, cap_bytes=1 << 16):
    from netidx_amd.codec import PathTable
    return PathTable(codec, cap_paths, cap_bytes)


def home_slot(p, slots):
    """Where the table's probe for path p starts (the hash of nxg_route_subscribes.hip, restated:
    used only to pick paths that share a chain)."""
    def mix(h, w):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & M64
        return h ^ (h >> 29)
    h = 0x243F6A8885A308D3 ^ len(p)
    for i in range(0, len(p), 8):
        h = mix(h, int.from_bytes(p[i:i + 8], "little"))
    h ^= h >> 32
    h = (h * 0xD6E8FEB86659FD93) & M64
    h ^= h >> 29
    return (h + 2 if h < 2 else h) & (slots - 1)


def test_empty_table_and_one_path(codec):
    t = table(codec, 4)
    assert len(t) == 0 and t.lookup([b"/a", b""]) == [NO_ID, NO_ID]
    assert t.insert([], []) == 0 and t.remove([]) == 0 and t.lookup([]) == []
    assert t.insert([b"/a"], [7]) == 0 and len(t) == 1
    assert t.lookup([b"/a", b"/b", b"/", b"/a/", b"/aa", b""]) == [7] + [NO_ID] * 5


def test_a_full_table_finds_every_path_and_no_near_miss(codec):
    cap = 1000  # exactly the capacity: the slots are half full, the longest chains allowed
    paths = [b"/app/%04d/value" % i for i in range(cap)]
    t = table(codec, cap)
    assert t.insert(paths, [3 * i + 1 for i in range(cap)]) == 0 and len(t) == cap
    assert t.lookup(paths) == [3 * i + 1 for i in range(cap)]
    miss = [b"/app/%04d/valuf" % i for i in range(cap)] + [b"/bpp/%04d/value" % i for i in range(cap)]
    assert t.lookup(miss) == [NO_ID] * (2 * cap)


def test_paths_that_differ_late_share_prefixes_or_are_prefixes(codec):
    base8, base64 = b"/abcdefg", b"/" + b"p" * 63
    paths = [b"/x/a", b"/x/b",                         # the last byte
             base8 + b"1", base8 + b"2", base8,        # the first 8 bytes; a proper prefix
             base64 + b"/1", base64 + b"/2", base64,   # the first 64 bytes
             b"a", b"ab", b"q" * 127, b"q" * 128, b"/" + b"r" * 299,  # lengths 1, 2, 127, 128, 300
             b"q" * 126 + b"r", b"q" * 127 + b"r"]
    t = table(codec, len(paths))
    assert t.insert(paths, list(range(100, 100 + len(paths)))) == 0
    assert t.lookup(paths) == list(range(100, 100 + len(paths)))
    miss = [b"/x/c", b"/x/", b"/x", base8 + b"3", base8[:-1], base64 + b"/3", base64[:-1],
            b"b", b"aa", b"q" * 126, b"q" * 129, b"/" + b"r" * 298, b"/" + b"r" * 298 + b"s",
            b"q" * 120 + b"r" + b"q" * 6]
    assert t.lookup(miss) == [NO_ID] * len(miss)


def test_duplicates_inside_a_call_and_of_an_existing_path(codec):
    t = table(codec, 600)
    assert t.insert([b"/old"], [1]) == 0
    # /dup three times: index 1 wins over 3 and 5; /old keeps its Id
    assert t.insert([b"/n1", b"/dup", b"/old", b"/dup", b"/n2", b"/dup"], [10, 11, 12, 13, 14, 15]) == 3
    assert len(t) == 4
    assert t.lookup([b"/old", b"/dup", b"/n1", b"/n2"]) == [1, 11, 10, 14]
    # many copies spread over several workgroups: the lowest index of each path wins
    paths = [b"/k/%d" % (i % 37) for i in range(500)]
    assert t.insert(paths, [1000 + i for i in range(500)]) == 500 - 37
    assert t.lookup([b"/k/%d" % i for i in range(37)]) == [1000 + i for i in range(37)]
    assert len(t) == 41


def test_remove_leaves_a_tombstone_that_lookups_pass_and_inserts_reuse(codec):
    slots = 16  # cap_paths 8
    cands = [b"/c/%d" % i for i in range(400)]
    by_home = {}
    for p in cands:
        by_home.setdefault(home_slot(p, slots), []).append(p)
    a, b, c, d = max(by_home.values(), key=len)[:4]  # four paths whose probes start at one slot
    t = table(codec, 8)
    assert t.insert([a], [1]) == 0 and t.insert([b], [2]) == 0 and t.insert([c], [3]) == 0
    assert t.remove([a, b"/absent"]) == 1 and len(t) == 2
    assert t.lookup([a, b, c]) == [NO_ID, 2, 3]           # b and c sit behind a's tombstone
    assert t.remove([b]) == 0 and t.lookup([a, b, c, d]) == [NO_ID, NO_ID, 3, NO_ID]
    assert t.insert([d], [4]) == 0 and t.insert([a], [5]) == 0  # into the tombstones
    assert t.lookup([a, b, c, d]) == [5, NO_ID, 3, 4] and len(t) == 3
    assert t.insert([c], [9]) == 1 and t.lookup([c]) == [3]    # still found past the reused slots
    assert t.remove([a, a]) == 1 and t.remove([a]) == 1         # named twice: one finds it


def test_remove_half_of_a_full_table(codec):
    rng = random.Random(5)
    cap = 700
    paths = [b"/r/%x/%d" % (rng.getrandbits(24), i) for i in range(cap)]
    want = {p: i for i, p in enumerate(paths)}
    t = table(codec, cap, 1 << 17)
    assert t.insert(paths, list(range(cap))) == 0
    gone = paths[::2]
    assert t.remove(gone + [b"/never"]) == 1
    for p in gone:
        del want[p]
    assert t.lookup(paths) == [want.get(p, NO_ID) for p in paths] and len(t) == len(want)
    # reinsert after remove, with new Ids (len + n == cap_paths again); the survivors keep theirs
    assert t.insert(gone, [5000 + i for i in range(len(gone))]) == 0 and len(t) == cap
    want.update({p: 5000 + i for i, p in enumerate(gone)})
    assert t.lookup(paths) == [want[p] for p in paths]


def test_many_rounds_of_insert_and_remove_compact_the_slots(codec):
    t = table(codec, 64, 1 << 16)  # 128 slots: tombstones of a few rounds would fill them
    keep = [b"/keep/%d" % i for i in range(10)]
    assert t.insert(keep, list(range(10))) == 0
    for rnd in range(8):
        paths = [b"/round/%d/%d" % (rnd, i) for i in range(48)]
        assert t.insert(paths, [100 * rnd + i for i in range(48)]) == 0
        assert t.lookup(paths + keep) == [100 * rnd + i for i in range(48)] + list(range(10))
        assert t.remove(paths) == 0 and len(t) == 10
    assert t.lookup([b"/round/3/7"] + keep) == [NO_ID] + list(range(10))


def test_insert_past_the_capacity_is_refused_and_changes_nothing(codec):
    import netidx_amd
    t = table(codec, 5, 64)
    assert t.insert([b"/a", b"/b", b"/c"], [1, 2, 3]) == 0
    with pytest.raises(netidx_amd.CodecError, match="NXG_CAPACITY"):
        t.insert([b"/d", b"/e", b"/f"], [4, 5, 6])           # 3 + 3 > 5 paths
    with pytest.raises(netidx_amd.CodecError, match="NXG_CAPACITY"):
        t.insert([b"/" + b"z" * 60], [7])                     # 6 + 61 > 64 bytes
    with pytest.raises(netidx_amd.CodecError, match="NXG_NO_ID"):
        t.insert([b"/g"], [NO_ID])
    assert len(t) == 3
    assert t.lookup([b"/a", b"/b", b"/c", b"/d", b"/e", b"/f", b"/g"]) == [1, 2, 3] + [NO_ID] * 4
    assert t.insert([b"/d", b"/e"], [4, 5]) == 0 and t.lookup([b"/d", b"/e"]) == [4, 5]


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_counts_around_the_block(codec, n):
    rng = random.Random(n)
    paths = [b"/n/%d/%s" % (i, b"s" * rng.randrange(0, 40)) for i in range(n)]
    ids = [rng.getrandbits(64) % NO_ID for _ in range(n)]
    t = table(codec, n, 1 << 16)
    assert t.insert(paths, ids) == 0 and len(t) == n
    assert t.lookup(paths) == ids
    assert t.remove(paths[: n // 2]) == 0
    assert t.lookup(paths) == [NO_ID] * (n // 2) + ids[n // 2:]
