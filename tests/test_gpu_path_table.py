"""GPU tests of the device-resident by_path (nxg_path_table_*): every answer against a Python dict
holding the same paths. The lookup call is the seam: what was inserted is found with its Id, what
was not (near misses of the same length, prefixes, removed paths) is NXG_NO_ID. The second half
uses the crafted keys of tests/path_table_cases.py (paths with one hash, raw hashes 0-3, chains
that wrap) and a model that also keeps the table's accounting: capacities, and when it rehashes."""
import random

import pytest

import path_table_cases as pc

pytestmark = pytest.mark.gpu

NO_ID = 2**64 - 1
BLOCK = 256  # paths per workgroup of the table's kernels (nxg_internal.h kRwBlock)


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


home_slot = pc.home_slot  # (the restated hash, checked against nxg_path_hash on the CPU)


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


# ---- crafted keys (tests/path_table_cases.py) against a dict model with the table's accounting ----
class Model:
    """by_path as a dict, with the accounting include/nxg_codec.h states: an insert of n paths is
    refused when len + n > cap_paths, or when the call's bytes (duplicates included) exceed what
    is left of cap_bytes, which removed paths never give back. The slots that are not empty (live
    paths and tombstones) are tracked as bounds (lo, hi): exact after a rehash and while no
    tombstone exists; an insert next to tombstones reuses those its chains meet. The table
    rehashes in front of an insert of n paths when used + n > 3/4 of the slots."""

    def __init__(self, cap_paths, cap_bytes=1 << 16):
        self.cap_paths, self.cap_bytes = cap_paths, cap_bytes
        self.slots = 16
        while self.slots < 2 * cap_paths:
            self.slots *= 2
        self.thr = self.slots // 4 * 3
        self.d, self.heap, self.used, self.rehashes = {}, 0, (0, 0), 0

    def fits(self, paths):
        return (len(paths) <= self.cap_paths - len(self.d)
                and sum(len(p) for p in paths) <= self.cap_bytes - self.heap)

    def rehash_on(self, n):
        """Whether an insert of n paths rehashes first: True / False where the bounds decide it."""
        lo, hi = self.used
        return True if lo + n > self.thr else False if hi + n <= self.thr else None

    def insert(self, paths, ids):
        assert self.fits(paths) and len(paths) == len(ids)
        r, (lo, hi) = self.rehash_on(len(paths)), self.used
        if r:
            lo = hi = len(self.d)
            self.rehashes += 1
        elif r is None:
            lo = len(self.d)
        dup = new = 0
        for p, i in zip(paths, ids):
            if p in self.d:
                dup += 1
            else:
                self.d[p] = i
                new += 1
        self.heap += sum(len(p) for p in paths)
        self.used = (max(lo, len(self.d)), hi + new)  # every new path in a tombstone / in none
        return dup

    def remove(self, paths):
        miss = 0
        for p in paths:
            if self.d.pop(p, None) is None:
                miss += 1
        return miss


class Pair:
    """A table and its model, driven together; every call is followed by a lookup of `universe`."""

    def __init__(self, codec, cap_paths, universe, cap_bytes=1 << 16):
        self.t, self.m = table(codec, cap_paths, cap_bytes), Model(cap_paths, cap_bytes)
        self.universe = list(universe)

    def check(self):
        assert self.t.lookup(self.universe) == [self.m.d.get(p, NO_ID) for p in self.universe]
        assert len(self.t) == len(self.m.d)

    def ins(self, paths, ids, rehash=None):
        if rehash is not None:  # (the plan of the test, checked before the call is made)
            assert self.m.rehash_on(len(paths)) is rehash, (self.m.used, len(paths))
        want = self.m.insert(paths, ids)
        assert self.t.insert(paths, ids) == want
        self.check()

    def rem(self, paths):
        want = self.m.remove(paths)
        assert self.t.remove(paths) == want
        self.check()


FILL = [b"/fill/%03d" % i for i in range(300)]


def collision_groups():
    return list(pc.collision_pairs()) + list(pc.plain_collision_pairs())


@pytest.mark.parametrize("g", range(5))
def test_paths_with_one_hash_are_told_apart_by_their_bytes(codec, g):
    a, b = collision_groups()[g]
    assert pc.path_hash(a) == pc.path_hash(b) and len(a) == len(b) and a != b
    p = Pair(codec, 8, [a, b])
    p.ins([a], [1])                       # a alone: its partner is not in the table
    assert p.t.lookup([b, a]) == [NO_ID, 1]
    p.rem([b])                            # ... and cannot be removed; a survives
    assert p.t.lookup([a]) == [1] and len(p.t) == 1
    p.ins([b], [2])
    p.ins([b, a], [3, 4])                 # both present: two duplicates, the Ids stay
    assert p.t.lookup([a, b]) == [1, 2]
    q = Pair(codec, 8, [a, b])
    q.ins([a, b], [1, 2])                 # in one call: not duplicates of each other
    assert q.t.lookup([a, b]) == [1, 2] and len(q.t) == 2
    q.rem([a])
    assert q.t.lookup([a, b]) == [NO_ID, 2]
    q.ins([a], [9])                       # again, under a new Id
    assert q.t.lookup([a, b]) == [9, 2]
    q.rem([b, b, a])
    assert len(q.t) == 0


def test_three_paths_with_one_hash_and_a_duplicate(codec):
    a, b, c = pc.collision_triple()
    p = Pair(codec, 8, [a, b, c])
    assert p.t.insert([a, b, c, c], [1, 2, 3, 4]) == p.m.insert([a, b, c, c], [1, 2, 3, 4]) == 1
    assert p.t.lookup([a, b, c]) == [1, 2, 3] and len(p.t) == 3  # the lowest index of c wins
    p.rem([b])
    p.ins([c, b, a], [7, 8, 9])
    assert p.t.lookup([a, b, c]) == [1, 8, 3]


def test_paths_with_one_hash_in_different_workgroups(codec):
    (a, b), (a3, b3, c3) = pc.collision_pairs()[0], pc.collision_triple()
    absent = [b"/absent/%03d" % i for i in range(BLOCK)]
    uni = [a] + FILL[:BLOCK - 1] + [b] + FILL[BLOCK - 1:] + [a3, b3, c3]  # a at 0, b at 256
    assert uni.index(a) == 0 and uni.index(b) == BLOCK
    p = Pair(codec, 512, uni)             # lookups: a and b in different workgroups
    p.ins([a] + FILL, list(range(301)))   # a alone
    assert p.t.lookup(uni)[BLOCK] == NO_ID
    p.rem(absent + [b])                   # b at index 256: missing, a survives
    assert p.t.lookup([a]) == [0]
    q = Pair(codec, 512, uni)
    paths = [a] + FILL[:BLOCK - 1] + [b, a3] + FILL[BLOCK - 1:] + [b3, c3, c3]
    assert paths.index(b) == BLOCK
    q.ins(paths, list(range(1000, 1000 + len(paths))))
    got = dict(zip(uni, q.t.lookup(uni)))
    assert (got[a], got[b]) == (1000, 1000 + BLOCK) and got[c3] == 1000 + len(paths) - 2
    q.rem([a] + FILL[:BLOCK - 1] + [b3])
    assert q.t.lookup([a, b, a3, b3, c3])[::3] == [NO_ID, NO_ID]
    q.ins(FILL[:BLOCK] + [a, b3], list(range(5000, 5000 + BLOCK + 2)))  # a at 256, new Ids
    got = dict(zip(uni, q.t.lookup(uni)))
    assert got[a] == 5000 + BLOCK and got[b] == 1000 + BLOCK and got[b3] == 5001 + BLOCK
    assert got[FILL[0]] == 5000 and got[FILL[BLOCK - 1]] == 1000 + BLOCK + 2  # that one stayed


def test_raw_hashes_that_mean_empty_and_tombstone_are_remapped(codec):
    r = pc.reserved_paths()
    four = [r[0], r[1], r[2], r[3]]
    p = Pair(codec, 8, four)
    assert p.t.lookup(four) == [NO_ID] * 4  # the empty table
    p.ins(four, [10, 11, 12, 13])
    assert len(p.t) == 4 and p.t.lookup(four) == [10, 11, 12, 13]
    p.rem([r[0]])                          # raw 0 and raw 2 are both stored as 2
    assert p.t.lookup([r[0], r[2]]) == [NO_ID, 12]
    p.rem([r[3], r[0]])
    assert p.t.lookup(four) == [NO_ID, 11, 12, NO_ID]
    p.ins([r[0], r[3]], [20, 23])
    p.ins([r[2], r[1]], [30, 31])          # present: duplicates
    assert p.t.lookup(four) == [20, 11, 12, 23]


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("first", ["last", "before"])
def test_chains_that_wrap_from_the_last_slot_to_slot_0(codec, one_call, first):
    last, before = pc.chain_paths(16, 15, 5), pc.chain_paths(16, 14, 3, b"v")
    assert {home_slot(x, 16) for x in last} == {15} and {home_slot(x, 16) for x in before} == {14}
    p = Pair(codec, 8, last + before + (b"/w/none",))

    def put(paths, id0):
        if one_call:  # which slot each gets depends on scheduling; the answers do not
            p.ins(list(paths), list(range(id0, id0 + len(paths))))
        else:
            for k, x in enumerate(paths):
                p.ins([x], [id0 + k])

    a, b, c, d, e = last
    if first == "before":
        put(before, 20)                    # slots 14, 15, 0
    put([a, b, c, d], 1)                   # home 15: across the wrap
    p.rem([a])                             # b, c, d behind a's tombstone
    p.ins([e], [5])
    if first == "last":
        put(before, 20)
    else:
        p.rem([before[0]])
    assert len(p.t) == (7 if first == "last" else 6)
    p.rem([b, before[1], b])
    p.ins([a], [9])
    assert p.t.lookup([a, b, c, d, e]) == [9, NO_ID, 3, 4, 5]


@pytest.mark.parametrize("cap_paths,sizes", [
    # (n, a rehash comes first) per round; Pair.ins checks each against the model's bounds before
    # the call. 16 slots, 3/4 of them 12, 3 survivors: used + n = 3+5 | 8+4 = 12 exactly: none |
    # >= 8+5: #1, used = 3+5 | 8+5 = 13, one more than 12: #2 | 8+4 = 12 | >= 8+5: #3
    (8, [(5, False), (4, False), (5, True), (5, True), (4, False), (5, True)]),
    # 128 slots, 3/4 of them 96, 11 survivors: 11+53 | 64+32 = 96 exactly | >= 64+33: #1, used =
    # 11+33 | 44+53 = 97: #2 | 64+32 = 96 | >= 64+40: #3
    (64, [(53, False), (32, False), (33, True), (53, True), (32, False), (40, True)]),
])
def test_rehash_keeps_colliding_and_wrapping_survivors(codec, cap_paths, sizes):
    slots = 2 * cap_paths
    x, y = pc.collision_pair_at(slots, slots - 1)   # one hash, home in the last slot: slots - 1, 0
    last, before = pc.wrap_paths(slots)
    keep = [x, y, last[0]]
    if cap_paths > 8:
        keep += list(last[1:]) + list(before) + list(pc.plain_collision_pairs()[0])
    ids = list(range(700, 700 + len(keep)))
    p = Pair(codec, cap_paths, keep + [b"/r/0/0", b"/r/3/1"])
    assert p.m.slots == slots and len(keep) == (3 if cap_paths == 8 else 11)
    p.ins(keep, ids)
    exact = set()
    for rnd, (n, rehash) in enumerate(sizes):
        lo, hi = p.m.used
        if lo == hi:
            exact.add(lo + n - p.m.thr)    # used is known: how far the call is from the threshold
        paths = [b"/r/%d/%d" % (rnd, i) for i in range(n)]
        p.ins(paths, [100 * rnd + i for i in range(n)], rehash=rehash)
        assert p.t.lookup(paths) == [100 * rnd + i for i in range(n)]
        p.rem(paths)
        assert p.t.lookup(keep) == ids     # the survivors, after every round
    assert p.m.rehashes >= 2 and {0, 1} <= exact, (p.m.rehashes, exact)


SEQ_BYTES = 1000  # cap_bytes of the sequence below: what its inserts ask for runs past it


def test_a_sequence_of_calls_against_the_model(codec):
    import netidx_amd
    rng = random.Random(77)
    last, before = pc.wrap_paths(64)
    uni = [q for g in collision_groups() for q in g] + list(pc.collision_triple())
    uni += list(pc.reserved_paths().values()) + list(last) + list(before)
    uni += list(pc.collision_pair_at(64, 63)) + [b"/seq/%d" % i for i in range(60 - len(uni) - 2)]
    assert len(uni) == len(set(uni)) == 60
    p = Pair(codec, 32, uni, cap_bytes=SEQ_BYTES)  # 64 slots
    next_id, refused, inserted = 1, {"paths": 0, "bytes": 0}, 0
    for call in range(44):
        if rng.random() < 0.6:
            paths = rng.sample(uni, rng.randrange(1, 9))
            if rng.random() < 0.4:
                paths += rng.sample(paths, 1)            # a duplicate inside the call
            ids = list(range(next_id, next_id + len(paths)))
            next_id += len(paths)
            if p.m.fits(paths):
                p.ins(paths, ids)
                inserted += 1
            else:
                refused["paths" if len(paths) > 32 - len(p.m.d) else "bytes"] += 1
                with pytest.raises(netidx_amd.CodecError, match="NXG_CAPACITY"):
                    p.t.insert(paths, ids)
                p.check()                                # nothing changed
        else:
            live = list(p.m.d)
            paths = rng.sample(live, min(len(live), rng.randrange(1, 12))) + rng.sample(uni, 2)
            if rng.random() < 0.5 and paths:
                paths += [paths[0]]                      # named twice: one finds it
            p.rem(paths)
    # the bytes ever inserted (duplicates and removed paths included) ran into cap_bytes
    assert inserted >= 12 and refused["bytes"] >= 2 and p.m.heap <= SEQ_BYTES, (inserted, refused)
    left = SEQ_BYTES - p.m.heap
    assert 0 < left and len(p.m.d) < 32
    with pytest.raises(netidx_amd.CodecError, match="NXG_CAPACITY"):
        p.t.insert([b"/" + b"z" * left], [9998])         # one byte more than is left
    p.check()
    p.universe.append(b"/" + b"z" * (left - 1))
    p.ins([p.universe[-1]], [9999])                      # exactly what is left
    with pytest.raises(netidx_amd.CodecError, match="NXG_CAPACITY"):
        p.t.insert([b"z"], [9997])
    p.check()

