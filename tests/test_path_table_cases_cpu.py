"""CPU checks of tests/path_table_cases.py: its restatement of the path table's hash against the
library's nxg_path_hash, every property the crafted keys are built to have, and the sweep's
plain-ness rule against nxg_path_is_plain. No GPU."""
import random
import time

import netidx_amd
import path_table_cases as pc
import subscribe_route_model as sm


def test_the_restated_hash_is_the_librarys():
    rng = random.Random(41)
    for n in range(41):
        for off in range(8):
            p = rng.randbytes(n)
            assert netidx_amd.path_hash(p, off) == pc.path_hash(p), (n, off, p)
    for p in pc.all_crafted():
        for off in (0, 3):
            assert netidx_amd.path_hash(p, off) == pc.path_hash(p), (off, p)
    assert netidx_amd.path_hash(b"") == pc.path_hash(b"") == pc.stored(pc.finish_raw(pc.SEED))


def test_the_inverses_invert():
    rng = random.Random(42)
    for _ in range(200):
        h, w, s = rng.getrandbits(64), rng.getrandbits(64), rng.choice([29, 32])
        assert pc.mix(h, pc.word_for(h, w)) == w
        assert pc.finish_raw(pc.unfinish(h)) == h
        x = pc.unxorshift(h, s)
        assert x ^ (x >> s) == h


def test_collisions_share_a_hash_and_a_length_and_no_bytes():
    groups = list(pc.collision_pairs()) + [pc.collision_triple()] + list(pc.plain_collision_pairs())
    assert len(pc.collision_pairs()) >= 2 and len(pc.plain_collision_pairs()) >= 2
    for g in groups:
        assert len(set(g)) == len(g), g
        assert len({len(p) for p in g}) == 1 and len({pc.path_hash(p) for p in g}) == 1, g
        assert len({netidx_amd.path_hash(p) for p in g}) == 1, g
    c, d = pc.collision_pairs()[1]
    assert c[:8] == d[:8] and c[8:16] != d[8:16]  # they differ past the first word only
    assert len({pc.path_hash(g[0]) for g in groups}) == len(groups)  # and the groups are apart


def test_the_plain_collisions_are_plain_ascii():
    for pair in pc.plain_collision_pairs():
        for p in pair:
            assert netidx_amd.path_is_plain(p) and sm.is_plain(p) and pc.plain_rule(p), p
            assert p.startswith(b"/") and all(0x21 <= c < 0x7F for c in p), p


def test_the_reserved_paths_have_raw_hashes_0_to_3():
    r = pc.reserved_paths()
    assert sorted(r) == [0, 1, 2, 3] and len(set(r.values())) == 4
    for raw, p in r.items():
        assert len(p) == 8 and pc.raw_hash(p) == raw
        assert netidx_amd.path_hash(p) == (2, 3, 2, 3)[raw]


def test_the_chains_start_where_they_were_built_to():
    for slots in (16, 128):
        last, before = pc.wrap_paths(slots)
        assert len(set(last)) == 4 and len(set(before)) == 3
        for p in last:
            assert netidx_amd.path_hash(p) & (slots - 1) == slots - 1 and pc.plain_rule(p)
        for p in before:
            assert netidx_amd.path_hash(p) & (slots - 1) == slots - 2 and pc.plain_rule(p)
        x, y = pc.collision_pair_at(slots, slots - 1)
        assert x != y and len(x) == len(y) == 16
        assert netidx_amd.path_hash(x) == netidx_amd.path_hash(y) == pc.path_hash(x)
        assert pc.home_slot(x, slots) == slots - 1


def test_the_sweeps_rule_is_the_librarys():
    sw = pc.sweep()
    for p, plain in sw:
        assert netidx_amd.path_is_plain(p) is plain is sm.is_plain(p), p
    paths = {p for p, _ in sw}
    assert b"/" in paths and (b"/", True) in sw
    for n in pc.SWEEP_LENGTHS:
        c = pc.clean_path(n)
        assert len(c) == n and (c, True) in sw
        assert (c[:-1] + b"/", n == 1) in sw
        for i in range(n):
            assert (c[:i] + b"\\" + c[i + 1:], False) in sw
            if i + 1 < n:
                assert (c[:i] + b"//" + c[i + 2:], False) in sw
    # a lone `/` on either side of a word boundary stays plain
    c = pc.clean_path(17)
    for i in (7, 8, 15):
        assert (c[:i] + b"/" + c[i + 1:], True) in sw
    assert len(sw) <= 700


def test_building_every_case_is_quick():
    for f in (pc.collision_pairs, pc.collision_triple, pc.plain_collision_pairs, pc.reserved_paths,
              pc.chain_paths, pc.sweep):
        f.cache_clear()
    t0 = time.perf_counter()
    n = len(pc.all_crafted())
    dt = time.perf_counter() - t0
    assert n > 600 and dt < 2.0, (n, dt)
