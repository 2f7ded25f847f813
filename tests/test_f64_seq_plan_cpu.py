"""The grouping plan of a sequential-id backlog (plan_seq_backlog, netidx_amd/csrc/nxg_api.cpp),
through its debug entry point nxg_debug_f64s_plan. No GPU: the plan is a function of addresses
and lengths alone.

One launch of the backlog kernel runs its frames in backlog order in every wave, but no wave waits
for another, so a launch may hold two frames that touch the same memory in one case only: the same
id and fixed arrays, the same cap_rows and the same length (then the wave of a row is the same for
both, and the frame is marked `reuse`). Every other overlap, an empty frame, a frame of 256 MiB or
more and the 33rd frame start a new launch.
"""
import ctypes as C

import numpy as np

import netidx_amd

WREC = 256           # records per tile
KXCD = 256 << 20     # frames from here on keep the per-frame kernel
MB = 1 << 20


def plan(frames, waves=8192):
    """frames: (wire address, length, id address, fixed address, cap_rows) per frame.
    Returns (launches, start[], reuse[], tiles[])."""
    f = netidx_amd.lib().nxg_debug_f64s_plan
    f.restype = C.c_uint32
    n = len(frames)
    cols = [np.array([fr[k] for fr in frames], np.uint64) for k in range(5)]
    start, reuse = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    tiles = np.zeros(n, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    launches = f(C.c_uint32(n), p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), p(cols[4]),
                 C.c_uint32(waves), p(start), p(reuse), p(tiles))
    return launches, start.tolist(), reuse.tolist(), tiles.tolist()


def frame(k, length=13000, cols=None, cap=1000):
    """Frame k at an address of its own; columns `cols` (default: set k), 16 MiB apart."""
    c = k if cols is None else cols
    return (0x100000000 + k * 16 * MB, length, 0x800000000 + c * 16 * MB,
            0x800000000 + c * 16 * MB + 8 * MB, cap)


def expected_tiles(W, waves):
    t = -(-(W // 12 + 1) // WREC)
    return -(-t // waves)


def test_distinct_frames_share_launches_of_32():
    for n, want in ((1, 1), (2, 1), (3, 1), (32, 1), (33, 2), (40, 2), (64, 2), (65, 3)):
        launches, start, reuse, _ = plan([frame(k) for k in range(n)])
        assert launches == want, n
        assert [j for j in range(n) if start[j]] == list(range(0, n, 32)), n
        assert not any(reuse)


def test_empty_frame_cuts_before_and_behind():
    fr = [frame(0), frame(1), frame(2, length=0), frame(3), frame(4)]
    launches, start, reuse, tiles = plan(fr)
    assert (launches, start) == (2, [1, 0, 1, 1, 0])
    assert tiles[2] == 0 and all(tiles[j] > 0 for j in (0, 1, 3, 4))
    # only empty frames: nothing is launched
    assert plan([frame(0, length=0), frame(1, length=0)])[0] == 0


def test_long_frame_goes_alone():
    for length, alone in ((KXCD - 1, False), (KXCD, True), (KXCD + 1, True)):
        fr = [frame(0), (0x4000000000, length, 0x5000000000, 0x6000000000, length // 12 + 1),
              frame(2)]
        launches, start, _, tiles = plan(fr)
        assert start == ([1, 1, 1] if alone else [1, 0, 0]), length
        assert launches == (3 if alone else 1)
        assert (tiles[1] == 0) == alone


def test_wire_in_an_earlier_frames_columns_cuts():
    a = frame(0)
    id0, fx0, cap = a[2], a[3], a[4]
    for wire, cut in ((id0, True), (id0 + 8 * cap - 1, True), (id0 + 8 * cap, False),
                      (id0 - 13000, False), (id0 - 12999, True), (fx0 + 8, True)):
        b = (wire, 13000) + frame(1)[2:]
        launches, start, reuse, _ = plan([a, b])
        assert start == [1, int(cut)] and launches == 1 + cut, hex(wire)
        assert reuse == [0, 0]
    # ... of any earlier frame of the launch, not only the one before
    b = (fx0, 13000) + frame(2)[2:]
    assert plan([a, frame(1), b])[1] == [1, 0, 1]


def test_columns_over_an_earlier_frames_wire_cuts():
    a = frame(0)
    for idp, cut in ((a[0], True), (a[0] + a[1] - 1, True), (a[0] + a[1], False),
                     (a[0] - 8 * 1000, False), (a[0] - 8 * 1000 + 1, True)):
        b = frame(1)[:2] + (idp, frame(1)[3], 1000)
        assert plan([a, b])[1] == [1, int(cut)], hex(idp)
    b = frame(1)[:3] + (a[0] + 16, 1000)  # the fixed array
    assert plan([a, b])[1] == [1, 1]


def test_same_columns_and_length_stay_with_the_reuse_mark():
    # 7 frames into 3 column sets in rotation: one launch, frames 3.. marked
    fr = [frame(k, cols=k % 3) for k in range(7)]
    launches, start, reuse, tiles = plan(fr)
    assert (launches, start, reuse) == (1, [1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1, 1])
    assert len(set(tiles)) == 1
    # the bench's shape: 20 frames, 3 sets
    launches, start, reuse, _ = plan([frame(k % 3, cols=k % 3) for k in range(20)])
    assert launches == 1 and sum(start) == 1 and reuse == [0] * 3 + [1] * 17


def test_other_overlaps_of_columns_cut():
    a = frame(0, cols=0)
    same = frame(1, cols=0)
    assert plan([a, same])[1:3] == ([1, 0], [0, 1])
    other_len = frame(1, length=13013, cols=0)
    other_cap = frame(1, cols=0, cap=999)
    shifted = same[:2] + (same[2] + 128 * 8, same[3] + 128 * 8, 1000 - 128)
    other_fixed = same[:3] + (same[3] + 8, 1000)
    crossed = same[:2] + (same[3], same[2], 1000)  # id and fixed exchanged
    id_in_fixed = frame(1)[:3] + (a[2] + 800, 1000)  # its fixed array inside frame 0's id array
    for b in (other_len, other_cap, shifted, other_fixed, crossed, id_in_fixed):
        launches, start, reuse, _ = plan([a, b])
        assert (launches, start, reuse) == (2, [1, 1], [0, 0]), b
    # the frame whose columns are used again need not be the one before
    launches, start, reuse, _ = plan([a, frame(1, cols=1), shifted[:2] + frame(2, cols=1)[2:],
                                      frame(3, cols=0)])
    assert (start, reuse) == ([1, 0, 0, 0], [0, 0, 1, 1])
    launches, start, reuse, _ = plan([a, shifted, frame(2, cols=0)])
    # (frame 2 shares a launch with `shifted` only, and overlaps it)
    assert (launches, start, reuse) == (3, [1, 1, 1], [0, 0, 0])


def test_a_cut_forgets_the_frames_before_it():
    a, b = frame(0, cols=0), frame(1, length=13013, cols=0)
    launches, start, reuse, _ = plan([a, b, frame(2, cols=0), frame(3, length=13013, cols=0)])
    # frame 2 differs from frame 1 in length (cut); frame 3 from frame 2 (cut)
    assert (launches, start, reuse) == (4, [1, 1, 1, 1], [0, 0, 0, 0])
    launches, start, reuse, _ = plan([a, b, frame(2, length=13013, cols=0), frame(3, cols=1)])
    assert (launches, start, reuse) == (2, [1, 1, 0, 0], [0, 0, 1, 0])


def test_the_33rd_frame_cuts_with_reuse_too():
    fr = [frame(k % 3, cols=k % 3) for k in range(40)]
    launches, start, reuse, _ = plan(fr)
    assert launches == 2 and [j for j in range(40) if start[j]] == [0, 32]
    assert reuse == [0] * 3 + [1] * 29 + [0] * 3 + [1] * 5


def test_tiles_per_wave():
    for waves in (4, 8, 12, 6144, 8192):
        unit = 12 * WREC * waves  # bytes of one more tile for every wave, at 12 bytes a record
        for m in (1, 2, 3, 6):
            # W / 12 + 1 records at most: m tiles a wave below unit m bytes, m + 1 from there on
            for d, want in ((-13, m), (-12, m), (-1, m), (0, m + 1), (1, m + 1), (11, m + 1),
                            (12, m + 1)):
                W = unit * m + d
                _, _, _, tiles = plan([frame(0, length=W, cap=W // 12 + 1)], waves)
                assert tiles == [want], (waves, m, d)
    rng = np.random.default_rng(5)
    for W in [1, 11, 12, 13, 3071, 3072, 3073] + rng.integers(1, KXCD, 200).tolist():
        for waves in (4, 12, 8192):
            k = plan([frame(0, length=int(W))], waves)[3][0]
            assert k == expected_tiles(int(W), waves)
            # the waves' tiles cover every record the frame can hold, and no whole round is spare
            assert k * waves * WREC >= W // 12 + 1 > (k - 1) * waves * WREC
