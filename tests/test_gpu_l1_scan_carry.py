"""Every carry into the greedy scan, kernel against twin (run with -m gpu on the MI355X box).

The level-1 step gives the lanes that the last step's match still covers the map of a literal, and the scan's first three
stages take the upper dword of the shifted map from a constant of the lane (hd_device.hpp Fn8Ident, fn8_scan_state0).
Both rest on "state 0 enters lane 0, and a literal hands it on": the first live lane, lane c for a carry of c, must see
state 0 behind c covered lanes, wherever c falls in its row.  tests/test_gpu_l1_scan_rows.py carries at most 14 lanes
into a step; here it is every c = 1..63.

A block is 8192 seeded random bytes below 144, as there (8-bit literals in the static code; by themselves they hold next
to no match).  A copy of c + 4 bytes is planted at B - 4, its source 1500 bytes back: taken, it leaves the step at B with
a carry of c.  A second copy of 4..8 bytes (source 1700 back) starts exactly at lane c, B + c: the first live lane
starts a match, long enough to cross the next row seam (or the step's edge) wherever that lies within its eight bytes.
B = 2048 is a step of the group loop, B = N - 256 a step of the block's tail outside the groups: 126 blocks.

A plant the parse does not take tests nothing, so each block is checked on the CPU first, through the twin: the block
codes strictly smaller than the same block with either plant alone, and each of those smaller than the block without
plants (seeds are searched until it does: the 11-bit hash table keeps one position per entry).  No case is left out.

Then one launch per level (1, and 2, whose parse kernel runs the same scan) codes them all: kernel bytes == twin bytes,
the oracle inflates them back, and the CRC is the oracle's."""
import functools
import os

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

N = 8192
BACK = 1500
BACK2 = BACK + 200
BASES = [2048, N - 256]
CARRIES = range(1, 64)


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def _size(d):
    r, z = hdtest.oracle_twin(d.tobytes(), 1)
    assert r == 0
    return len(z)


def _second_length(c):
    """4..8 bytes, and past the next row seam (the step's edge behind row 3) where eight bytes reach it"""
    to_seam = 16 - c % 16
    return max(4, to_seam + 1) if to_seam < 8 else 4 + c % 5


def _build(rng, B, c):
    """[both plants, the first alone, the second alone, none], or None where the seed's bytes spoil a plant's edges"""
    L1, L2 = c + 4, _second_length(c)
    p1, p2 = B - 4, B + c
    base = rng.integers(0, 144, N, dtype=np.uint8)
    d = base.copy()
    d[p2:p2 + L2] = d[p2 - BACK2:p2 - BACK2 + L2]
    if d[p2 + L2] == d[p2 - BACK2 + L2]:
        d[p2 + L2] = (int(d[p2 + L2]) + 1) % 144
    only2 = d.copy()
    d[p1:p1 + L1] = d[p1 - BACK:p1 - BACK + L1]
    if d[p1 - 1] == d[p1 - BACK - 1]:
        d[p1 - 1] = (int(d[p1 - 1]) + 1) % 144
    only2[p1 - 1] = d[p1 - 1]
    only1 = d.copy()
    only1[p2:p2 + L2] = base[p2:p2 + L2]
    bare = base.copy()
    bare[p1 - 1], bare[p2 + L2] = d[p1 - 1], d[p2 + L2]
    # the first copy ends exactly at lane c: the byte behind it (the second plant's first, or the seed's own) differs
    # from the source's next; and the second copy is still whole behind the first
    nxt = d[p1 - BACK + L1]
    if d[p2] == nxt or only1[p2] == nxt or not np.array_equal(d[p2:p2 + L2], d[p2 - BACK2:p2 - BACK2 + L2]):
        return None
    return [d, only1, only2, bare]


def _searched(B, c):
    for k in range(400):
        blocks = _build(np.random.default_rng([B, c, k]), B, c)
        if blocks is None:
            continue
        both, only1, only2, bare = [_size(b) for b in blocks]
        if both < only1 < bare and both < only2 < bare and bare < N + 5:
            return blocks[0], (both, only1, only2, bare)
    raise AssertionError("no seed makes the parse take both plants of carry %d at %d" % (c, B))


@functools.lru_cache(maxsize=None)
def _blocks():
    """[(name, bytes, sizes)], every block checked through the twin: both plants taken"""
    out = []
    for B in BASES:
        for c in CARRIES:
            d, sizes = _searched(B, c)
            out.append(("carry/B%d/c%d" % (B, c), d.tobytes(), sizes))
    return out


def test_every_carry_is_realised():
    blocks = _blocks()
    assert [k for k, _, _ in blocks] == ["carry/B%d/c%d" % (B, c) for B in BASES for c in range(1, 64)]
    assert len(blocks) == 126
    for name, d, (both, only1, only2, bare) in blocks:
        assert len(d) == N
        assert both < only1 < bare and both < only2 < bare, (name, both, only1, only2, bare)
    for c in CARRIES:
        L2 = _second_length(c)
        assert 4 <= L2 <= 8
        if 16 - c % 16 < 8:
            assert c + L2 > 16 * (c // 16 + 1), c          # the first live lane's match crosses the seam


@pytest.mark.parametrize("level", [1, 2])
def test_scan_carries_match_twin(pkg, level):
    blocks = _blocks()
    blob = b"".join(d for _, d, _ in blocks)
    offs = [i * N for i in range(len(blocks))]
    lens = [N] * len(blocks)
    members, crc, st = pkg.batch_deflate(blob, offs, lens, level, pkg.FRAME_RAW)
    for i, (name, d, _) in enumerate(blocks):
        assert st[i] == 0, name
        r, twin = hdtest.oracle_twin(d, level)
        assert r == 0 and members[i] == twin, (name, level, len(members[i]), len(twin))
        r, back = hdtest.oracle_inflate(members[i], N)
        assert r == 0 and back == d, name
        assert int(crc[i]) == hdtest.oracle_crc32(d), name
