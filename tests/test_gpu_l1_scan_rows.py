"""The greedy scan's seams, kernel against twin (run with -m gpu on the MI355X box).

The level-1 step resolves the greedy parse of its 64 positions with a six-stage DPP scan over the lanes
(hd_device.hpp fn8_scan_state0): four stages inside a row of 16 lanes, two across the rows, whose shifted rows are written
straight into the registers that hold the stages' identity constants, and the carry of the step before in front of it.
A wrong row in one of those registers, or a start mask shifted the wrong way, shows only where the automaton crosses a
row seam (or the step's edge) in a state other than 0 -- inside a match that began on the other side.

So the blocks here are built to put every state across every seam.  A block is 8192 seeded random bytes below 144 (such
bytes are 8-bit literals in the static code, so the stream stays under the stored size and the block is coded, not
stored; by themselves they hold next to no match).  ONE copy of an earlier phrase of L = 3..8 bytes is planted at B - j,
j = 1..L-1, its source 1500 bytes back, a differing byte behind it and in front of it: the automaton crosses B in state
L - j.  B is a step boundary (2048: the carry) and the three row seams of that step (2064, 2080, 2096) inside a
16-step group, and the same four offsets in a step of the block's tail outside the groups, n - 256 + 16 r.  A second set
plants two such copies back to back across the seam, a third plants phrases of 9..15 bytes out of hdtest.corpus_phrases
(the capped matches: the long-match events and their re-threading) at the same seams.

A plant the parse does not take tests nothing, so the blocks are checked on the CPU first, through the twin: every
planted block codes smaller than the same block without its plant (seeds are searched until it does -- the 11-bit hash
table keeps one position per entry, and 1500 positions later about six in ten entries have been taken over).  L = 3 is
below the minimum match of every level (HD_MIN_MATCH = 4): those blocks are the near miss at the seam, three equal bytes
and a differing one, and must code to exactly the size of the block without them.

Then one launch per level (1, and 2, whose parse kernel runs the same scan) codes them all: kernel bytes == twin bytes,
and the oracle inflates them back."""
import functools
import os

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

N = 8192
BACK = 1500
SEAMS = [2048 + 16 * r for r in range(4)] + [N - 256 + 16 * r for r in range(4)]


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


def _copy(d, p, length, back, phrase=None):
    """d[p:p+length] becomes a copy of d[p-back:...] (of `phrase`, written there first), the bytes around it differ"""
    if phrase is not None:
        d[p - back:p - back + length] = phrase
    d[p:p + length] = d[p - back:p - back + length]
    if d[p + length] == d[p - back + length]:
        d[p + length] = (int(d[p + length]) + 1) % 144
    if d[p - 1] == d[p - back - 1]:
        d[p - 1] = (int(d[p - 1]) + 1) % 144


def _searched(case, build):
    """build(rng) -> the list of blocks [whole plant, ..., no plant] of one case, each a step less planted than the one in
    front of it; the first seed whose sizes fall strictly along the list (three-byte plants: stay equal) is taken"""
    for k in range(200):
        rng = np.random.default_rng([case, k])
        blocks = build(rng)
        sizes = [_size(b) for b in blocks]
        if all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < N + 5:
            return blocks[0], sizes
    raise AssertionError("no seed makes the parse take the plant of case %r" % (case,))


@functools.lru_cache(maxsize=None)
def _blocks():
    """[(name, bytes)], every block checked through the twin: planted and taken"""
    out = []
    words = np.frombuffer(b"".join(hdtest.corpus_phrases(4100, 6)), dtype=np.uint8) % 144
    case = 0
    for si, B in enumerate(SEAMS):
        # one plant of 3..8 bytes, every state across the seam
        for L in range(3, 9):
            for j in range(1, L):
                case += 1
                if L < 4:                                  # below HD_MIN_MATCH: the near miss
                    rng = np.random.default_rng([case, 0])
                    d = rng.integers(0, 144, N, dtype=np.uint8)
                    bare = d.copy()
                    _copy(d, B - j, L, BACK)
                    bare[B - j - 1], bare[B - j + L] = d[B - j - 1], d[B - j + L]
                    assert _size(d) == _size(bare), ("a three-byte repeat is no match", B, L, j)
                    out.append(("one/B%d/L%d/j%d" % (B, L, j), d.tobytes()))
                    continue

                def one(rng, B=B, L=L, j=j):
                    d = rng.integers(0, 144, N, dtype=np.uint8)
                    bare = d.copy()
                    _copy(d, B - j, L, BACK)
                    bare[B - j - 1], bare[B - j + L] = d[B - j - 1], d[B - j + L]
                    return [d, bare]
                d, sizes = _searched(case, one)
                out.append(("one/B%d/L%d/j%d" % (B, L, j), d.tobytes()))
        # two plants back to back: the seam inside the first, the second starts where the first ends
        for L1 in range(4, 9):
            for j in range(1, L1):
                case += 1
                L2 = 4 + (L1 + j + si) % 5

                def two(rng, B=B, L1=L1, L2=L2, j=j):
                    d = rng.integers(0, 144, N, dtype=np.uint8)
                    bare = d.copy()
                    p1, p2 = B - j, B - j + L1
                    _copy(d, p2, L2, BACK + 200)
                    first_missing = d.copy()
                    _copy(d, p1, L1, BACK)
                    # (the first copy's end byte is the second's first: it differs from the first source's next byte or the seed is passed over)
                    if d[p2] == d[p1 - BACK + L1] or not np.array_equal(d[p2:p2 + L2], d[p2 - BACK - 200:p2 - BACK - 200 + L2]):
                        return [d, d]
                    first_missing[p1 - 1] = d[p1 - 1]
                    bare[p1 - 1], bare[p2 + L2], bare[p2 - 1] = d[p1 - 1], d[p2 + L2], first_missing[p2 - 1]
                    return [d, first_missing, bare]
                d, sizes = _searched(case, two)
                out.append(("two/B%d/L%d+%d/j%d" % (B, L1, L2, j), d.tobytes()))
        # capped matches: dictionary phrases of 9..15 bytes
        for L in range(9, 16):
            for j in sorted({1, 4, 8, L - 1}):
                case += 1

                def long(rng, B=B, L=L, j=j):
                    d = rng.integers(0, 144, N, dtype=np.uint8)
                    w = int(rng.integers(0, len(words) - L))
                    bare = d.copy()
                    _copy(d, B - j, L, BACK, phrase=words[w:w + L])
                    bare[B - j - BACK:B - j - BACK + L] = words[w:w + L]
                    bare[B - j - 1], bare[B - j + L] = d[B - j - 1], d[B - j + L]
                    return [d, bare]
                d, sizes = _searched(case, long)
                out.append(("phrase/B%d/L%d/j%d" % (B, L, j), d.tobytes()))
    return out


def test_every_plant_is_taken_by_the_parse():
    """(the construction asserts it block by block; here: the sets are whole)"""
    names = [k for k, _ in _blocks()]
    assert len(names) == len(set(names)) == 8 * (27 + 25 + sum(len({1, 4, 8, L - 1}) for L in range(9, 16)))


@pytest.mark.parametrize("level", [1, 2])
def test_scan_seams_match_twin(pkg, level):
    blocks = _blocks()
    blob = b"".join(d for _, d in blocks)
    offs = [i * N for i in range(len(blocks))]
    lens = [N] * len(blocks)
    members, crc, st = pkg.batch_deflate(blob, offs, lens, level, pkg.FRAME_RAW)
    for i, (name, d) in enumerate(blocks):
        assert st[i] == 0, name
        r, twin = hdtest.oracle_twin(d, level)
        assert r == 0 and members[i] == twin, (name, level, len(members[i]), len(twin))
        r, back = hdtest.oracle_inflate(members[i], N)
        assert r == 0 and back == d, name
        assert int(crc[i]) == hdtest.oracle_crc32(d), name
