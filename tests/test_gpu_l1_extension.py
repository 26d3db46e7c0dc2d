"""Level 1's long matches at the edges of a step: the cooperative extension of a match whose first eight bytes agree, the
re-threading of the parse behind it, and the token queue that takes what the step made -- the code the level-1 step hands
from one step to the next (hd_deflate_static.hpp).

The bar of the GPU tests is the one of every encode test here: kernel bytes == CPU twin bytes (oracle/hd_deflate_twin.c), in
all six frames.  That only says something where the member is a static-Huffman block whose tokens carry the planted match, so
the inputs are built for it and test_planted_inputs_cover_the_cases (no GPU) holds them to it on the twin: every planted block
comes out as ONE static block (BTYPE 1) with a match of the planted length and distance at the planted position.
  * The filler is random bytes below 144: eight-bit static codes, so a block of literals stays under its stored size, and a
    four-byte repeat inside the window is rare.  The 1536-entry table is direct-mapped, so a candidate lives only until another
    position hashes to its slot: near sources lie a few hundred bytes back, far ones behind a run of one byte (one slot for
    all of it); a block whose planted match the twin does not take (a slot was overwritten all the same, or a stray repeat
    covers the spot) is built again from the next seed.
  * matches of every length 8..20 and of 63, 64, 65 and 258 bytes, starting at every lane 40..63 of a step inside a 16-step
    group, so that the first mismatch falls before, on and behind lane 63; every third lane also in one of the block's last
    steps, which run one at a time with the end-of-block tests compiled in;
  * distances 1..8, where the source overlaps the match.  A lane's candidate was published by an EARLIER step, so a token's
    distance exceeds its lane: these start at lanes 0 and d - 1, every length;
  * the far edge: 2700 bytes back, about as far as the window reaches at every step of a group (the ring is filled up to
    1344 bytes ahead of the step), found and asserted; and 4095 back, the nominal edge, which the ring never reaches (it is filled at
    least 384 bytes ahead of the step, so a candidate lies at most ~3700 back): the twin takes none of them, and the kernel
    must not either (asserted: a static block, and the kernel's bytes are the twin's);
  * the same matches cut short by the end of the block, a few bytes and many bytes in;
  * at least three matches longer than eight bytes back to back in one step;
  * and three thousand seeded FASTQ-like and text blocks in every launch.
Every launch must leave hipdeflate_stall_count() at 0 and give every member status 0."""
import gzip
import os
import zlib

import numpy as np
import pytest

import deflate_tokens
import hdtest

LENGTHS = list(range(8, 21)) + [63, 64, 65, 258]
LANES = list(range(40, 64))
NEAR = 200
FAR = 2700
EDGE = 4095
FRAMES = [("BGZF", 18, 8), ("MIGZ", 20, 8), ("GZIP", 10, 8), ("ZLIB", 2, 4), ("RAW", 0, 0), ("RAW_FLUSH", 0, 0)]
SLOT = 65536
GROUP_STEP = 1088        # a step in the middle of a 16-step group (the ring is refilled at S = 704 + 1024 k)
LATE_STEP = 4160         # ... and one three refills on, for the far sources


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def _filler(rng, n):
    return bytearray(rng.integers(0, 144, n, dtype=np.uint8).tobytes())


def _plant(out, dist, length):
    """append `length` bytes copied from `dist` back (byte by byte: the source may overlap), then one byte that ends the match"""
    for _ in range(length):
        out.append(out[-dist])
    out.append((out[-dist] + 1) % 144)


def _twin_tokens(b):
    r, twin = hdtest.oracle_twin(b, 1, cap=SLOT)
    assert r == 0
    st = deflate_tokens.read(twin, expand=False)
    return st.blocks


def _has(blocks, pos, length, dist):
    return len(blocks) == 1 and blocks[0].kind == "static" and (pos, length, dist) in blocks[0].matches()


def _build(seed, make):
    """make(rng) -> (bytes, expected (pos, length, dist) or a predicate on the twin's blocks); the first seed the twin agrees with"""
    for attempt in range(200):
        b, want = make(np.random.default_rng([seed, attempt]))
        blocks = _twin_tokens(b)
        if (want(blocks) if callable(want) else _has(blocks, *want)):
            return b, want
    raise AssertionError("no seed gives the planted tokens")


def _with_source(rng, start, dist):
    """filler up to `start` with the source `dist` back; a far source lies behind a run of one byte, which takes one table slot"""
    if dist <= 1000:
        return _filler(rng, start)
    out = _filler(rng, start - dist + 300)
    out += bytes([143]) * (dist - 300 - 70)
    out += _filler(rng, 70)
    assert len(out) == start
    return out


def match_block(lane, length, dist, step, clip=None, tail=1400):
    def make(rng):
        start = step + lane
        out = _with_source(rng, start, dist)
        _plant(out, dist, 300 if clip is not None else length)
        if clip is not None:
            return bytes(out[:start + clip]), (start, clip, dist)
        out += _filler(rng, tail if tail is not None else int(rng.integers(0, 70)))
        return bytes(out), (start, length, dist)
    return make


def edge_block(lane, length):
    """the source 4095 back: past the window's reach at most steps, so the twin says what becomes of it"""
    def make(rng):
        out = _with_source(rng, LATE_STEP + lane, EDGE)
        _plant(out, EDGE, length)
        out += _filler(rng, 1400)
        return bytes(out), (lambda blocks: len(blocks) == 1 and blocks[0].kind == "static")
    return make


def _chain_ok(blocks):
    if len(blocks) != 1 or blocks[0].kind != "static":
        return False
    m = [x for x in blocks[0].matches() if x[1] > 8]
    for i in range(len(m) - 2):
        a, b, c = m[i], m[i + 1], m[i + 2]
        if a[0] + a[1] == b[0] and b[0] + b[1] == c[0] and a[0] // 64 == c[0] // 64:
            return True
    return False


def chain_block(rng0):
    def make(rng):
        out = _filler(rng, GROUP_STEP + int(rng.integers(0, 20)))
        src = len(out) - 320                     # pieces of the 300 bytes in front, one straight behind the other
        end = len(out) + 150
        while len(out) < end:
            ln = int(rng.integers(9, 22))
            o = src + int(rng.integers(0, 300 - ln))
            out += out[o:o + ln]
        out += _filler(rng, 1400)
        return bytes(out), _chain_ok
    return make


def planted_specs():
    """(name, make) of every planted block"""
    specs = []
    for dist in (NEAR, FAR):
        step = GROUP_STEP if dist == NEAR else LATE_STEP
        for lane in LANES:
            for length in LENGTHS:
                specs.append(("match/d%d/l%d/n%d" % (dist, lane, length), match_block(lane, length, dist, step)))
            for clip in sorted({8, 9, 20, 64 - lane + 4, 65 - lane + 8, 100, 257}):
                specs.append(("clip/d%d/l%d/c%d" % (dist, lane, clip), match_block(lane, 0, dist, step, clip=clip)))
        for lane in LANES[::3]:
            for length in LENGTHS:
                specs.append(("end/d%d/l%d/n%d" % (dist, lane, length), match_block(lane, length, dist, LATE_STEP, tail=None)))
    for dist in range(1, 9):
        for lane in sorted({0, dist - 1}):
            for length in LENGTHS:
                specs.append(("near/d%d/l%d/n%d" % (dist, lane, length), match_block(lane, length, dist, GROUP_STEP)))
            for clip in (8, 9, 64, 100):
                specs.append(("nearclip/d%d/l%d/c%d" % (dist, lane, clip), match_block(lane, 0, dist, GROUP_STEP, clip=clip)))
    for lane in LANES[::3]:
        for length in LENGTHS:
            specs.append(("edge/l%d/n%d" % (lane, length), edge_block(lane, length)))
    for i in range(60):
        specs.append(("chain/%d" % i, chain_block(i)))
    return specs


_PLANTED = []


def planted_blocks():
    """(name, bytes, what the twin must make of it)"""
    if not _PLANTED:
        for i, (name, make) in enumerate(planted_specs()):
            b, want = _build(i, make)
            _PLANTED.append((name, b, want))
    return _PLANTED


def seeded_blocks():
    s = hdtest.synth()
    rng = np.random.default_rng(7042)
    pools = [bytes(s.fastq_like(1 << 20, seed=31)), bytes(s.fastq_like(1 << 20, seed=32, first_record=0)),
             bytes(s.text_like(1 << 20, seed=33)), bytes(s.text_like(1 << 20, seed=34))]
    blocks = []
    for i in range(3000):
        pool = pools[int(rng.integers(0, 4))]
        n = 0xff00 if i % 16 == 0 else int(rng.integers(1, 12000))
        o = int(rng.integers(0, len(pool) - n))
        blocks.append(("seeded/%d" % i, pool[o:o + n]))
    return blocks


_BLOCKS = []


def all_blocks():
    if not _BLOCKS:
        _BLOCKS.extend([(n, b) for n, b, _ in planted_blocks()] + seeded_blocks())
    return _BLOCKS


def _launch(pkg, blocks, frame):
    blob, offs, lens = bytearray(), [], []
    for b in blocks:
        offs.append(len(blob))
        lens.append(len(b))
        blob += b + bytes(-len(b) % 16)
    return pkg.batch_deflate(bytes(blob), offs, lens, 1, frame, slot=SLOT)


def test_planted_inputs_cover_the_cases():
    """no GPU: the twin's stream of every planted block is one static block that holds the planted token"""
    blocks = planted_blocks()
    names = {n for n, _, _ in blocks}
    for dist in (NEAR, FAR):
        for lane in LANES:
            for length in LENGTHS:
                assert "match/d%d/l%d/n%d" % (dist, lane, length) in names
    for dist in range(1, 9):
        for length in LENGTHS:
            assert "near/d%d/l%d/n%d" % (dist, dist - 1, length) in names
    found_edge = 0
    for name, b, want in blocks:
        r, twin = hdtest.oracle_twin(b, 1, cap=SLOT)
        assert r == 0, name
        st = deflate_tokens.read(twin)
        assert bytes(st.out) == b, name
        assert len(st.blocks) == 1 and st.blocks[0].kind == "static", (name, [x.kind for x in st.blocks])
        if callable(want):
            assert want(st.blocks), name
            found_edge += name.startswith("edge/") and any(d == EDGE for _, _, d in st.blocks[0].matches())
        else:
            pos, length, dist = want
            assert (pos, length, dist) in st.blocks[0].matches(), (name, want)
            kind, lane = name.split("/")[0], int(name.split("/")[2][1:])
            assert pos % 64 == lane and (kind in ("near", "nearclip") or 40 <= lane <= 63), name
            if kind in ("clip", "nearclip"):
                assert pos + length == len(b), name           # cut by n
            else:
                assert b[pos + length] != b[pos + length - dist], name
    print("edge blocks whose 4095-byte match the twin takes: %d" % found_edge)


@pytest.mark.gpu
@pytest.mark.parametrize("frame,hdr,trl", FRAMES)
def test_level1_matches_across_the_step_edge_match_twin(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    blocks = all_blocks()
    assert sum(1 for n, _ in blocks if n.startswith("seeded/")) == 3000
    members, crc, st = _launch(pkg, [b for _, b in blocks], fr)
    assert pkg.lib().hipdeflate_stall_count() == 0
    twin_fn = hdtest.oracle_twin_flush if fr == pkg.FRAME_RAW_FLUSH else hdtest.oracle_twin
    for i, (name, b) in enumerate(blocks):
        m = members[i]
        assert int(st[i]) == 0, (name, frame, int(st[i]))
        r, twin = twin_fn(b, 1, cap=SLOT - hdr - trl)
        assert r == 0, (name, frame, r)
        assert m[hdr:len(m) - trl] == twin, (name, frame, len(m), len(twin))
        assert int(crc[i]) == zlib.crc32(b), (name, frame)
        if frame in ("BGZF", "MIGZ", "GZIP"):
            assert gzip.decompress(m) == b, (name, frame)
        elif frame == "ZLIB":
            assert zlib.decompress(m) == b, (name, frame)
        elif frame == "RAW":
            assert zlib.decompress(m, -15) == b, (name, frame)
