"""Level 1's back end at its edges (run with -m gpu): the token queue held in a register and filled by a cross-lane push, and
the 64-dword staging ring that is emptied in front of every emit pass (hd_deflate_static.hpp).

The bar is the one of every encode test here: kernel bytes == CPU twin bytes (oracle/hd_deflate_twin.c), in every frame --
BGZF / MiGz / gzip / zlib / raw / raw-flush start the staging ring at 18 / 20 / 10 / 2 / 0 / 0 header bytes, i.e. at different
bit phases.  The inputs are planted where the new code has its corners:
  * bytes without matches whose static stream stays just under the stored size: 64 tokens in EVERY step, so a pass every step
    and a queue count that never moves -- and the same with a few nine-bit literals more, which walk the stream across the
    stored limit one bit at a time;
  * random bytes: the stored fallback, taken after dwords of the abandoned stream have already left for the slot;
  * runs of one byte: a token per 258 bytes, the queue count stays below 64 for many steps and the last pass is short;
  * far matches with long lengths: the widest codes, passes close to the 62 dwords the ring is sized for;
  * mixes of all of these, which walk the queue count through every residue;
  * blocks of 0, 1, 63, 64, 65, 0xff00 and 0x10000 bytes of each kind;
  * and a few thousand seeded FASTQ-like / text / random blocks in one launch.
The push itself (hd::queue_push: every queue count, masks from empty to full, the address wrap it leans on) is checked on
the device by hipdeflate_selftest()."""
import gzip
import os
import zlib

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 0xff00, 0x10000]
_POOLS = []            # FASTQ-like and text bytes the mixes cut their pieces from


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def _eight_bit_literals(rng, n, nine=0):
    """n bytes below 144 (eight-bit static codes), no byte pair repeated inside the window often enough to matter; `nine` of
    them replaced by bytes >= 144 (nine bits each)"""
    a = rng.integers(0, 144, n, dtype=np.uint8)
    if nine and n:
        a[rng.choice(n, size=min(nine, n), replace=False)] = rng.integers(144, 256, min(nine, n), dtype=np.uint8)
    return a.tobytes()


def _far_long_matches(rng, n):
    """a 3 KiB random head, then copies of 130..258 of its bytes from ~3000 back, a fresh byte between them: length codes with
    five extra bits, distance codes with ten"""
    out = bytearray(rng.integers(0, 256, 3000, dtype=np.uint8).tobytes())
    while len(out) < n:
        ln = int(rng.integers(130, 259))
        o = len(out) - 3000 + int(rng.integers(0, 200))
        out += out[o:o + ln]
        out.append(int(rng.integers(0, 256)))
    return bytes(out[:n])


def _mix(rng, n):
    """pieces of every kind, a few to a few hundred bytes each: the tokens per step go from 1 to 64 and back"""
    if not _POOLS:
        s = hdtest.synth()
        _POOLS.extend([bytes(s.fastq_like(200000, seed=21)), bytes(s.text_like(200000, seed=22))])
    fq, tx = _POOLS
    out = bytearray()
    while len(out) < n:
        k, ln = int(rng.integers(0, 6)), int(rng.integers(3, 400))
        if k == 0:
            out += _eight_bit_literals(rng, ln)
        elif k == 1:
            out += bytes([int(rng.integers(0, 256))]) * (ln * 3)
        elif k == 2:
            out += rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        elif k == 3 and len(out) > 600:
            o = len(out) - int(rng.integers(300, min(len(out), 4000)))
            out += out[o:o + ln]
        elif k == 4:
            o = int(rng.integers(0, len(fq) - ln))
            out += fq[o:o + ln]
        else:
            o = int(rng.integers(0, len(tx) - ln))
            out += tx[o:o + ln]
    return bytes(out[:n])


def planted_blocks():
    rng = np.random.default_rng(20251)
    blocks = []
    for n in SIZES:
        blocks.append(("lit8/%d" % n, _eight_bit_literals(rng, n)))
        blocks.append(("random/%d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        blocks.append(("run/%d" % n, b"A" * n))
        blocks.append(("far/%d" % n, _far_long_matches(rng, n) if n > 3000 else _mix(rng, n)))
        blocks.append(("mix/%d" % n, _mix(rng, n)))
    # the stored limit, crossed a bit at a time: static = 3 + 8 n + nine + 7 bits against stored = n + 5 bytes
    for nine in list(range(0, 40)) + [100, 1000]:
        blocks.append(("lit8+%d" % nine, _eight_bit_literals(rng, 0xff00, nine)))
        blocks.append(("lit8+%d/4000" % nine, _eight_bit_literals(rng, 4000 + nine, nine)))
    # runs that end inside a step, and queue counts of every residue at the block's end
    for n in range(258 * 3, 258 * 3 + 70, 3):
        blocks.append(("run/%d" % n, b"\x00" * n))
    for n in range(1, 130):
        blocks.append(("lit8/%d" % n, _eight_bit_literals(rng, n)))
        blocks.append(("mix/%d" % (5000 + 37 * n), _mix(rng, 5000 + 37 * n)))
    return blocks


def _launch(pkg, blocks, frame, slot):
    blob, offs, lens = bytearray(), [], []
    for b in blocks:
        offs.append(len(blob))
        lens.append(len(b))
        blob += b + bytes(-len(b) % 16)
    return pkg.batch_deflate(bytes(blob), offs, lens, 1, frame, slot=slot)


def _check_member(pkg, frame, hdr, trl, name, b, m, st, crc, room):
    twin_fn = hdtest.oracle_twin_flush if frame == pkg.FRAME_RAW_FLUSH else hdtest.oracle_twin
    r, twin = twin_fn(b, 1, cap=room - hdr - trl)
    assert (st == 0) == (r == 0), (name, frame, st, r)
    if r:
        return
    assert m[hdr:len(m) - trl] == twin, (name, frame, len(m), len(twin))
    assert int(crc) == zlib.crc32(b), (name, frame)
    if frame == pkg.FRAME_BGZF:
        assert int.from_bytes(m[16:18], "little") == len(m) - 1 and gzip.decompress(m) == b, (name, frame)
    elif frame == pkg.FRAME_MIGZ:
        assert int.from_bytes(m[16:20], "little") == len(m) - 28 and gzip.decompress(m) == b, (name, frame)
    elif frame == pkg.FRAME_GZIP:
        assert gzip.decompress(m) == b, (name, frame)
    elif frame == pkg.FRAME_ZLIB:
        assert zlib.decompress(m) == b, (name, frame)
    elif frame == pkg.FRAME_RAW:
        assert zlib.decompress(m, -15) == b, (name, frame)


def test_cross_lane_push_on_the_device(pkg):
    assert pkg.lib().hipdeflate_selftest() == 0


@pytest.mark.parametrize("frame,hdr,trl", [("BGZF", 18, 8), ("MIGZ", 20, 8), ("GZIP", 10, 8), ("ZLIB", 2, 4), ("RAW", 0, 0),
                                           ("RAW_FLUSH", 0, 0)])
def test_level1_planted_blocks_match_twin_in_every_frame(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    blocks = planted_blocks()
    # BGZF members end at 65536 bytes whatever the slot; the other frames get room for the stored form of 0x10000 bytes
    slot = 65536 if frame == "BGZF" else (int(pkg.lib().hipdeflate_bound(0x10000, 1)) + 15) // 16 * 16
    members, crc, st = _launch(pkg, [b for _, b in blocks], fr, slot)
    stored = 0
    for i, (name, b) in enumerate(blocks):
        _check_member(pkg, fr, hdr, trl, name, b, members[i], int(st[i]), crc[i], slot)
        stored += int(st[i]) == 0 and len(members[i]) - hdr - trl >= len(b) + 5
    assert stored >= 10          # (the stored fallback was among them)


@pytest.mark.parametrize("frame,hdr,trl", [("BGZF", 18, 8), ("RAW", 0, 0)])
def test_level1_three_thousand_seeded_blocks_in_one_launch(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    s = hdtest.synth()
    rng = np.random.default_rng(77)
    pools = [bytes(s.fastq_like(1 << 20, seed=11)), bytes(s.fastq_like(1 << 20, seed=12, first_record=0)),
             bytes(s.text_like(1 << 20, seed=13)), bytes(s.random_bytes(1 << 18, seed=14))]
    blocks = []
    for i in range(3000):
        pool = pools[int(rng.integers(0, 4)) if i % 8 else 3]
        # mostly a few KiB, every 16th a full BGZF block
        n = 0xff00 if i % 16 == 0 else int(rng.integers(1, 12000))
        o = int(rng.integers(0, len(pool) - n))
        blocks.append(pool[o:o + n])
    members, crc, st = _launch(pkg, blocks, fr, 65536)
    for i, b in enumerate(blocks):
        _check_member(pkg, fr, hdr, trl, "seeded/%d" % i, b, members[i], int(st[i]), crc[i], 65536)
