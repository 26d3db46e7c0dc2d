"""Level 1 deep inside its 16-step groups: the edge of the condition a group is entered on, the longest matches, several
long matches per step and the stream that is given up on the way (hd_deflate_static.hpp: the group loop, the long-match
loop of the step, emit_tokens and the drain it is wrapped round).

The bar is the one of test_gpu_l1_extension.py, whose builders these inputs are made with: kernel bytes == CPU twin bytes
(oracle/hd_deflate_twin.c, hdo_deflate_twin) in all six frames, a few hundred blocks of 2..12 KiB in one launch; and
test_planted_inputs_cover_the_cases (no GPU) holds every planted block to what it is planted for, on the twin.

  * group edge.  A group of 16 steps starts at Sg = 704 + 1024 k.  It is entered only where every lane of its last step
    has a full match length ahead (Sg + 15 * 64 + 63 + 258 <= n, i.e. n >= Sg + 1281), so that the long-match loop's
    `maxlen` is the constant 258 there; the parent commit entered it from n >= Sg + 1160 on and clipped per match.  Block
    lengths Sg + {1159, 1160, 1161, 1280, 1281, 1282} for Sg = 704, 1728, 2752 stand on both edges.  The last 400 bytes
    copy an earlier span at distance 9, 300 and 3000 (where the block is shorter than that in front of its tail: at the
    largest distance it has, the tail's own offset), so matches start in each of the last five steps of the would-be group
    and run into the block's end: a group entered too early does not clip them, a general step must.
  * long matches of exactly 258, 259, 516 and 600 bytes starting at lanes 0, 31, 62 and 63 of a step deep inside a group,
    at distance 8 (which a lane beyond 7 cannot see: there the copy is taken from the next step's first lane on), 64, 3700
    and the largest the window admits at that step (the ring holds 2752 + 64 k + lane bytes behind
    lane `lane` of a group's step k: 3712 + lane in its last step, where these stand); and the same lengths with the match
    itself or its source lying across a multiple of 4096, where the ring wraps.
  * several long matches in a step: phrases of 9..12 and of 16..20 bytes copied at spacings that put two to six long
    starts into one step of a group -- the bookkeeping of the lanes still to be handled (`todo`) -- and a pair A, B laid out
    so that the eight-byte parse jumps OVER the start of B: the walk behind A's extension lands on a lane that was no
    start before, whose own match is long, so the fresh start is the next event.
  * the abandoned stream: 4 KiB that code at eight bits a byte, then bytes that take nine, until the static stream
    passes the stored size in a pass whose drained dwords have just left; the reverse order; the member is the twin's
    stored one.  And slot-limited launches (tests/encode_room.py: the room one below, at and one above what the member
    needs), where the stream is given up against the slot instead and the member is refused or the twin's."""
import gzip
import os
import zlib

import numpy as np
import pytest

import deflate_tokens
import encode_room as er
import hdtest
import test_gpu_encode_room as room
import test_gpu_l1_extension as ext

FRAMES, SLOT = ext.FRAMES, ext.SLOT
GROUPS = (704, 1728, 2752)
EDGE_LENGTHS = (1159, 1160, 1161, 1280, 1281, 1282)
TAIL = 400
LONG_LENGTHS = (258, 259, 516, 600)
LONG_LANES = (0, 31, 62, 63)
LAST_STEP = 3776 + 15 * 64           # step 15 of the group that starts at 704 + 3 * 1024
MID_STEP = 3776 + 7 * 64


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def _static(blocks):
    return len(blocks) == 1 and blocks[0].kind == "static"


# ---- group edge --------------------------------------------------------------------------------------------------

def edge_block(sg, extra, dist):
    n = sg + extra
    start = n - TAIL
    d = min(dist, start)

    def make(rng):
        out = ext._with_source(rng, start, d) if d == dist else ext._filler(rng, start)
        for _ in range(TAIL):
            out.append(out[-d])

        def want(blocks):
            if not _static(blocks):
                return False
            m = [x for x in blocks[0].matches() if x[2] == d and x[0] >= start]
            steps = {x[0] // 64 for x in m}
            # the copy is taken from its first bytes on, piece by piece up to the block's end, which the last piece reaches
            return bool(m) and m[0][0] <= start + 16 and sum(x[1] for x in m) >= TAIL - 32 and m[-1][0] + m[-1][1] == n \
                and max(x[1] for x in m) > 8 and (d < 100 or len(steps) >= 2)
        return bytes(out), want
    return make, n, d


def edge_specs():
    specs = []
    for sg in GROUPS:
        for extra in EDGE_LENGTHS:
            for dist in (9, 300, 3000):
                make, n, d = edge_block(sg, extra, dist)
                specs.append(("edge/g%d/n%d/d%d" % (sg, n, d), make))
    return specs


# ---- long matches ------------------------------------------------------------------------------------------------

def window_reach(step, lane):
    """the largest distance lane `lane` of `step` can match at: the ring is refilled to Sg + 1344 at the group's start Sg
    and holds the 4096 bytes below that"""
    sg = 704 + (step - 704) // 1024 * 1024
    return (step + lane) - (sg + 1344 - 4096)


def long_block(lane, length, dist, step):
    def make(rng):
        start = step + lane
        out = ext._with_source(rng, start, dist)
        ext._plant(out, dist, length)
        out += ext._filler(rng, 1400)
        first = min(length, 258)

        def want(blocks):
            if not _static(blocks):
                return False
            if dist <= lane:
                # (a lane's candidate was published by an EARLIER step, so a token's distance exceeds its lane: this copy
                # is found from the next step's first lane on, and is long from there)
                return any(d == dist and start < p <= start + 64 and (ln == 258 or p + ln == start + length)
                           for p, ln, d in blocks[0].matches())
            if (start, first, dist) not in blocks[0].matches():
                return False
            # the rest of a longer copy follows in tokens that end where the copy ends
            ends = {p + ln for p, ln, _ in blocks[0].matches()}
            return length == first or start + length in ends or length - first < 4
        return bytes(out), want
    return make


def long_specs():
    specs = []
    for lane in LONG_LANES:
        for length in LONG_LENGTHS:
            for dist in (8, 64, 3700, window_reach(LAST_STEP, lane)):
                specs.append(("long/l%d/n%d/d%d" % (lane, length, dist), long_block(lane, length, dist, LAST_STEP)))
            # the match lies across 4096 (positions 4030 + ... in step 3 of the group at 3776) ...
            for dist in (8, 64, window_reach(3968, lane)):
                specs.append(("wrapdst/l%d/n%d/d%d" % (lane, length, dist), long_block(lane, length, dist, 3968)))
            # ... or its source does: it starts 100 below 4096, the match in step 8 of the group at 5824
            specs.append(("wrapsrc/l%d/n%d" % (lane, length), long_block(lane, length, 6336 + lane - 3996, 6336)))
    return specs


# ---- several long matches per step -------------------------------------------------------------------------------

def _long_starts_by_step(blocks):
    by = {}
    for p, ln, _ in blocks[0].matches():
        if ln > 8:
            by[p // 64] = by.get(p // 64, 0) + 1
    return by


def phrase_block(lengths, count):
    """phrases of the given lengths, cut from the 300 bytes in front, `count` of them spread over each 64-byte step"""
    def make(rng):
        out = ext._filler(rng, MID_STEP - 64 + int(rng.integers(0, 8)))
        src = len(out) - 320
        end = len(out) + 4 * 64
        while len(out) < end:
            ln = int(rng.choice(lengths))
            o = src + int(rng.integers(0, 300 - ln))
            out += out[o:o + ln]
            out += ext._filler(rng, max(0, 64 // count - ln) + int(rng.integers(0, 2)))
        out += ext._filler(rng, 1400)

        def want(blocks):
            return _static(blocks) and count in [v for k, v in _long_starts_by_step(blocks).items() if MID_STEP <= 64 * k < MID_STEP + 192]
        return bytes(out), want
    return make


def fresh_start_block(la, lb):
    """A (la bytes) straight in front of B (lb bytes), both copies of phrases further back; and, planted behind those
    phrases, A's bytes from the eighth on with B's first three: the candidate of the lane eight behind A's start, a match
    that ends beyond B's start -- the eight-byte parse has no token starting on B, the true one has"""
    def make(rng):
        out = ext._filler(rng, MID_STEP - 400)
        a0 = len(out)
        out += ext._filler(rng, la)
        out += ext._filler(rng, 30)
        b0 = len(out)
        out += ext._filler(rng, lb)
        out += ext._filler(rng, 30)
        out += out[a0 + 8:a0 + la] + out[b0:b0 + 3]
        out += ext._filler(rng, MID_STEP + int(rng.integers(4, 30)) - len(out))
        pa = len(out)
        out += out[a0:a0 + la] + out[b0:b0 + lb]
        out += ext._filler(rng, 1400)

        def want(blocks):
            m = blocks[0].matches() if _static(blocks) else []
            return (pa, la, pa - a0) in m and (pa + la, lb, pa + la - b0) in m and pa // 64 == (pa + la) // 64
        return bytes(out), want
    return make


def several_specs():
    specs = []
    for i, lengths in enumerate(((9, 10, 11, 12), (16, 17, 18, 19, 20))):
        for count in range(2, 7) if i == 0 else range(2, 4):
            specs.append(("several/%s/c%d" % ("short" if i == 0 else "long", count), phrase_block(lengths, count)))
    for la in (9, 10, 11, 12):
        for lb in (16, 18, 20):
            specs.append(("fresh/a%d/b%d" % (la, lb), fresh_start_block(la, lb)))
    return specs


# ---- the abandoned stream ----------------------------------------------------------------------------------------

def _nine_bit(rng, n):
    return bytearray(rng.integers(144, 256, n, dtype=np.uint8).tobytes())


def abandoned_blocks():
    """(name, bytes): eight-bit bytes (with a few matches) and nine-bit bytes, in both orders; the nine-bit part is long
    enough that the static stream passes the stored size, at a different pass for every length"""
    rng = np.random.default_rng(9081)
    out = []
    for i, noise in enumerate((4600, 5000, 5333, 6000, 7777, 8000)):
        head = ext._filler(rng, 3600)
        head += head[100:100 + 496]                       # 4096 bytes, a few long matches at its end
        tail = _nine_bit(rng, noise)
        out.append(("abandoned/fwd/%d" % noise, bytes(head + tail)))
        out.append(("abandoned/rev/%d" % noise, bytes(tail + head)))
    # and compressible text in front of noise that only just does not pay: the twin says which form it is
    s = hdtest.synth()
    text = bytes(s.text_like(4096, seed=5))
    for noise in (2000, 7000):
        out.append(("abandoned/text/%d" % noise, text + bytes(_nine_bit(rng, noise))))
        out.append(("abandoned/textrev/%d" % noise, bytes(_nine_bit(rng, noise)) + text))
    return out


# ---- the launches ------------------------------------------------------------------------------------------------

_PLANTED = []


def planted_blocks():
    if not _PLANTED:
        for i, (name, make) in enumerate(edge_specs() + long_specs() + several_specs()):
            b, want = ext._build(9000 + i, make)
            _PLANTED.append((name, b, want))
    return _PLANTED


def all_blocks():
    return [(n, b) for n, b, _ in planted_blocks()] + abandoned_blocks()


def test_planted_inputs_cover_the_cases():
    """no GPU: what the twin makes of every planted block"""
    blocks = planted_blocks()
    names = [n for n, _, _ in blocks]
    assert sum(n.startswith("edge/") for n in names) == 54 and sum(n.startswith("long/") for n in names) == 64
    assert 200 <= len(all_blocks()) <= 400
    for name, b, want in blocks:
        assert 2000 <= len(b) <= 12288 or name.startswith("edge/g704"), (name, len(b))
        r, twin = hdtest.oracle_twin(b, 1, cap=SLOT)
        assert r == 0, name
        st = deflate_tokens.read(twin)
        assert bytes(st.out) == b, name
        assert want(st.blocks), name
    # every number of long starts from two to six stands in one step of a group
    counts = set()
    for name, b, _ in blocks:
        if name.startswith("several/"):
            by = _long_starts_by_step(ext._twin_tokens(b))
            counts |= {v for k, v in by.items() if MID_STEP <= 64 * k < MID_STEP + 192}
    assert counts >= {2, 3, 4, 5, 6}, counts
    kinds = {}
    for name, b in abandoned_blocks():
        assert 2000 <= len(b) <= 12288 + 200, (name, len(b))
        kinds[name] = ext._twin_tokens(b)[0].kind
    assert all(k == "stored" for n, k in kinds.items() if "/fwd/" in n or "/rev/" in n), kinds
    assert "static" in kinds.values(), kinds


@pytest.mark.gpu
@pytest.mark.parametrize("frame,hdr,trl", FRAMES)
def test_level1_deep_group_cases_match_twin(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    blocks = all_blocks()
    members, crc, st = ext._launch(pkg, [b for _, b in blocks], fr)
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


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [er.RAW, er.RAW_FLUSH, er.BGZF], ids=["raw", "raw_flush", "bgzf"])
def test_level1_slot_limited_stream_is_refused_or_the_twins(pkg, frame):
    """the stream given up against the slot: one launch per room one below, at and one above each member's need"""
    flush = frame == er.RAW_FLUSH
    picked = [(n, b) for n, b in all_blocks() if n.startswith(("abandoned/", "edge/g2752", "fresh/"))][::3]
    names, datas = [n for n, _ in picked], [b for _, b in picked]
    models = [room.model(d, 1, flush) for d in datas]
    packed = room._pack(datas)
    hdr, trl = er.FRAME_BYTES[frame]
    rooms = sorted({r for b in models for r in (b.need - 1, b.need, b.need + 1)})
    assert len(rooms) <= 3 * len(picked)
    bad = []
    for r in rooms:
        total = r + hdr + trl
        bad += [(total,) + x for x in room.check_launch(pkg, names, datas, models, 1, frame, False, room.up16(total), total, packed)]
    assert not bad, bad[:12]
    assert pkg.lib().hipdeflate_stall_count() == 0
