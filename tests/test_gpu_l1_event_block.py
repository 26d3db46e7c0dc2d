"""Level 1's long-match events as the step runs them: one block of assembly per step that takes the capped starts in rising
lane order, extends each over the ring, re-threads the parse behind it and hands the step's token starts back
(hd_deflate_static.hpp, HD_L1_EVENTS).

The bar of the GPU test is the one of every encode test here: kernel bytes == CPU twin bytes (oracle/hd_deflate_twin.c), here
in the RAW, RAW_FLUSH and BGZF frames, a few hundred blocks of 4..8 KiB in one launch (a 16-step group, where the block
runs with the constant bound of 258, needs n >= 704 + 1281) and one 0xff00-byte block, whose last steps run outside the
groups with the bound cut to the bytes the block has left.  The inputs are made with the builders of test_gpu_l1_extension.py
and test_gpu_l1_deep_groups.py.

What the block does differently from the C++ it replaces is what the planted inputs stand on, and
test_planted_inputs_reach_every_case (no GPU) holds them to it.  That test restates the step in Python as the kernel runs
it -- table look-up and publish, the eight-byte verify, the greedy chain over the eight-byte lengths, then the EVENTS -- checks
the restatement against the twin's own tokens, and asserts that the planted blocks contain:
  * an event at lane 0 and one at lane 63 (the lane select lives in M0);
  * a true length of exactly 8 (no exit of its own: the walk ends where it begins and nothing changes);
  * the lengths 9, 15, 16, 65, 66 (a second pass of the extension: the passes compare bytes 2..65, 66..129, 130..193 and
    194..257 of the match), 71, 72, 129, 130, 193, 194, 257, 258 and 300 (258 is the no-hit exit of the last pass);
  * a match that runs into the block's end;
  * up to six events in one step;
  * an event on a fresh start made by the previous event's walk;
  * walks of 0, 1 and at least 8 hops, a walk that lands on lane 63 and one that leaves the step;
  * a stream that is abandoned on the way, in blocks long enough to run in groups: the twin's member is the stored one."""
import gzip
import os
import zlib

import numpy as np
import pytest

import hdtest
import test_gpu_l1_deep_groups as deep
import test_gpu_l1_extension as ext

FRAMES = [f for f in ext.FRAMES if f[0] in ("RAW", "RAW_FLUSH", "BGZF")]
SLOT = ext.SLOT
LENGTHS = (8, 9, 15, 16, 65, 66, 71, 72, 129, 130, 193, 194, 257, 258)
STEP = 2752 + 5 * 64                 # a step in the middle of the group that starts at 704 + 2 * 1024
WIN, ENTRIES, LOOKAHEAD, PIECE = 4096, 1536, 384, 1024          # include/hipdeflate_params.h, level 1
K1, K2 = 0x9E3779, 0xC2B2AE


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


# ---- the step, restated --------------------------------------------------------------------------------------------

def _slot(b, p):
    lo24 = b[p] | (b[p + 1] << 8) | (b[p + 2] << 16)
    hi16 = b[p + 2] | (b[p + 3] << 8)
    return ((((lo24 * K1 + hi16 * K2) & 0xffffffff) >> 16) * ENTRIES) >> 16


def events_of(b):
    """([(step, lane, true length, hops, where the walk ended: a lane or 64 = it left the step, on a fresh start of the event
    before, lane clipped by the block's end)], events per step, [(position, length, distance)] of the parse)"""
    n = len(b)
    table = [0] * ENTRIES
    filled, carry = 0, 0
    events, per_step, tokens = [], {}, []
    for S in range(0, n, 64):
        while filled < n and filled < S + LOOKAHEAD:
            filled += PIECE
        lo = max(0, filled - WIN)
        lanes = min(64, n - S)
        cand = [0] * 64
        slots = [-1] * 64
        for l in range(lanes):
            p = S + l
            if p + 4 <= n:
                slots[l] = _slot(b, p)
                cand[l] = table[slots[l]]                # (blocks below 2^16: position + 1 itself)
        for l in range(lanes):
            if slots[l] >= 0:
                table[slots[l]] = S + l + 1
        jump8, capped, dist = [1] * 64, [False] * 64, [0] * 64
        for l in range(lanes):
            p, c = S + l, cand[l] - 1
            if slots[l] < 0 or c < lo or b[c:c + 4] != b[p:p + 4]:
                continue
            k = 4
            while k < 8 and p + k < n and b[c + k] == b[p + k]:
                k += 1
            jump8[l], dist[l] = k, p - c
            capped[l] = k == 8 and n - p > 8
        if carry >= lanes:
            carry -= lanes
            continue
        starts, x = set(), carry
        while x < lanes:
            starts.add(x)
            x += jump8[x]
        lenv = list(jump8)
        todo = {l for l in range(lanes) if capped[l]}
        fresh_before = set()
        while starts & todo:
            m = min(starts & todo)
            todo.discard(m)
            p, d = S + m, dist[m]
            maxlen = min(258, n - p)
            ln = 8
            while ln < maxlen and b[p + ln] == b[p + ln - d]:
                ln += 1
            per_step[S] = per_step.get(S, 0) + 1
            on_fresh = m in fresh_before
            if ln == 8:
                events.append((S, m, 8, 0, min(m + 8, 64), on_fresh, False))
                continue
            lenv[m] = ln
            x, hops, fresh = m + ln, 0, set()
            while x < 64 and x not in starts:
                fresh.add(x)
                x += lenv[x]
                hops += 1
            starts = {s for s in starts if not m < s < min(x, 64)} | fresh
            fresh_before = fresh
            events.append((S, m, ln, hops, min(x, 64), on_fresh, ln == n - p and ln < 258))
        last = max(s for s in starts if s < lanes)
        for s in sorted(starts):
            if s < lanes and dist[s]:
                tokens.append((S + s, lenv[s], dist[s]))
        carry = max(last + lenv[last], 64) - 64 if lanes == 64 else 0
    return events, per_step, tokens


# ---- the inputs ----------------------------------------------------------------------------------------------------

def run_block(lane, length, dist):
    """a copy of `length` bytes at distance `dist`, and behind it nothing for the next 80 bytes that the table knows: the
    walk behind the match lands on old starts (literals) at once"""
    return ext.match_block(lane, length, dist, STEP, tail=2600)


def planted_specs():
    specs = []
    for lane in (0, 31, 63):
        for length in LENGTHS:
            specs.append(("len/l%d/n%d" % (lane, length), run_block(lane, length, ext.NEAR)))
        specs.append(("len/l%d/n300" % lane, deep.long_block(lane, 300, 64 + lane + 1, STEP)))
        for clip in (9, 40, 100, 257):
            specs.append(("clip/l%d/c%d" % (lane, clip), ext.match_block(lane, 0, ext.NEAR, ext.GROUP_STEP, clip=clip)))
    for count in range(2, 7):
        specs.append(("several/c%d" % count, deep.phrase_block((9, 10, 11, 12), count)))
    for la in (9, 12):
        for lb in (16, 20):
            specs.append(("fresh/a%d/b%d" % (la, lb), deep.fresh_start_block(la, lb)))
    return specs


def walk_blocks():
    """FASTQ-like blocks: quality strings are full of short repeats a few bytes apart, which is where the walk behind a
    long match takes many hops.  (Seeded; test_planted_inputs_reach_every_case says what they hold)"""
    s = hdtest.synth()
    pool = bytes(s.fastq_like(1 << 19, seed=77))
    return [("walk/%d" % i, pool[o:o + 6144]) for i, o in enumerate(range(0, 24 * 20000, 20000))]


_PLANTED = []


def planted_blocks():
    if not _PLANTED:
        for i, (name, make) in enumerate(planted_specs()):
            b, _ = ext._build(7000 + i, make)
            _PLANTED.append((name, b))
        _PLANTED.extend(walk_blocks())
        _PLANTED.extend((n, b) for n, b in deep.abandoned_blocks() if "/fwd/" in n or "/rev/" in n)
    return _PLANTED


def seeded_blocks():
    s = hdtest.synth()
    rng = np.random.default_rng(9177)
    pools = [bytes(s.fastq_like(1 << 20, seed=41)), bytes(s.fastq_like(1 << 20, seed=42, first_record=0)), bytes(s.text_like(1 << 20, seed=43))]
    blocks = []
    for i in range(300):
        pool = pools[i % 3]
        n = int(rng.integers(4096, 8193))
        o = int(rng.integers(0, len(pool) - n))
        blocks.append(("seeded/%d" % i, pool[o:o + n]))
    blocks.append(("seeded/ff00", pools[0][12345:12345 + 0xff00]))
    return blocks


_BLOCKS = []


def all_blocks():
    if not _BLOCKS:
        _BLOCKS.extend(planted_blocks() + seeded_blocks())
    return _BLOCKS


def test_planted_inputs_reach_every_case():
    """no GPU: the restated step agrees with the twin's tokens on every planted block, and its events cover the cases"""
    ev, most, long300 = [], 0, 0
    for name, b in planted_blocks():
        blocks = ext._twin_tokens(b)
        events, per_step, tokens = events_of(b)
        if name.startswith("abandoned/"):
            # given up on the way, in a block that runs in groups; the eight-bit part in front has long matches
            assert blocks[0].kind == "stored" and len(b) >= 704 + 1281 and (events or "/rev/" in name), name
            continue
        assert len(blocks) == 1 and blocks[0].kind == "static", name
        assert tokens == sorted(blocks[0].matches()), name
        grouped = len(b) >= 704 + 1281
        ev += [e + (grouped and 704 <= e[0] < 704 + (len(b) - 704 - 1281) // 1024 * 1024 + 1024,) for e in events]
        most = max([most] + list(per_step.values()))
        long300 += name.endswith("/n300") and any(e[2] == 258 for e in events)
    in_group = [e for e in ev if e[7]]
    lengths = {e[2] for e in in_group}
    assert lengths >= set(LENGTHS), sorted(set(LENGTHS) - lengths)
    assert any(e[1] == 0 and e[2] > 8 for e in in_group) and any(e[1] == 63 and e[2] > 8 for e in in_group)
    # 300 bytes: a token of 258 whose copy goes on behind it
    assert long300 == 3, long300
    assert any(e[6] for e in ev), "no match runs into the block's end"
    assert any(e[6] and not e[7] for e in ev), "... outside the groups, where the bound is what the block has left"
    assert most >= 6, most
    assert any(e[5] for e in in_group), "no event on a fresh start of the event before"
    hops = {e[3] for e in in_group if e[2] > 8}
    assert 0 in hops and 1 in hops and max(hops) >= 8, sorted(hops)
    assert any(e[3] >= 1 and e[4] == 63 for e in in_group), "no walk lands on lane 63"
    assert any(e[3] >= 1 and e[4] == 64 for e in in_group), "no walk leaves the step"
    assert any(e[3] == 0 and e[4] == 64 for e in in_group), "no match leaves the step itself"
    print("events %d (in groups %d), most per step %d, hops up to %d" % (len(ev), len(in_group), most, max(hops)))


@pytest.mark.gpu
@pytest.mark.parametrize("frame,hdr,trl", FRAMES)
def test_level1_event_block_matches_twin(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    blocks = all_blocks()
    assert 300 <= len(blocks) <= 500
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
        if frame == "BGZF":
            assert gzip.decompress(m) == b, (name, frame)
        elif frame == "RAW":
            assert zlib.decompress(m, -15) == b, (name, frame)
