"""Level 1's step after four of its vector instructions went (hd_deflate_static.hpp `step`, hd_device.hpp
queue_push): the candidate's bytes aligned by the candidate's whole position, the match token word made from a position
register that carries the word's constant, the queue push in which every lane sends, and the long-match events' ring
addresses masked with a literal.  The bar is the one of test_gpu_l1_extension.py and test_gpu_l1_deep_groups.py, whose
builders the inputs are made with: kernel bytes == CPU twin bytes (oracle/hd_deflate_twin.c) in the RAW, RAW_FLUSH and BGZF
frames, one launch of a few hundred blocks of 4..9 KiB per frame plus one block of 0xff00 and one of exactly 65536 bytes;
test_planted_inputs_reach_every_case (no GPU) holds the inputs to what they are planted for, on the twin.

  * candidate bytes (item 1).  A candidate at position 0xffc + j, j = 0..3 -- every bit of the position from bit 2 up to
    the ring's size set, its three dwords crossing the ring's end into the 16 mirrored bytes -- for a match at a position
    with every value of its low two bits: all sixteen combinations.  The same at 0xff7c + j in the last steps of a
    65536-byte block, and own bytes across the ring's wrap at 8192.  (A lane without a candidate passes -1, all
    32 bits set: every literal of every block.)
  * token word (item 2).  Matches of 4, 8, 9 and 258 bytes at distances 1, 2, 4 and the largest the window admits, in the
    first group of a block and in its last; in the last steps of the last group of the 0xff00- and the 65536-byte block,
    where the position is as large as a group's step sees it (0xfabf, 0xfebf: the token word's constant is added to it and
    must reach the tag's bits only), and in the general steps behind; and the blocks of test_gpu_l1_deep_groups.py whose
    stream is abandoned part-way.
  * queue push (item 3).  Blocks planned step by step -- k - 1 literals and a match that covers the rest of the step and as
    much of the next as its plan wants -- so that the steps of the groups push every token count 0..64 into the queue at every
    fill 0..63: all 4160 pairs, counted on the twin's tokens.  With them come a token on lane 63, lanes without a token
    above the last token, pushes that wrap round lane 63 by 1 and by 63, and steps wholly covered by a match, which push
    nothing.
  * event addresses (item 4).  Matches of 9, 15, 16, 65, 66, 130, 257 and 258 bytes whose own bytes cross position 4096 --
    the ring's end and its 16 mirrored bytes -- 4, 12 and 64 bytes in (where they are long enough to reach it), the same
    lengths with the candidate's bytes crossing
    it, and the blocks of test_gpu_l1_deep_groups.py with two to six long matches in one step.
Every launch must leave hipdeflate_stall_count() at 0 and give every member status 0."""
import gzip
import os
import zlib

import numpy as np
import pytest

import deflate_tokens
import hdtest
import test_gpu_l1_deep_groups as deep
import test_gpu_l1_extension as ext

FRAMES = [f for f in ext.FRAMES if f[0] in ("RAW", "RAW_FLUSH", "BGZF")]
SLOT = ext.SLOT
FIRST_GROUP_STEP = 704 + 64          # step 1 of a block's first group ...
LAST_GROUP_STEP = 704 + 4096 + 64    # ... and of the last group of a block that ends ~1500 bytes behind it
WORD_LENGTHS = (4, 8, 9, 258)
EVENT_LENGTHS = (9, 15, 16, 65, 66, 130, 257, 258)
BIG = ((0xff00, 63168 + 15 * 64), (65536, 64192 + 15 * 64))      # (n, the last step of its last group)
BIG_CAND = 0xff7c                    # candidates of the 65536-byte block's last steps: the last place with room for four matches behind
QUEUE_N = 8192
QUEUE_BLOCKS_MAX = 260


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def in_group(S, n):
    """step S of a block of n bytes runs inside a 16-step group (hd_deflate_static.hpp: the main loop's condition)"""
    if S < 704:
        return False
    sg = 704 + (S - 704) // 1024 * 1024
    return sg + 15 * 64 + 63 + 258 <= n


# ---- item 1: candidate positions with all upper bits set, every pair of low bits -----------------------------------

def cand_specs():
    specs = []
    for j in range(4):
        for i in range(4):
            step = 704 + 4096 + 3 * 64                 # 4992, a multiple of 4
            lane = 8 + i
            specs.append(("cand/c%d/p%d" % (j, i), ext.match_block(lane, 12, step + lane - (0xffc + j), step)))
    # own bytes across the ring's wrap at 8192: lanes 60..63 of step 8128 (step 4 of the group at 7872)
    for i in range(4):
        specs.append(("ownwrap/p%d" % i, ext.match_block(60 + i, 12, 200 + i, 8128)))
    return specs


# ---- item 2: the token word ------------------------------------------------------------------------------------------

def word_specs():
    specs = []
    for where, step in (("first", FIRST_GROUP_STEP), ("last", LAST_GROUP_STEP)):
        for length in WORD_LENGTHS:
            for dist in (1, 2, 4):
                for lane in sorted({0, dist - 1}):
                    specs.append(("word/%s/d%d/l%d/n%d" % (where, dist, lane, length), ext.match_block(lane, length, dist, step)))
            lane = 37
            specs.append(("word/%s/reach/l%d/n%d" % (where, lane, length),
                          deep.long_block(lane, length, min(deep.window_reach(step, lane), step + lane - 40), step)
                          if step > 2000 else ext.match_block(lane, length, step + lane - 40, step)))
    return specs


def big_block(n, last_step):
    """filler, a compressible stretch, and matches in the last steps of the block's last group and in the steps behind it;
    -> (bytes, predicate): one static block that holds every planted token"""
    plan = [(last_step - 8 * 64, 0, 9, 1), (last_step - 7 * 64, 1, 8, 2), (last_step - 6 * 64, 3, 4, 4),
            (last_step - 5 * 64, 20, 258, 300), (last_step, 5, 4, 640), (last_step, 30, 9, 700), (last_step, 63, 12, 950),
            (n - 260, 0, 9, 300), (n - 130, 0, 40, 77)]

    def make(rng):
        out = ext._filler(rng, 2000)
        for _ in range(24):
            ext._plant(out, 300, 258)
        planted = []
        for step, lane, length, dist in plan:
            out += ext._filler(rng, step + lane - len(out))
            planted.append((len(out), length, dist))
            ext._plant(out, dist, length)
        out += ext._filler(rng, n - len(out))
        assert len(out) == n

        def want(blocks):
            return deep._static(blocks) and all(p in blocks[0].matches() for p in planted)
        want.planted = planted
        return bytes(out), want
    return make


def big_cand_block():
    """the 65536-byte block again, with candidates at BIG_CAND + j for matches in the general steps at its end"""
    def make(rng):
        out = ext._filler(rng, 2000)
        for _ in range(24):
            ext._plant(out, 300, 258)
        src = BIG_CAND
        out += ext._filler(rng, src + 13 - len(out))   # the sources: nine bytes from src + j on are copied below, inside one step
        planted = []
        for j in range(4):
            pad = (j + 1 - len(out)) & 3               # the match starts at a position = j + 1 mod 4: every pair over the four
            out += ext._filler(rng, pad)
            planted.append((len(out), 9, len(out) - (src + j)))
            for k in range(9):
                out.append(out[src + j + k])
            out.append((out[src + j + 9] + 1) % 144)
        out += ext._filler(rng, 65536 - len(out))
        assert len(out) == 65536

        def want(blocks):
            return deep._static(blocks) and all(p in blocks[0].matches() for p in planted)
        want.planted = planted
        return bytes(out), want
    return make


# ---- item 4: the events' ring addresses ------------------------------------------------------------------------------

def event_specs():
    specs = []
    for length in EVENT_LENGTHS:
        # own bytes across 4096: the match starts 4, 12 and 64 bytes below it (step 4032 = step 4 of the group at 3776)
        for lane in (60, 52, 0):
            if 4032 + lane + length <= 4096:
                continue
            specs.append(("evown/l%d/n%d" % (lane, length), deep.long_block(lane, length, 200, 4032)))
        # the candidate's bytes across 4096: the source starts 6, 2 and (the longer ones) 96 bytes below it
        for below in (6, 2, 96):
            if below == 96 and length < 130:
                continue
            step, lane = 704 + 4096 + 2 * 64, 10
            specs.append(("evcand/b%d/n%d" % (below, length), deep.long_block(lane, length, step + lane - (4096 - below), step)))
    return specs


# ---- item 3: every token count into every queue fill -------------------------------------------------------------------

def step_pushes(b, positions):
    """[(S, fill in front of the step, tokens of the step)] of a block whose token positions are `positions`"""
    n = len(b)
    counts = np.bincount(np.asarray(positions, dtype=np.int64) // 64, minlength=(n + 63) // 64)
    out, fill = [], 0
    for k, c in enumerate(counts):
        out.append((64 * k, fill, int(c)))
        fill = (fill + int(c)) % 64
    return out


def queue_block(rng, todo, n=QUEUE_N):
    """a block planned so that its steps push the (fill, count) pairs still in `todo`; what it really pushes the twin says"""
    out = ext._filler(rng, 64)
    fill, avoid = 0, -1
    end = n - 1500

    def literals(k):
        nonlocal avoid
        for _ in range(k):
            v = int(rng.integers(0, 144))
            if v == avoid:
                v = (v + 1) % 144
            out.append(v)
            avoid = -1

    def pick(f, lo, hi):
        want = [c for c in range(lo, hi + 1) if (f, c) in todo]
        return int(rng.choice(want)) if want else int(rng.integers(lo, hi + 1))

    while len(out) < end:
        pos = len(out)
        S = pos // 64 * 64
        a = S + 64 - pos
        c = pick(fill, 1, a)
        f2 = (fill + c) % 64
        c2 = pick(f2, 0, 64)
        j2 = 64 + int(rng.integers(0, 24)) if c2 == 0 else int(rng.integers(0, min(64 - c2, 30) + 1))
        fill = f2
        if c == a and j2 == 0:
            literals(a)
            continue
        L = min(max(a - (c - 1) + j2, 4), 258)
        literals(c - 1)
        d = int(rng.integers(65, min(len(out), 700) + 1)) if len(out) >= 130 else 0
        if not d:
            literals(L)
            continue
        for _ in range(L):
            out.append(out[-d])
        avoid = out[-d]
    literals(n - len(out))
    return bytes(out)


_QUEUE = []


def queue_blocks():
    """(name, bytes, None) until the twin's tokens cover every (fill, count) pair in the steps of the groups"""
    if not _QUEUE:
        todo = {(f, c) for f in range(64) for c in range(65)}
        rng = np.random.default_rng(31415)
        while todo and len(_QUEUE) < QUEUE_BLOCKS_MAX:
            b = queue_block(rng, todo)
            blocks = ext._twin_tokens(b)
            if not deep._static(blocks):
                continue
            before = len(todo)
            todo -= {(f, c) for S, f, c in step_pushes(b, blocks[0].pos) if in_group(S, len(b))}
            if len(todo) < before:
                _QUEUE.append(("queue/%d" % len(_QUEUE), b, None))
    return _QUEUE


# ---- the launch -------------------------------------------------------------------------------------------------------

_PLANTED = []


def planted_blocks():
    """(name, bytes, what the twin must make of it)"""
    if not _PLANTED:
        specs = cand_specs() + word_specs() + event_specs()
        specs += [("big/%d" % n, big_block(n, last)) for n, last in BIG] + [("bigcand/65536", big_cand_block())]
        for i, (name, make) in enumerate(specs):
            b, want = ext._build(14000 + i, make)
            _PLANTED.append((name, b, want))
    return _PLANTED


def borrowed_blocks():
    """of test_gpu_l1_deep_groups.py: two to six long matches in one step, and the streams given up part-way"""
    return [(n, b) for n, b, _ in deep.planted_blocks() if n.startswith(("several/", "fresh/"))] + deep.abandoned_blocks()


def all_blocks():
    return [(n, b) for n, b, _ in planted_blocks()] + [(n, b) for n, b, _ in queue_blocks()] + borrowed_blocks()


def test_planted_inputs_reach_every_case():
    """no GPU: what the twin makes of every input"""
    blocks = planted_blocks()
    names = {n for n, _, _ in blocks}
    assert {"cand/c%d/p%d" % (j, i) for j in range(4) for i in range(4)} <= names
    for name, b, want in blocks:
        assert name.startswith(("big", "ownwrap")) or 2000 <= len(b) <= 9216, (name, len(b))
        r, twin = hdtest.oracle_twin(b, 1, cap=SLOT)
        assert r == 0, name
        st = deflate_tokens.read(twin)
        assert bytes(st.out) == b, name
        assert deep._static(st.blocks), name
        m = st.blocks[0].matches()
        assert want(st.blocks) if callable(want) else want in m, name
        kind = name.split("/")[0]
        if kind == "cand":
            j, i = int(name.split("/")[1][1:]), int(name.split("/")[2][1:])
            pos, length, dist = want
            assert pos - dist == 0xffc + j and pos & 3 == i and in_group(pos // 64 * 64, len(b)), name
        elif kind == "ownwrap":
            pos, length, dist = want
            assert pos < 8192 < pos + length and in_group(pos // 64 * 64, len(b)), name
        elif kind == "word" and not callable(want):
            pos, length, dist = want
            assert in_group(pos // 64 * 64, len(b)), name
            first, last = pos < 704 + 1024, not in_group(pos // 64 * 64 + 1024, len(b))
            assert (first if "/first/" in name else last and not first), name
        elif kind == "evown":
            length = int(name.split("/")[2][1:])
            assert any(p < 4096 < p + ln and ln == length and in_group(p // 64 * 64, len(b)) for p, ln, d in m), name
        elif kind == "evcand":
            length = int(name.split("/")[2][1:])
            assert any(p - d < 4096 < p - d + ln and ln == length and in_group(p // 64 * 64, len(b)) for p, ln, d in m), name
    # the big blocks: the last step of the last group holds planted matches, and so do the general steps behind it
    for (n, last), (name, b, want) in zip(BIG, [x for x in blocks if x[0].startswith("big/")]):
        assert len(b) == n and in_group(last, n) and not in_group(last + 64, n), name
        assert any(p // 64 * 64 == last and p % 64 == 63 for p, _, _ in want.planted), name
        assert any(p > last + 64 for p, _, _ in want.planted), name
        assert {d for _, _, d in want.planted} >= {1, 2, 4} and {ln for _, ln, _ in want.planted} >= {4, 8, 9, 258}, name
    name, b, want = next(x for x in blocks if x[0] == "bigcand/65536")
    assert len(b) == 65536 and {((p - d) & 3, p & 3) for p, _, d in want.planted} == {(j, (j + 1) & 3) for j in range(4)}
    assert all(BIG_CAND <= p - d < BIG_CAND + 4 for p, _, d in want.planted)
    # every length and distance of the token word, in a first and in a last group
    words = {tuple(n.split("/")[1:]) for n in names if n.startswith("word/")}
    for where in ("first", "last"):
        for length in WORD_LENGTHS:
            assert (where, "reach", "l37", "n%d" % length) in words
            for dist in (1, 2, 4):
                assert (where, "d%d" % dist, "l%d" % (dist - 1), "n%d" % length) in words
    # a stream given up part-way, and up to six events in one step
    borrowed = borrowed_blocks()
    assert any(ext._twin_tokens(b)[0].kind == "stored" for n, b in borrowed if n.startswith("abandoned/"))
    counts = set()
    for n, b in borrowed:
        if n.startswith("several/"):
            counts |= set(deep._long_starts_by_step(ext._twin_tokens(b)).values())
    assert counts >= {2, 3, 4, 5, 6}, counts


def test_queue_inputs_push_every_count_into_every_fill():
    """no GPU: on the twin's tokens, the steps of the groups push 0..64 tokens into the queue at every fill 0..63"""
    blocks = queue_blocks()
    assert 30 <= len(blocks) <= QUEUE_BLOCKS_MAX, len(blocks)
    seen, lane63, above, covered = set(), 0, 0, 0
    for name, b, _ in blocks:
        assert len(b) == QUEUE_N
        st = ext._twin_tokens(b)
        assert deep._static(st), name
        pos = set(st[0].pos)
        ends = {p + max(ln, 1) for p, ln in zip(st[0].pos, st[0].length)}
        for S, f, c in step_pushes(b, st[0].pos):
            if not in_group(S, len(b)):
                continue
            seen.add((f, c))
            lane63 += S + 63 in pos
            above += c > 0 and S + 63 not in pos
            # a step that pushes nothing lies inside one match
            if c == 0:
                covered += 1
                assert not any(S < e <= S + 64 for e in ends) or S + 64 in ends, (name, S)
    missing = {(f, c) for f in range(64) for c in range(65)} - seen
    assert not missing, sorted(missing)[:20]
    assert lane63 >= 64 and above >= 64 and covered >= 64, (lane63, above, covered)
    # pushes that wrap round lane 63 by 1 and by 63 tokens
    assert any(f + c - 64 == 1 for f, c in seen) and any(f + c - 64 == 63 for f, c in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("frame,hdr,trl", FRAMES)
def test_level1_trimmed_step_matches_twin(pkg, frame, hdr, trl):
    fr = getattr(pkg, "FRAME_" + frame)
    blocks = all_blocks()
    assert 200 <= len(blocks) <= 700, len(blocks)
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
