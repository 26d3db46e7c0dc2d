"""The piece decoders of both indexes and the carry kernels -- k_inflate_piece, k_carry_piece, k_carry_decode, k_carry_tails,
k_carry_resolve (hd_inflate_size.hpp, hd_carry.hpp) -- held to the hand-built corpus of tests/deflate_gen.py, which the other
inflate kernels already answer to, and to the carry_ring family of tests/carry_rows.py.  Bit-exact against references that
hold none of the code under test: deflate_gen.expand() of the token lists for the bytes, the oracle for the verdicts, and the
plain-Python models, which tests/test_index_models_vs_oracle.py and tests/test_carry_rows.py pin to both.  64 sentinel bytes
around every output, a sentinel row around every table, hipdeflate_stall_count() == 0 behind every test.  No case provokes a
fault: every offset and length of a table lies inside its buffer, every refusal is a verdict the header defines, each runs once.

  * one-row streams: every corpus stream but the cap_minus1 family as a RAW stream through both indexes -- every code shape,
    every reject rule, 13..15-bit codewords, and the line between status 1 and status 2;
  * cut streams (carry_rows.cut_every / cut_mid): the index, then the decode on its table -- GZIP, a stride in ZLIB (the Adler
    pieces) and RAW; a stride of cut_every at groups of 4,096 bytes and of 1 byte (every row its own group: k_carry_tails
    loads its window from `out` once per row);
  * carry_ring at the default group size and at 65,536;
  * the faults family as row 1 behind a row of literals: the chain ends there, the claimed table is status 2 at row 1;
  * tables too tight on rows that are fine: out_size one (and 100) short on rows that end in a literal, a match, a stored
    block; reach one short behind 0 / 2 / 37 / 300 literals and inside a run of 15-bit codewords.

Which carry_ring case lands on which line of k_carry_decode, argued from the code (no broken kernel is run).  A group whose
rows all have reach 0 goes through the batch inflate and never sees these lines: every carry_ring row with a match reaches
back by itself (carry_rows.row_fill), and tests/test_carry_rows.py asserts from the token lists that each lies in a group of
the marker path at both group sizes used here:
  * `& (CARRY_WINDOW - 1)` on the ring store of copy(): without it a destination at row position >= 32768 is stored past the
    ring, and the next match that reads that slot gets a stale symbol -- ring_wrap_*: every (length, distance) has its
    destination across 32768 (ring_dA / ring_dB), and the matches behind 65536 (ring_s*_65536) read what was stored there;
  * the same mask on copy()'s ring LOAD: ring_s*_32768, a source across row position 32768;
  * put_literals before copy in the window loop: swapped, a literal behind a match of distance 32768 - k lands on the slot the
    match still reads -- ring_far_then_literals_* (literal_behind_far_k_in_ring), k = 0, 1, 2, 63, 64, 65, 257;
  * `s < 0` in copy(), the marker branch, from the window path: ring_straddle (straddle_p_1_257, p_32511_32767); from the
    scalar path: ring_long_codes, whose 13..15-bit matches reach over the row's start;
  * k_carry_tails' register layout and k_carry_resolve's body: ring_all_markers_* put a marker on every symbol of rows of
    1,023 .. 70,001 bytes; ring_source_slot_* put the byte a marker names on slots 0, 1, 32767 of the window in LDS."""
import importlib
import os

import pytest

import carry_rows as cr
import deflate_gen as dg
import hdtest
import stream_carry_model as cm
from carry_dev import GZIP, RAW, ZLIB, both, decode_check, index_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def dev():
    return importlib.import_module("7bgzf_amd.device")


@pytest.fixture(autouse=True)
def no_stalls(pkg):
    yield
    pkg.lib().hipdeflate_test_carry_group(0)
    assert pkg.lib().hipdeflate_stall_count() == 0


@pytest.fixture(scope="module")
def corpus():
    return [c for c in dg.cached_corpus() if c.family != "cap_minus1"]


@pytest.fixture(scope="module")
def every():
    return cr.cached("every")[0]


@pytest.fixture(scope="module")
def mid():
    return cr.cached("mid")[0]


@pytest.fixture(scope="module")
def ring():
    return cr.cached("ring")


def run_both(torch, dev, c, frame):
    x, t = both(torch, dev, c.compose(frame), frame, c.plain, zlib_ok=c.zlib)
    sizes, reach = c.table()
    assert t[2] == sizes and t[4] == reach, c.name
    return x, t


# ---- one-row streams: the two piece decoders at every header and token edge ---------------------------------------------------------

@pytest.mark.parametrize("k", range(8))
def test_one_row_streams(torch, dev, corpus, k):
    part = corpus[k::8]
    assert len(part) >= 70
    seen = set()
    for c in part:
        x = index_check(torch, dev, c.stream, RAW, carry=False)
        y = index_check(torch, dev, c.stream, RAW)
        seen |= {x[0]["status"], y[0]["status"]}
    assert seen == {0, 1, 2}                                  # (every slice holds streams of all three kinds)


# ---- cut streams: the index, then the decode on its table ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(16))
def test_cut_every(torch, dev, every, k):
    for c in every[k::16]:
        run_both(torch, dev, c, GZIP)


@pytest.mark.parametrize("k", range(8))
def test_cut_mid(torch, dev, mid, k):
    for c in mid[k::8]:
        run_both(torch, dev, c, GZIP)


@pytest.mark.parametrize("frame", (ZLIB, RAW))
def test_cut_streams_in_the_other_frames(torch, dev, every, mid, frame):
    for c in every[3::8] + mid[5::8]:
        run_both(torch, dev, c, frame)


def test_libdeflate_only_forms_as_rows(torch, dev, every, mid):
    """litlen 286 / 287 and offset 30 / 31 in a row of their own: zlib refuses them, the bytes are the token lists'; the
    row reaches back into the stored row in front of it (but for static_lit286_off0, whose distance is 1)"""
    n = back = 0
    for c in every + mid:
        if not c.zlib:
            n += 1
            x, t = run_both(torch, dev, c, ZLIB)
            assert t[4] == c.table()[1] and (max(t[4]) > 0) == (c.name != "static_lit286_off0"), c.name
            back += max(t[4]) > 0
    assert (n, back) == (10, 8)


@pytest.mark.parametrize("group", (4096, 1))
def test_small_groups(torch, dev, pkg, every, group):
    for c in every[::8]:
        pkg.lib().hipdeflate_test_carry_group(group)
        run_both(torch, dev, c, GZIP)


# ---- carry_ring ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", (0, 65536))
@pytest.mark.parametrize("k", range(10))
def test_carry_ring(torch, dev, pkg, ring, k, group):
    for c in ring[k::10]:
        pkg.lib().hipdeflate_test_carry_group(group)
        run_both(torch, dev, c, RAW if k & 1 else GZIP)


# ---- fault rows ------------------------------------------------------------------------------------------------------------------------

def test_fault_rows(torch, dev, corpus):
    n = valid = 0
    names = set()
    for c in corpus:
        if c.family != "faults":
            continue
        n += 1
        names.add(c.name)
        r, out = hdtest.oracle_inflate(c.stream, 1 << 21)
        f = cr.fault_row(c, len(out) if r == dg.OK else None)
        x = index_check(torch, dev, f.stream, RAW)[0]
        alone = cm.index_carry(c.stream, RAW)[0]
        d = decode_check(torch, dev, f.stream, RAW, *f.table, plain=f.plain)
        if f.plain is not None:                               # dist_past_out_*: the match reaches into the lead
            valid += 1
            assert x["status"] == 0 and d["status"] == 0 and d["out_bytes"] == len(f.plain), c.name
            continue
        assert x["status"] == alone["status"] and x["nchunks"] == 1 + alone["nchunks"], c.name
        assert (d["status"], d["bad_chunk"]) == (2, 1), c.name
    assert n >= 60 and valid == len(dg.MATCH_DISTS)
    assert {"cap_over_on_literal", "cap_over_on_match", "cap_over_on_stored"} <= names       # the three scalar room checks


# ---- tables too tight, on rows that are fine -------------------------------------------------------------------------------------------

def _ends(row):
    """how a row ends: 'stored' | 'match' | 'literal' | 'literals300' (300 literals and more behind its last match)"""
    b = row[-1]
    if b.kind == "stored":
        return "stored" if b.data else None
    if not b.tokens:
        return None
    if not isinstance(b.tokens[-1], int):
        return "match"
    n = 0
    while n < len(b.tokens) and isinstance(b.tokens[-1 - n], int):
        n += 1
    return "literals300" if n >= 300 else "literal"


def _plain_rows(c):
    """the stream's rows are its lists: no flush point inside one"""
    return len(c.table()[0]) == len(c.rows)


def tight_size_picks(every, per=4):
    picks = {"stored": [], "match": [], "literal": [], "literals300": []}
    for c in every:
        if not _plain_rows(c):
            continue
        reach = c.table()[1]
        for i in range(1, len(c.rows)):
            kind = _ends(c.rows[i])
            if kind and len(picks[kind]) < per and max(reach[:i + 1]) > 0 and \
                    (kind == "literals300" or not any(c is p[0] for p in picks[kind])):       # (a stream gives one row of a kind)
                picks[kind].append((c, i))
    return picks


def test_out_size_too_small(torch, dev, every):
    picks = tight_size_picks(every + [cr.literal_tails()])
    assert all(len(v) >= 2 for v in picks.values()), {k: len(v) for k, v in picks.items()}
    for kind, rows in picks.items():
        for c, i in rows:
            stream = c.compose(GZIP)
            x, *t = cm.index_carry(stream, GZIP)
            for less in (1, 100) if kind == "literals300" else (1,):
                u = [list(col[:i + 1]) for col in t]
                u[2][i] -= less
                d = decode_check(torch, dev, stream, GZIP, *u)
                assert (d["status"], d["bad_chunk"]) == (2, i), (c.name, i, kind, less)


def tight_reach_picks(every):
    """(a) per count of literals in front: a match-matrix row whose one match reaches over the row's start;
    (b) rows whose furthest match has a 15-bit litlen codeword.  Only rows whose table, with that reach lowered by one, still
    holds a reach > 0 in the rows up to it: else the group goes through the batch inflate, and k_inflate's distance refusal
    would answer in the place of k_carry_decode's check against the claim"""
    a, b = {}, []
    for c in every:
        if not _plain_rows(c):
            continue
        reach = c.table()[1]
        for i in range(1, len(c.rows)):
            blk = c.rows[i][0]
            if blk.kind == "stored" or not (reach[i] > 1 or (reach[i] and max(reach[:i]))):
                continue                                         # (lowered by one, the table must still take the marker path)
            p, far = 0, None
            for j, t in enumerate(blk.tokens):
                if isinstance(t, int):
                    p += 1
                    continue
                if t[1] - p == reach[i] and far is None:
                    far = (j, t)
                p += t[0]
            if far is None:
                continue
            j, t = far
            if c.name.startswith("match_d") and j in (0, 2, 37, 300) and all(isinstance(q, int) for q in blk.tokens[:j]):
                a.setdefault(j, (c, i))
            if blk.lit_lens is not None and len(t) == 4 and len(b) < 3 and 0 < j < len(blk.tokens) - 1 and \
                    all(blk.lit_lens[q if isinstance(q, int) else q[2]] == 15 for q in blk.tokens[j - 1:j + 2]):
                b.append((c, i))
    return a, b


def test_reach_too_small(torch, dev, every):
    a, b = tight_reach_picks(every)
    assert sorted(a) == [0, 2, 37, 300] and b, (sorted(a), len(b))
    for c, i in list(a.values()) + b:
        stream = c.compose(GZIP)
        x, *t = cm.index_carry(stream, GZIP)
        u = [list(col[:i + 1]) for col in t]
        u[4][i] -= 1
        assert all(cr.marker_path_rows(u[2], u[4])), (c.name, i)
        d = decode_check(torch, dev, stream, GZIP, *u)
        assert (d["status"], d["bad_chunk"]) == (2, i), (c.name, i)
