"""What tests/wg_block_gen.py promises, pinned on the CPU twin: the GPU test of the per-block schedule
(test_gpu_wg_per_block.py) holds the kernels to the twin on these inputs, and these tests say why the inputs reach the
paths they are meant for -- how many DEFLATE blocks each `cuts` member has (the rounds of k_emit_wg: EW_SLOTS = 4 to a
round), how many matches of each `borders` block start behind a share border and have their source in front of it, which
piece counts `sizes` holds, that the noise is stored.  The counts are printed (pytest -s shows them) before they are
asserted.  Token lists come from deflate_tokens.read, which shares nothing with the twin."""
import zlib

import pytest

import deflate_tokens
import hdtest
import wg_block_gen as wg

LEVELS = (3, 4, 5, 6)
EW_SLOTS = 4                                          # hd_emit_wg.hpp


@pytest.fixture(scope="module")
def corpus():
    return wg.cached_corpus()


_streams = {}


def stream(c, level):
    """(member, token stream) of the twin's latency form at the default room"""
    key = (c.name, level)
    if key not in _streams:
        r, m = hdtest.codec_twin(c.data, level)
        assert r == 0, (c.name, level)
        _streams[key] = (m, deflate_tokens.read(m, expand=False))
    return _streams[key]


def fifth_block_room(member):
    """the room in which the member's fifth DEFLATE block just does not end: one byte less than the byte it ends in"""
    st = deflate_tokens.read(member, expand=False)
    assert len(st.blocks) > EW_SLOTS
    return (st.blocks[EW_SLOTS].end_bit + 7) // 8 - 1


def test_corpus_is_stable_and_within_a_block(corpus):
    again = wg.corpus()
    assert [(c.name, c.family, hdtest.sha(c.data)) for c in again] == [(c.name, c.family, hdtest.sha(c.data)) for c in corpus]
    assert {c.family for c in corpus} == {"sizes", "borders", "cuts", "fallbacks"}
    assert all(len(c.data) <= wg.MAX_BLOCK for c in corpus)
    assert len({hdtest.sha(c.data) for c in corpus if c.data}) == len([c for c in corpus if c.data]), "two blocks alike"


@pytest.mark.parametrize("level", LEVELS)
def test_every_input_encodes_the_same_in_both_forms(corpus, level):
    for c in corpus:
        r, lat = hdtest.codec_twin(c.data, level)
        r2, plain = hdtest.oracle_twin(c.data, level)
        assert r == 0 and r2 == 0 and lat == plain, (c.name, level)
        assert zlib.decompress(lat, -15) == c.data, (c.name, level)


def test_sizes_hold_every_piece_count(corpus):
    sizes = [c for c in corpus if c.family == "sizes"]
    assert [len(c.data) for c in sizes] == wg.SIZES
    assert sorted({wg.npieces(len(c.data)) for c in sizes}) == wg.PIECE_COUNTS
    # every rounding of the shares: for SP = 2 and 4, piece counts of every residue, and sharers without a piece
    for sp in (2, 4):
        assert {wg.npieces(len(c.data)) % sp for c in sizes} == set(range(sp))
        assert any(0 < wg.npieces(len(c.data)) < sp for c in sizes)


@pytest.mark.parametrize("level", LEVELS)
def test_cuts_reach_every_round_of_the_emit_kernel(corpus, level):
    counts = {}
    for c in corpus:
        if c.family == "cuts":
            counts[c.name] = len(stream(c, level)[1].blocks)
    print("level %d, DEFLATE blocks per cuts member: %s" % (level, counts))
    assert {4, 5, 6, 7} <= set(counts.values()), counts
    # the last block of the first round, the first of the second, the last of the second, the third round
    assert counts["cut4"] == 4 and counts["cut5"] == 5 and counts["cut6"] == 6 and counts["cut7"] == 7, counts
    assert counts["cut8"] == 2 * EW_SLOTS and counts["cut10"] > 2 * EW_SLOTS, counts
    if level == 3:
        assert counts["cut8_l3"] == 8, counts
    for c in corpus:
        if c.family == "cuts":
            assert all(b.kind == "dynamic" for b in stream(c, level)[1].blocks), c.name


@pytest.mark.parametrize("level", LEVELS)
def test_borders_have_matches_across_every_share_border(corpus, level):
    at_window = beyond = 0
    for c in corpus:
        if c.family != "borders":
            continue
        ms = stream(c, level)[1].all_matches()
        at_window += sum(1 for _, _, d in ms if d == 32768)
        beyond += sum(1 for _, _, d in ms if d > 32768)
        if c.name == "far_32769":
            assert not ms, "the only copies lie 32769 bytes back"
            continue
        for sp in (2, 4):
            borders = wg.share_borders(len(c.data), sp)
            assert len(borders) == sp - 1
            crossing = [sum(1 for p, _, d in ms if p >= b > p - d) for b in borders]
            print("level %d %s SP=%d: matches with their source across borders %s: %s" % (level, c.name, sp, borders, crossing))
            assert min(crossing) >= 8, (c.name, level, sp, crossing)
    print("level %d: %d matches at distance 32768" % (level, at_window))
    assert at_window >= 1 and beyond == 0


@pytest.mark.parametrize("level", LEVELS)
def test_border_blocks_have_the_stated_pieces_and_distances(corpus, level):
    by = {c.name: c for c in corpus}
    want = {"b64": 64, "b33": 33, "b17": 17, "b9": 9}
    for name, n, period, _ in wg.BORDER_BLOCKS:
        c = by[name]
        assert len(c.data) == n and wg.npieces(n) == want[name.split("_")[0]]
        ms = stream(c, level)[1].all_matches()
        assert sum(1 for _, _, d in ms if d == period) >= 8, (name, level)


@pytest.mark.parametrize("level", LEVELS)
def test_fallbacks_are_what_they_say(corpus, level):
    by = {c.name: c for c in corpus}
    for name in ("noise_65536", "noise_65535", "noise_1024"):
        m, st = stream(by[name], level)
        assert all(b.kind == "stored" for b in st.blocks), name
        assert len(m) == len(by[name].data) + 5 * len(st.blocks)
    assert len(stream(by["zeros_65536"], level)[1].blocks) == 1
    tail = stream(by["cut7_noise_tail"], level)[1]
    print("level %d cut7_noise_tail: %d DEFLATE blocks" % (level, len(tail.blocks)))
    assert len(tail.blocks) > EW_SLOTS
    assert len(stream(by["fib_lits"], level)[1].blocks) == 1


@pytest.mark.parametrize("level", (3, 6))
def test_rooms_of_the_verdict_in_round_two_exist(corpus, level):
    """the three rooms test_gpu_wg_per_block.py gives a 7-block member: it fits its own length exactly; one byte less
    and the room in which its FIFTH block does not end both answer non-zero"""
    c = {c.name: c for c in corpus}["cut7"]
    m, st = stream(c, level)
    assert len(st.blocks) == 7
    r, again = hdtest.codec_twin(c.data, level, cap=len(m))
    assert r == 0 and again == m
    room5 = fifth_block_room(m)
    assert (st.blocks[3].end_bit + 7) // 8 <= room5 < len(m) - 1, "the first round fits, the second does not"
    for room in (len(m) - 1, room5):
        r, out = hdtest.codec_twin(c.data, level, cap=room)
        assert r != 0 and out == b"", (level, room)
