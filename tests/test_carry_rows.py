"""tests/carry_rows.py pinned on the CPU: every composed stream decodes to the token lists' bytes -- by zlib where zlib takes
the form, by the second reader (deflate_tokens.read) where it does not and on a stride of the rest -- both plain-Python
models take it whole with the table the token lists give, and the streams reach the edges they are built for, counted from the token lists by name.
tests/test_gpu_carry_rows.py puts the same streams through the kernels."""
import collections
import zlib

import pytest

import carry_rows as cr
import deflate_gen as dg
import deflate_tokens
import hdtest
import stream_carry_model as cm
import stream_index_model as m

RAW, ZLIB, GZIP = m.FRAME_RAW, m.FRAME_ZLIB, m.FRAME_GZIP


def pin(c, frame, second_reader=True):
    """one composed stream: the bytes, the index with the token lists' table, the decode on it.  The bytes by zlib where
    zlib takes the form; by the second reader where it does not, and where the caller asks (it is plain Python: a stride)"""
    stream = c.compose(frame)
    if c.zlib:
        assert zlib.decompress(stream, m.WBITS[frame]) == c.plain, c.name
    else:
        with pytest.raises(zlib.error):
            zlib.decompress(stream, m.WBITS[frame])
    if second_reader or not c.zlib:
        body = stream[len(m.HEADER[frame]):len(stream) - m.TRAILER[frame]]
        assert deflate_tokens.read(body, wide=True).out == c.plain, c.name
    sizes, reach = c.table()
    x, *t = cm.index_carry(stream, frame)
    assert (x["status"], x["nchunks"], x["out_bytes"], x["end_offset"]) == (0, len(sizes), len(c.plain), len(stream)), c.name
    assert t[2] == sizes and t[4] == reach, c.name
    d, out = cm.decode_carry(stream, frame, *t, plain=None if c.zlib else c.plain)
    assert d["status"] == 0 and out == c.plain, c.name
    return sizes, reach


@pytest.mark.parametrize("key,frame", (("every", GZIP), ("mid", ZLIB)))
def test_cut_streams(key, frame):
    streams, single = cr.cached(key)
    names = {c.name for c in streams}
    rows = nreach = nlong = 0
    for k, c in enumerate(streams):
        sizes, reach = pin(c, frame, k % 4 == 0)
        assert len(sizes) > 1, c.name
        rows += len(sizes)
        nreach += sum(1 for r in reach if r)
        nlong += sum(1 for s in sizes if s > cr.W)
    print("%s: %d streams, %d rows, %d reach back, %d longer than the window, %d cases give one row" %
          (key, len(streams), rows, nreach, nlong, len(single)))
    # the floors: conditions, not what the code gives (measured on the corpus as it stood when they were set)
    assert len(streams) >= 385 and len(single) <= 70
    if key == "every":
        assert rows >= 6000 and nreach >= 3500
    else:
        assert nreach >= 300 and nlong >= 20 and all(len(c.rows) == 2 for c in streams)
    for n in ("static_lit286_off0", "static_lit287_off5", "static_lit285_off30", "static_lit257_off31", "static_lit286_off31"):
        assert n in names, n
    # the cases left out have nowhere to cut: no Huffman block behind the stream's first block
    by = {c.name: c for c in dg.cached_corpus()}
    for n in single:
        assert not any(b.kind != "stored" for b in by[n].blocks[1:]), n


def test_cut_every_matrix_rows_are_short_and_marked():
    """a match-matrix case becomes 10..30 short rows, and each row's match is a marker wherever its distance exceeds the
    0, 2, 37 or 300 literals in front of it"""
    streams, _ = cr.cached("every")
    mm = [c for c in streams if c.name.startswith("match_d")]
    assert len(mm) >= 100
    lead = collections.Counter()
    for c in mm:
        assert 2 <= len(c.rows) <= 40, c.name
        for row in c.rows[1:]:
            nl = next(i for i, t in enumerate(row[0].tokens) if not isinstance(t, int))
            ln, d = row[0].tokens[nl][:2]
            if d > nl:
                lead[nl] += 1
    assert sorted(lead) == [0, 2, 37, 300] and min(lead.values()) >= 300, lead
    n = sorted(len(c.rows) for c in mm)
    assert n[len(n) // 2] >= 10, n


def test_carry_ring_streams():
    for k, c in enumerate(cr.cached("ring")):
        pin(c, RAW, k % 4 == 0)
        assert len(c.rows[0]) and all(b.kind == "stored" for b in c.rows[0]) and cr._size(c.rows[0]) >= cr.LEAD_BYTES, c.name


def test_literal_tails():
    c = cr.literal_tails()
    sizes, reach = pin(c, GZIP)
    assert sizes == [1000, 450, 380, 3] and reach == [0, 900, 490, 1]


def test_carry_ring_is_deterministic():
    import numpy as np
    a, b = cr.cached("ring"), cr.carry_ring(np.random.default_rng(2028))
    assert [(c.name, c.compose(RAW)) for c in a] == [(c.name, c.compose(RAW)) for c in b]
    assert len({c.name for c in a}) == len(a) and sum(len(c.plain) for c in a) <= 48 << 20


# what carry_ring must keep reaching, by name, counted from the token lists as they are written (carry_rows._row_stats)
RING_COVERAGE = {
    "ring_dA_32768": 210, "ring_dB_32768": 210,                      # every (length, distance) across row position 32768, both phases
    **{"ring_%s_%d" % (k, w): 8 for w in (32768, 65536) for k in ("d0", "d1", "sA", "sB", "s0", "s1")},
    "ring_dA_65536": 8, "ring_dB_65536": 8,
    "ring_dst_across_32768": 420, "ring_dst_across_65536": 16, "ring_src_across_32768": 24, "ring_src_across_65536": 24,
    "straddle_row_start": 80, "straddle_row_start_overlap": 30, "straddle_row_start_plain": 30,
    "straddle_p_1_257": 60, "straddle_p_32511_32767": 5,
    **{"literal_behind_far_%d" % k: 4 for k in cr.FAR_K}, **{"literal_behind_far_%d_in_ring" % k: 4 for k in cr.FAR_K},
    **{"all_markers_row_%d" % s: 2 for s in cr.ALL_MARKER_SIZES}, "row_of_1_byte": 1,
    **{"source_slot_%d_back_%d" % (s, b): 1 for s in (0, 1, 32767) for b in (1, 32768)}, "source_first_tail_slot_back_1": 1,
    "long_code_row_13bit": 1, "long_code_row_14bit": 1, "long_code_row_15bit": 1,
    **{"long_code_marker_matches_%dbit" % L: 4 for L in (13, 14, 15)},     # (the four the builder plants at the run's head)
}


def test_carry_ring_coverage():
    ring = cr.cached("ring")
    tot = collections.Counter()
    for c in ring:
        tot.update(c.stats)
    short = {k: (tot.get(k, 0), n) for k, n in RING_COVERAGE.items() if tot.get(k, 0) < n}
    assert not short, short
    pairs = {(ln, d): tot["ring_pair_%d_%d" % (ln, d)] for ln in dg.MATCH_LENGTHS for d in cr.RING_DISTS}
    assert len(pairs) == 210 and min(pairs.values()) == 2, {k: v for k, v in pairs.items() if v != 2}
    # what is counted above is counted on the device only where the row goes through the carry kernels: every row with a
    # match lies in a group whose largest reach is > 0, at both group sizes the GPU test runs the family at
    for c in ring:
        sizes, reach = c.table()
        assert len(sizes) == len(c.rows), c.name
        for group in (0, 65536):
            path = cr.marker_path_rows(sizes, reach, group)
            for i, row in enumerate(c.rows):
                if i and any(not isinstance(t, int) for b in row if b.kind != "stored" for t in b.tokens):
                    assert path[i], (c.name, i, group)
    by = {c.name: c for c in ring}
    # the ring-wrap rows reach back each by itself: a row of 70,001 bytes is a group of its own at 65,536
    for c in ring:
        if c.name.startswith("ring_wrap_"):
            assert min(c.table()[1][1:]) >= 300, c.name
    # the marker-source streams put the row where its name says: (row start - backdist) mod 32768
    for slot in (0, 1, 32767):
        for back in (1, 32768):
            c = by["ring_source_slot_%d_back_%d" % (slot, back)]
            start = cr._size(c.rows[0])
            assert (start - back) % cr.W == slot and c.table()[1][-1] == back, c.name
    c = by["ring_source_first_tail_slot_back_1"]
    start, size = cr._size(c.rows[0]), cr._size(c.rows[1])
    assert size == 65535 and (start - 1) % cr.W == (start + size - cr.W) % cr.W
    # the all-marker rows: nothing but (length, 32768); every thread and register slot of k_carry_tails holds a marker from
    # 32768 symbols on (symbol k: thread k mod 1024, 16-bit half (k / 1024) & 1, byte (k / 1024) & 3)
    for s in cr.ALL_MARKER_SIZES:
        c = by["ring_all_markers_%d" % s]
        sizes, reach = c.table()
        assert sizes[1:] == [s, 5, 0, 300, s, 3] and reach[1] == reach[5] == cr.W, c.name
        assert all(t[1] == cr.W for i in (1, 5) for t in c.rows[i][0].tokens)
    # the long-code rows: a stored block of 65,535 bytes behind the run, marker matches in the run and in the next row's
    c = by["ring_long_codes"]
    for row in c.rows[1:]:
        assert [b.kind for b in row] == ["dynamic", "stored", "dynamic"] and len(row[1].data) == 65535
        assert max(row[0].lit_lens) in (13, 14, 15)
    assert min(c.table()[1][1:]) > 0


def test_fault_rows():
    """every member of the faults family as row 1 behind a row of 100 literals: the chain ends at row 1 with the verdict the
    model gives the fault stream alone; the claimed table is refused at row 1 (status 2) -- but for dist_past_out_*, whose
    one match reaches into the lead: valid there, and the bytes are those of the token lists"""
    n = 0
    for c in dg.cached_corpus():
        if c.family != "faults":
            continue
        n += 1
        r, out = hdtest.oracle_inflate(c.stream, 1 << 21)
        f = cr.fault_row(c, len(out) if r == dg.OK else None)
        x, *t = cm.index_carry(f.stream, RAW)
        alone = cm.index_carry(c.stream, RAW)[0]
        if f.plain is not None:
            assert x["status"] == 0 and x["out_bytes"] == len(f.plain), c.name
            assert t[2][0] == 100 and sum(t[2][1:]) == f.table[2][1] and max(t[4]) == 1, c.name
            d, out = cm.decode_carry(f.stream, RAW, *f.table)
            assert d["status"] == 0 and out == f.plain, c.name
            continue
        assert x["status"] == (alone["status"] or 0) and x["nchunks"] == 1 + alone["nchunks"], c.name
        if c.code == dg.INSUFFICIENT_SPACE:
            assert x["status"] == 0 and f.table[2][1] == t[2][1] - 1, c.name          # a good row in a room one byte short
        else:
            assert x["status"] in (1, 2) and x["end_offset"] == f.table[0][1] + alone["end_offset"], c.name
        d, out = cm.decode_carry(f.stream, RAW, *f.table)
        assert (d["status"], d["bad_chunk"]) == (2, 1), c.name
    assert n >= 60
