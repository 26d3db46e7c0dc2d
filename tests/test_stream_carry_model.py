"""The carry model (tests/stream_carry_model.py) against zlib: both writers of streams that carry the window across their
flush points, in all three frames; against stream_index_model on streams that do not carry it; and the hand-built rows."""
import zlib

import numpy as np
import pytest

import deflate_gen as dg
import stream_carry_model as cm
import stream_index_model as sm

FRAMES = (sm.FRAME_RAW, sm.FRAME_ZLIB, sm.FRAME_GZIP)
WRITERS = (cm.sync_writer, cm.pigz_writer)


@pytest.fixture(scope="module")
def text():
    return cm.words(np.random.default_rng(7), 150000)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("level", (1, 6))
def test_writers_give_valid_streams_and_the_model_decodes_them(text, writer, frame, level):
    pieces = cm.cut(text, [1, 100, 4096, 40000, 10, 70000])
    stream = writer(pieces, frame, level)
    assert zlib.decompress(stream, sm.WBITS[frame]) == text
    s, in_off, in_len, out_size, out_off, reach = cm.index_carry(stream, frame)
    assert s["status"] == 0 and s["nchunks"] == len(pieces) and s["out_bytes"] == len(text) and s["end_offset"] == len(stream)
    assert out_size == [len(p) for p in pieces]
    assert reach[0] == 0 and max(reach) > 0 and all(r <= min(o, cm.WINDOW) for r, o in zip(reach, out_off))
    v, out = cm.decode_carry(stream, frame, in_off, in_len, out_size, out_off, reach)
    assert v["status"] == 0 and out == text and v["in_bytes"] == len(stream) and v["bad_chunk"] == len(pieces)
    assert v["check"] == (zlib.adler32(text) if frame == sm.FRAME_ZLIB else zlib.crc32(text))


@pytest.mark.parametrize("frame", FRAMES)
def test_equals_the_index_model_on_full_flush_streams(text, frame):
    stream, _ = sm.writer(cm.cut(text, [5000, 1, 70000]), frame)
    want = sm.index(stream, frame)
    got = cm.index_carry(stream, frame)
    assert got[:5] == want and got[5] == [0] * len(want[1])
    for cap in (0, 1, 2):
        want, got = sm.index(stream, frame, max_chunks=cap), cm.index_carry(stream, frame, max_chunks=cap)
        assert got[:5] == want and got[0]["status"] == 3


@pytest.mark.parametrize("writer", WRITERS)
def test_the_old_index_stops_at_the_first_row_that_reaches_back(text, writer):
    stream = writer(cm.cut(text, [3000]), sm.FRAME_GZIP)
    old = sm.index(stream, sm.FRAME_GZIP)[0]
    s, in_off, _, _, _, reach = cm.index_carry(stream, sm.FRAME_GZIP)
    first = min(i for i, r in enumerate(reach) if r > 0)
    assert old["status"] == 1 and old["end_offset"] == in_off[first] and old["nchunks"] == first and s["status"] == 0


def test_reach_rule_and_its_small_table_clause():
    rng = np.random.default_rng(3)
    lead = [int(x) for x in rng.integers(0, 256, 40)]
    rows = [[dg.Block("static", lead)], [dg.Block("static", [65, (10, 40), 66])], [dg.Block("static", [(5, 43), 67], final=True)]]
    stream, plain = cm.compose_rows(rows, sm.FRAME_ZLIB)
    assert zlib.decompress(stream) == plain
    s, in_off, in_len, out_size, out_off, reach = cm.index_carry(stream, sm.FRAME_ZLIB)
    assert s["status"] == 0 and reach == [0, 39, 43] and out_off == [0, 40, 52]
    # a first row that reaches back, and a later one that reaches over the start of the stream
    body = dg.encode([dg.Block("static", [65, (3, 2), 66])], chunk=True) + dg.encode([dg.Block("static", [67], final=True)])
    s0 = cm.index_carry(body, sm.FRAME_RAW)
    assert s0[0]["status"] == 1 and s0[0]["nchunks"] == 0 and s0[0]["end_offset"] == 0
    body = dg.encode([dg.Block("static", lead)], chunk=True)
    body1 = dg.encode([dg.Block("static", [65, (3, 42)])], chunk=True)
    body2 = dg.encode([dg.Block("static", [67], final=True)])
    stream = body + body1 + body2
    s1 = cm.index_carry(stream, sm.FRAME_RAW)
    assert s1[0] == {"nchunks": 1, "out_bytes": 40, "end_offset": len(body), "ncandidates": 3, "hdr_bytes": 0, "status": 1}
    assert s1[1] == [0] and s1[5] == [0]
    # the table too small: the rule is applied to the rows it holds
    assert cm.index_carry(stream, sm.FRAME_RAW, max_chunks=1)[0]["status"] == 3
    assert cm.index_carry(stream, sm.FRAME_RAW, max_chunks=1)[0]["nchunks"] == 3
    assert cm.index_carry(stream, sm.FRAME_RAW, max_chunks=2)[0] == s1[0]


def test_decode_verdicts_in_the_headers_order(text):
    stream = cm.pigz_writer(cm.cut(text[:30000], [10000]), sm.FRAME_GZIP)
    s, in_off, in_len, out_size, out_off, reach = cm.index_carry(stream, sm.FRAME_GZIP)
    t = (in_off, in_len, out_size, out_off, reach)
    assert s["status"] == 0 and reach[1] > 0

    def run(k, i, v, **kw):
        u = [list(x) for x in t]
        u[k][i] = v
        return cm.decode_carry(stream, sm.FRAME_GZIP, *u, **kw)[0]
    assert run(4, 1, reach[1] - 1)["status"] == 2 and run(4, 1, reach[1] - 1)["bad_chunk"] == 1
    assert run(4, 1, 32769)["status"] == 1 and run(4, 1, out_off[1] + 1)["status"] == 1 and run(4, 0, 1)["bad_chunk"] == 0
    assert (run(1, 1, in_len[1] - 1)["status"], run(1, 1, in_len[1] - 1)["bad_chunk"]) == (2, 1)
    assert (run(3, 2, out_off[2] + 1)["status"], run(3, 2, out_off[2] + 1)["bad_chunk"]) == (1, 1)
    assert run(4, 1, out_off[1], out_cap=29999)["status"] == 3 and run(4, 1, out_off[1], out_cap=30000)["status"] == 0
    bad = bytearray(stream)
    bad[-5] ^= 1
    v, _ = cm.decode_carry(bytes(bad), sm.FRAME_GZIP, *t)
    assert v["status"] == 2 and v["bad_chunk"] == len(in_off)
