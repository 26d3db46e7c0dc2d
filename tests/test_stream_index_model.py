"""The model of the stream index (tests/stream_index_model.py) held to zlib: on streams zlib writes with Z_FULL_FLUSH at
uneven cuts the chain from candidate 0 gives the offsets the writer recorded, the pieces concatenate to what
zlib.decompress gives, and the check of the decode is zlib's.  No GPU."""
import random
import zlib

import pytest

import stream_index_model as m

FRAMES = (m.FRAME_RAW, m.FRAME_ZLIB, m.FRAME_GZIP)


def _data(n, seed=1):
    rng = random.Random(seed)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


DATA = _data(300000)


def _decompress(stream, frame):
    return zlib.decompress(stream, m.WBITS[frame])


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("level", (1, 6, 9))
def test_full_flush_stream_of_one_writer(frame, level):
    cuts = [0, 70000, 70001, 200000, 200017, 300000]
    pieces = [DATA[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    stream, off = m.writer(pieces, frame, level)
    s, in_off, in_len, out_size, out_off = m.index(stream, frame)
    assert s["status"] == 0 and in_off == off and out_size == [len(p) for p in pieces]
    assert s == {"nchunks": len(pieces), "out_bytes": len(DATA), "end_offset": len(stream), "ncandidates": len(pieces),
                 "hdr_bytes": len(m.HEADER[frame]), "status": 0}
    assert [a + b for a, b in zip(in_off, in_len)][:-1] == in_off[1:]
    d, out = m.decode(stream, frame, in_off, in_len, out_size, out_off)
    assert out == _decompress(stream, frame) == DATA
    want = zlib.adler32(DATA) if frame == m.FRAME_ZLIB else zlib.crc32(DATA)
    assert d == {"out_bytes": len(DATA), "in_bytes": len(stream), "bad_chunk": len(pieces), "nchunks": len(pieces),
                 "check": want, "status": 0}


def six_pieces():
    """70000, 1, 0 and 129999 bytes, a level-0 piece whose payload is 50 markers, 500 noise bytes and one more marker, and a
    final piece of 100000 bytes"""
    rng = random.Random(2)
    stored = m.MARKER * 50 + bytes(rng.randrange(256) for _ in range(500)) + m.MARKER
    return [DATA[:70000], DATA[70000:70001], b"", DATA[70001:200000], (stored, 0), DATA[200000:]]


@pytest.mark.parametrize("frame", FRAMES)
def test_six_pieces_and_fifty_one_decoys(frame):
    stream, off, plain = m.compose(six_pieces(), frame)
    assert _decompress(stream, frame) == plain
    s, in_off, in_len, out_size, out_off = m.index(stream, frame)
    assert s["status"] == 0 and s["nchunks"] == 6 and s["end_offset"] == len(stream)
    assert in_off == off and out_size == [70000, 1, 0, 129999, 704, 100000]
    cand = m.candidates(stream, frame, s["hdr_bytes"])
    false = [c for c in cand if c not in off]
    # the 51 markers of the stored payload, and whatever the noise and the coded bytes hold by chance
    assert s["ncandidates"] == len(cand) and len(false) >= 51 and not set(false) & set(in_off)
    d, out = m.decode(stream, frame, in_off, in_len, out_size, out_off)
    assert d["status"] == 0 and out == plain
    assert d["check"] == (zlib.adler32(plain) if frame == m.FRAME_ZLIB else zlib.crc32(plain))


def test_two_flushes_in_a_row_are_a_row_of_size_zero():
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    assert c.flush(zlib.Z_FULL_FLUSH) == bytes.fromhex("000000ffff")
    v, stop, used, size, blocks = m.piece(bytes.fromhex("000000ffff0300"), 0, 7)
    assert (v, stop, used, size) == (m.OK, m.FLUSH, 5, 0) and blocks[0].sync_flush
    assert m.piece(bytes.fromhex("000000ffff0300"), 5, 2)[:4] == (m.OK, m.FINAL, 2, 0)


def test_sync_flush_that_carries_the_window_is_bad_from_its_start():
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    part = DATA[:5000]
    a = c.compress(part) + c.flush(zlib.Z_SYNC_FLUSH)
    stream = a + c.compress(part) + c.flush()
    assert zlib.decompress(stream, -15) == part + part
    s, in_off, in_len, out_size, _ = m.index(stream, m.FRAME_RAW)
    assert (s["status"], s["nchunks"], s["end_offset"]) == (1, 1, len(a)) and (in_off, in_len, out_size) == ([0], [len(a)], [5000])


@pytest.mark.parametrize("frame", FRAMES)
def test_every_truncation_is_cut_or_refused(frame):
    pieces = [DATA[:300], DATA[300:301], DATA[301:900]]
    stream, off = m.writer(pieces, frame)
    ends = off[1:] + [len(stream) - m.TRAILER[frame]]
    for n in range(len(stream)):
        s, in_off, _, _, _ = m.index(stream[:n], frame)
        assert s["status"] == 2, (n, s)                                  # a prefix of a valid stream is never bad data
        # the rows are the pieces that lie whole in front of the cut payload's end
        assert in_off == [o for o, e in zip(off, ends) if e <= n - m.TRAILER[frame]], (n, s)
    assert m.index(stream, frame)[0]["status"] == 0


def test_bounds_and_table_size():
    stream, off = m.writer([DATA[:4000], DATA[4000:9000], DATA[9000:9500]], m.FRAME_ZLIB)
    s, in_off, in_len, _, _ = m.index(stream, m.FRAME_ZLIB)
    assert s["status"] == 0
    assert m.index(stream, m.FRAME_ZLIB, max_chunks=2)[0] == dict(s, status=3, out_bytes=9000)
    assert m.index(stream, m.FRAME_ZLIB, max_chunk_in=in_len[1])[0]["status"] == 0
    t = m.index(stream, m.FRAME_ZLIB, max_chunk_in=in_len[1] - 1)[0]
    assert (t["status"], t["nchunks"], t["end_offset"]) == (1, 1, off[1])
    # bytes behind the trailer are not looked at
    u = m.index(stream + b"\x1f\x8b\x08\x00junk", m.FRAME_ZLIB)[0]
    assert u["status"] in (0, 2) and (u["status"] != 0 or u["end_offset"] == len(stream))


def test_decode_verdicts():
    pieces = [DATA[:4000], DATA[4000:9000], DATA[9000:9500]]
    stream, off = m.writer(pieces, m.FRAME_GZIP)
    s, in_off, in_len, out_size, out_off = m.index(stream, m.FRAME_GZIP)
    n = len(in_off)
    assert m.decode(stream, m.FRAME_GZIP, in_off, in_len, out_size, out_off, 9499)[0] == {
        "out_bytes": 9500, "in_bytes": 0, "bad_chunk": n, "nchunks": n, "check": None, "status": 3}
    swapped = [in_off[1], in_off[0]] + in_off[2:]
    assert m.decode(stream, m.FRAME_GZIP, swapped, in_len, out_size, out_off)[0]["status"] == 1
    bad = bytearray(stream)
    bad[-6] ^= 1
    d = m.decode(bytes(bad), m.FRAME_GZIP, in_off, in_len, out_size, out_off)[0]
    assert (d["status"], d["bad_chunk"]) == (2, n)
    assert m.decode(stream, m.FRAME_GZIP, [], [], [], [])[0]["status"] == 1
