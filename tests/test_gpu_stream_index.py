"""The stream index and the decode on its table -- hipdeflate_stream_index_dev, hipdeflate_stream_inflate_table_dev,
hip_inflate_stream and their device.py forms -- against the plain-Python model of tests/stream_index_model.py.  Bit-exact:
the four tables, every field of both summaries, the bytes, 64 sentinel bytes around every output and one sentinel row
around every table; hipdeflate_stall_count() stays 0.  No case provokes a fault: every refusal is a verdict the contract of
include/hipdeflate.h defines, each runs once, and none reads or writes outside its buffers.

Where the cases land (hd_stream.hpp, hd_index.hpp, hd_inflate_size.hpp):
  * own streams: every frame, levels 1 / 2 / 6, chunks of 16, 4096 and 65536 bytes, lengths around one chunk and 3 chunks + 1;
    5,000 chunks of 16 bytes (a chain longer than a scan tile, 13 rounds of pointer doubling); chunks above HD_SEG_LIMIT,
    which levels 1 and 2 code in segments;
  * a stream of another writer with a 1-byte piece, two flushes in a row, a level-0 piece and a final piece with output;
  * a marker at each of the 16 offsets of a granule, across a 1 KiB bitmap word (IDX_WORD) and across a 256 KiB tile
    (IDX_TILE), as a true flush point and as a decoy; a marker on the last payload byte; a marker that runs into the trailer;
  * 70,000 markers in a row, a decoy directly in front of a true flush point, an empty final stored block;
  * the refusals the header names."""
import importlib
import os
import random
import zlib

import numpy as np
import pytest

import framed_gen
import hdtest
import stream_index_model as m

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0xa5
RAW, ZLIB, GZIP = m.FRAME_RAW, m.FRAME_ZLIB, m.FRAME_GZIP
FRAMES = (RAW, ZLIB, GZIP)
X_FIELDS = ("nchunks", "out_bytes", "end_offset", "ncandidates", "hdr_bytes", "status")
S_FIELDS = ("out_bytes", "in_bytes", "bad_chunk", "nchunks", "check", "status")
IDX_WORD, IDX_TILE = 1024, 1024 * 256              # hd_index.hpp


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
    assert pkg.lib().hipdeflate_stall_count() == 0


_text = {}


def text(n, seed=1):
    """n bytes of words, shared and never modified"""
    if seed not in _text:
        rng = random.Random(seed)
        words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 9))) for _ in range(300)]
        out = bytearray()
        while len(out) < 400000:
            out += rng.choice(words) + b" "
        _text[seed] = bytes(out)
    assert n <= len(_text[seed])
    return _text[seed][:n]


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def u32(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32).copy()).cuda()


def u64(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


def fields(s, names):
    return {f: getattr(s, f) for f in names}


def index_check(torch, dev, stream, frame, max_chunks=None, max_chunk_in=0):
    """one hipdeflate_stream_index_dev held to the model: the summary, the rows, and a sentinel row either side of each
    table -> (the model's summary, its four tables)"""
    want = m.index(stream, frame, max_chunks, max_chunk_in)
    rows = len(want[1])
    cap = rows if max_chunks is None else max_chunks
    tabs = [torch.full((cap + 2,), -2, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int32, torch.int64)]
    s = dev.index_stream_call(to_dev(torch, stream), frame, cap, max_chunk_in, *(t[1:] for t in tabs))
    assert fields(s, X_FIELDS) == want[0]
    for t, w, mask in zip(tabs, want[1:], (None, 0xffffffff, 0xffffffff, None)):
        got = t.cpu().tolist()
        assert got[0] == -2 and got[rows + 1:] == [-2] * (cap + 1 - rows)
        assert [v & mask if mask else v for v in got[1:rows + 1]] == w
    return want


def decode_check(torch, dev, stream, frame, in_off, in_len, out_size, out_off, cap=None):
    """one hipdeflate_stream_inflate_table_dev held to the model's verdict, 64 sentinel bytes either side of the output"""
    want, out = m.decode(stream, frame, in_off, in_len, out_size, out_off, cap)
    room = (out_off[-1] + out_size[-1] if in_off else 0) if cap is None else cap
    room = min(room, 1 << 24)                                                  # (a table that claims more is refused before any use)
    buf = torch.full((GUARD + room + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_table_call(to_dev(torch, stream), frame, u64(torch, in_off), u32(torch, in_len), u32(torch, out_size),
                                      u64(torch, out_off), len(in_off), buf[GUARD:], room if cap is None else cap)
    got = fields(s, S_FIELDS)
    if want["check"] is None:
        got["check"] = None
    assert got == want
    b = bytes(buf.cpu().numpy())
    assert b[:GUARD] == bytes([SENT]) * GUARD and b[GUARD + room:] == bytes([SENT]) * GUARD
    if want["status"] in (1, 3):                                               # nothing is inflated
        assert b[GUARD:GUARD + room] == bytes([SENT]) * room
    if want["status"] == 0:
        assert b[GUARD:GUARD + room] == out
    return want


def both(torch, dev, stream, frame, plain=None):
    """the index, then the decode on its table where the index is satisfied"""
    x, in_off, in_len, out_size, out_off = index_check(torch, dev, stream, frame)
    if x["status"] == 0:
        d = decode_check(torch, dev, stream, frame, in_off, in_len, out_size, out_off)
        if plain is not None:
            assert d["status"] == 0 and d["out_bytes"] == len(plain)
    return x, in_off, in_len, out_size, out_off


# ---- own streams -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", (16, 4096, 65536))
@pytest.mark.parametrize("level", (1, 2, 6))
@pytest.mark.parametrize("frame", FRAMES)
def test_own_streams(torch, dev, frame, level, chunk):
    for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 1):
        data = text(n)
        strm, chunk_off, s = dev.deflate_stream(to_dev(torch, data), level, frame, chunk)
        stream = bytes(strm.cpu().numpy())
        x, in_off, in_len, out_size, _ = both(torch, dev, stream, frame, data)
        assert x["status"] == 0 and x["end_offset"] == len(stream)
        assert in_off == chunk_off.cpu().tolist() and x["nchunks"] == s.nchunks + 1
        assert out_size == [len(data[i:i + chunk]) for i in range(0, n, chunk)] + [0] and in_len[-1] == 2
        out, xs = dev.inflate_stream_auto(to_dev(torch, stream), frame)
        assert bytes(out.cpu().numpy()) == data and fields(xs, X_FIELDS) == x


def test_five_thousand_chunks(torch, dev):
    data = text(5000 * 16)
    strm, chunk_off, s = dev.deflate_stream(to_dev(torch, data), 1, GZIP, 16)
    stream = bytes(strm.cpu().numpy())
    x, in_off, _, _, _ = both(torch, dev, stream, GZIP, data)
    assert x["nchunks"] == 5001 and in_off == chunk_off.cpu().tolist()
    out, _ = dev.inflate_stream_auto(to_dev(torch, stream), GZIP)
    assert bytes(out.cpu().numpy()) == data


def test_chunks_the_encoder_codes_in_segments(torch, dev):
    """levels 1..2 code a chunk longer than HD_SEG_LIMIT (320 KiB) as full-flush segments: every segment is a row, and the
    encoder's chunk_off is a subsequence of in_off"""
    data, chunk = text(400000), 327680 + 16
    for level in (1, 2):
        strm, chunk_off, s = dev.deflate_stream(to_dev(torch, data), level, ZLIB, chunk)
        stream = bytes(strm.cpu().numpy())
        x, in_off, _, out_size, out_off = both(torch, dev, stream, ZLIB, data)
        assert x["status"] == 0 and x["nchunks"] > s.nchunks + 1 and set(chunk_off.cpu().tolist()) <= set(in_off)
        assert [out_off[in_off.index(o)] for o in chunk_off.cpu().tolist()] == [0, chunk, len(data)]
        out, _ = dev.inflate_stream_auto(to_dev(torch, stream), ZLIB)
        assert bytes(out.cpu().numpy()) == data


# ---- streams of another writer -------------------------------------------------------------------------------------------

def foreign_pieces():
    rng = random.Random(2)
    stored = m.MARKER * 50 + bytes(rng.randrange(256) for _ in range(500)) + m.MARKER
    t = text(300000)
    return [t[:70000], t[70000:70001], b"", t[70001:200000], (stored, 0), t[200000:]]


@pytest.mark.parametrize("frame", FRAMES)
def test_foreign_stream(torch, dev, frame):
    """zlib, Z_FULL_FLUSH at uneven cuts: a 1-byte piece, two flushes in a row, a level-0 piece full of markers, and
    Z_FINISH with input still left"""
    stream, off, plain = m.compose(foreign_pieces(), frame)
    assert zlib.decompress(stream, m.WBITS[frame]) == plain
    x, in_off, _, out_size, _ = both(torch, dev, stream, frame, plain)
    assert x["status"] == 0 and in_off == off and out_size == [70000, 1, 0, 129999, 704, 100000] and x["ncandidates"] >= 57
    stream, off = m.writer([plain[:70000], plain[70000:70001], plain[70001:200000], plain[200000:]], frame)
    x, in_off, _, _, _ = both(torch, dev, stream, frame, plain)
    assert x["status"] == 0 and in_off == off
    out, _ = dev.inflate_stream_auto(to_dev(torch, stream), frame)
    assert bytes(out.cpu().numpy()) == plain


# ---- scan granule edges -----------------------------------------------------------------------------------------------------

def stored(payload, final=False):
    """stored blocks of at most 65535 bytes; final marks the last"""
    out, parts = b"", [payload[i:i + 65535] for i in range(0, len(payload), 65535)] or [b""]
    for i, p in enumerate(parts):
        out += bytes([1 if final and i + 1 == len(parts) else 0]) + len(p).to_bytes(2, "little") + (len(p) ^ 0xffff).to_bytes(2, "little") + p
    return out


FLUSH_BLOCK = bytes.fromhex("000000ffff")


def padded_flush(at):
    """a piece of stored padding whose true flush marker's first byte is stream byte `at` of a raw stream"""
    n = at - 1 - 5
    while True:
        piece = stored(bytes([0x55]) * n) + FLUSH_BLOCK
        if len(piece) - 4 == at:
            return piece, n
        n -= (len(piece) - 4) - at


def padded_decoy(at):
    """a piece of stored padding that holds a marker whose first byte is stream byte `at`, then the true flush"""
    n = at + 4000
    body = bytearray(stored(bytes([0x55]) * n))
    body[at:at + 4] = m.MARKER
    # (the four bytes must be payload, not a block header: the padding's headers are 65540 bytes apart)
    assert all(not (h <= at + 3 and at <= h + 4) for h in range(0, len(body), 65540))
    return bytes(body) + FLUSH_BLOCK, n


@pytest.mark.parametrize("kind", ("true", "decoy"))
@pytest.mark.parametrize("base", (96, IDX_WORD, IDX_TILE))
def test_marker_at_every_granule_offset(torch, dev, base, kind):
    tail = zlib.compressobj(6, zlib.DEFLATED, -15)
    last = tail.compress(text(3000)) + tail.flush()
    for k in range(16):
        at = base - 8 + k                              # the 16 offsets of a granule; k = 5..7 straddle the base
        piece, n = (padded_flush if kind == "true" else padded_decoy)(at)
        stream = piece + last
        assert stream[at:at + 4] == m.MARKER
        x, in_off, _, out_size, _ = both(torch, dev, stream, RAW)
        assert x["status"] == 0 and in_off == [0, len(piece)] and out_size == [n, 3000]
        assert x["ncandidates"] == (2 if kind == "true" else 3)


@pytest.mark.parametrize("frame", FRAMES)
def test_marker_on_the_last_payload_byte_and_into_the_trailer(torch, dev, frame):
    hdr = m.HEADER[frame]
    # a flush point is the payload's last byte: no candidate behind it, the stream is cut there
    piece = stored(text(100)) + FLUSH_BLOCK
    stream = hdr + piece + bytes(m.TRAILER[frame])
    x = index_check(torch, dev, stream, frame)
    assert (x[0]["status"], x[0]["ncandidates"], x[0]["nchunks"], x[0]["end_offset"]) == (2, 1, 1, len(hdr) + len(piece))
    # the final block's payload ends in 00 00 and the trailer goes on with ff ff: not a candidate
    body = stored(text(50) + b"\0\0", final=True)
    stream = hdr + body + (b"\xff\xff" + bytes(m.TRAILER[frame]))[:m.TRAILER[frame]]
    x = index_check(torch, dev, stream, frame)
    assert (x[0]["status"], x[0]["ncandidates"], x[0]["nchunks"]) == (0, 1, 1)
    if frame != RAW:
        assert stream[len(hdr) + len(body) - 2:][:4] == m.MARKER


# ---- decoys ----------------------------------------------------------------------------------------------------------------

def test_seventy_thousand_markers(torch, dev):
    plain_tail = text(5000)
    stream, off, plain = m.compose([(m.MARKER * 70000, 0), plain_tail], GZIP)
    x, in_off, _, out_size, _ = both(torch, dev, stream, GZIP, plain)
    # (the count itself is the model's, held in index_check; zlib's stored blocks of 65535 bytes split four of the markers)
    assert x["status"] == 0 and in_off == off and out_size == [280000, 5000] and x["ncandidates"] >= 70000 - 4


def test_decoy_in_front_of_a_flush_point_and_an_empty_final_stored_block(torch, dev):
    # the decoy's candidate is the flush block itself: a piece of its own that is not on the chain
    payload = text(999) + m.MARKER
    pieces = [(stored(payload) + FLUSH_BLOCK, payload), (bytes.fromhex("010000ffff"), b"")]
    for frame in FRAMES:
        stream, off, plain = m.compose(pieces, frame, raw_pieces=True)
        assert zlib.decompress(stream, m.WBITS[frame]) == plain
        x, in_off, in_len, out_size, _ = both(torch, dev, stream, frame, plain)
        assert x["status"] == 0 and in_off == off and in_len == [1013, 5] and out_size == [1003, 0]
        assert x["ncandidates"] == 3                    # (the final block's own marker ends on the last payload byte)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_sync_flush_that_carries_the_window(torch, dev, pkg):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    part = text(5000)
    a = c.compress(part) + c.flush(zlib.Z_SYNC_FLUSH)
    stream = a + c.compress(part) + c.flush()
    x, in_off, in_len, out_size, out_off = index_check(torch, dev, stream, RAW)
    assert (x["status"], x["nchunks"], x["end_offset"]) == (1, 1, len(a))
    # row 0 is usable: the flush-rule batch inflate takes it as it stands
    out = torch.full((GUARD + 5000 + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out_len, crc, status = (torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    args = (to_dev(torch, stream), u64(torch, in_off), u32(torch, in_len), out[GUARD:], u64(torch, out_off), u32(torch, out_size))
    rc = pkg.lib().hipdeflate_batch_inflate_flush_dev(
        args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), 1, args[3].data_ptr(), args[4].data_ptr(), args[5].data_ptr(),
        out_len.data_ptr(), crc.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert bytes(out.cpu().numpy()) == bytes([SENT]) * GUARD + part + bytes([SENT]) * GUARD
    assert (int(status[0]), int(out_len[0]), int(crc[0]) & 0xffffffff) == (0, 5000, zlib.crc32(part))


@pytest.mark.parametrize("frame", FRAMES)
def test_every_truncation(torch, dev, frame):
    t = text(80)
    stream, off = m.writer([t[:30], t[30:31], t[31:]], frame)
    assert len(off) == 3 and len(stream) < 160
    for n in range(len(stream)):
        x = index_check(torch, dev, stream[:n], frame)[0]
        assert x["status"] in (1, 2)
    assert index_check(torch, dev, stream, frame)[0]["status"] == 0


def test_table_one_short_and_bound_one_short(torch, dev):
    t = text(9500)
    stream, off = m.writer([t[:4000], t[4000:9000], t[9000:]], ZLIB)
    x, in_off, in_len, _, _ = index_check(torch, dev, stream, ZLIB)
    assert x["status"] == 0 and x["nchunks"] == 3
    assert index_check(torch, dev, stream, ZLIB, max_chunks=2)[0] == dict(x, status=3, out_bytes=9000)
    assert index_check(torch, dev, stream, ZLIB, max_chunks=0)[0] == dict(x, status=3, out_bytes=0)
    assert index_check(torch, dev, stream, ZLIB, max_chunk_in=in_len[1])[0] == x
    y = index_check(torch, dev, stream, ZLIB, max_chunk_in=in_len[1] - 1)[0]
    assert (y["status"], y["nchunks"], y["end_offset"]) == (1, 1, off[1])


def test_flipped_bits(torch, dev):
    t = text(3000)
    stream, off, plain = m.compose([t[:1000], (t[1000:2000], 0), t[2000:]], GZIP)
    x, in_off, in_len, out_size, out_off = index_check(torch, dev, stream, GZIP)
    assert x["status"] == 0
    # in the LEN of the level-0 piece's stored block: the index stops there
    bad = bytearray(stream)
    assert bad[off[1]] == 0 and int.from_bytes(bad[off[1] + 1:off[1] + 3], "little") == 1000
    bad[off[1] + 1] ^= 4
    y = index_check(torch, dev, bytes(bad), GZIP)[0]
    assert (y["status"], y["nchunks"], y["end_offset"]) == (1, 1, off[1])
    # in its payload: every size holds, the check does not
    bad = bytearray(stream)
    bad[off[1] + 5 + 17] ^= 1
    assert index_check(torch, dev, bytes(bad), GZIP)[0] == x
    d = decode_check(torch, dev, bytes(bad), GZIP, in_off, in_len, out_size, out_off)
    assert (d["status"], d["bad_chunk"]) == (2, 3)
    # in a row's size, as a table claims it: that row
    wrong = list(out_size)
    wrong[2] -= 1
    wrong_off = [0, wrong[0], wrong[0] + wrong[1]]
    d = decode_check(torch, dev, stream, GZIP, in_off, in_len, wrong, wrong_off)
    assert (d["status"], d["bad_chunk"]) == (2, 2)
    # in the trailer
    for at in (len(stream) - 8, len(stream) - 1):
        bad = bytearray(stream)
        bad[at] ^= 0x10
        d = decode_check(torch, dev, bytes(bad), GZIP, in_off, in_len, out_size, out_off)
        assert (d["status"], d["bad_chunk"]) == (2, 3)


def test_room_and_tables_the_decode_refuses(torch, dev):
    t = text(9500)
    for frame in FRAMES:
        stream, off = m.writer([t[:4000], t[4000:9000], t[9000:]], frame)
        x, in_off, in_len, out_size, out_off = index_check(torch, dev, stream, frame)
        assert decode_check(torch, dev, stream, frame, in_off, in_len, out_size, out_off, cap=9499)["status"] == 3
        assert decode_check(torch, dev, stream, frame, in_off, in_len, out_size, out_off, cap=9500)["status"] == 0
    swapped = [in_off[1], in_off[0], in_off[2]]
    d = decode_check(torch, dev, stream, GZIP, swapped, in_len, out_size, out_off)
    assert (d["status"], d["bad_chunk"]) == (1, 0)
    for bad_off in ([0, 4000, 9001], [1, 4001, 9001]):
        assert decode_check(torch, dev, stream, GZIP, in_off, in_len, out_size, bad_off)["status"] == 1
    assert decode_check(torch, dev, stream, GZIP, in_off, [in_len[0], in_len[1], len(stream)], out_size, out_off)["status"] == 1
    assert decode_check(torch, dev, stream, GZIP, in_off, [in_len[0], in_len[1], 1 << 28], out_size, out_off)["status"] == 1
    assert decode_check(torch, dev, stream, GZIP, [9] + in_off[1:], in_len, out_size, out_off)["status"] == 1
    assert decode_check(torch, dev, stream, GZIP, [], [], [], [])["status"] == 1
    assert decode_check(torch, dev, b"\x1f\x8b\x07" + stream[3:], GZIP, in_off, in_len, out_size, out_off)["status"] == 1


def test_gzip_headers_and_a_second_member(torch, dev):
    t = text(6000)
    cases = [dict(flg=framed_gen.FNAME, name=65), dict(flg=framed_gen.FEXTRA, xlen=300),
             dict(flg=framed_gen.FEXTRA | framed_gen.FNAME | framed_gen.FCOMMENT | framed_gen.FHCRC, xlen=1, name=300, comment=63)]
    for kw in cases:
        hdr = framed_gen.gzip_header(**kw)
        stream, off, plain = m.compose([t[:2000], t[2000:2001], t[2001:]], GZIP, header=hdr)
        assert zlib.decompress(stream, 31) == plain
        x, in_off, _, _, _ = both(torch, dev, stream, GZIP, plain)
        assert x["status"] == 0 and x["hdr_bytes"] == len(hdr) and in_off == off
        # a second member behind the trailer: end_offset names it, and the walk goes on from there
        second, off2, plain2 = m.compose([t[:500], t[500:]], GZIP)
        y = index_check(torch, dev, stream + second, GZIP)[0]
        assert y["status"] == 0 and y["end_offset"] == len(stream) and y["nchunks"] == 3
        out, xs = dev.inflate_stream_auto(to_dev(torch, stream + second), GZIP)
        assert bytes(out.cpu().numpy()) == plain and xs.end_offset == len(stream)
    # a header the rules refuse, and one whose name never ends
    assert index_check(torch, dev, b"\x1f\x8b\x08\x20" + stream[4:], GZIP)[0]["status"] == 1
    assert index_check(torch, dev, framed_gen.gzip_header(flg=framed_gen.FNAME, name=40, nul=False), GZIP)[0]["status"] == 1


# ---- host form -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
def test_host_form(pkg, frame):
    data = text(3 * 4096 + 1)
    r, stream = pkg.hip_deflate_stream(data, 6, frame, 4096)
    assert r == 0
    r, out, need, used = pkg.hip_inflate_stream(stream, len(data), frame)
    assert (r, out, need, used) == (0, data, len(data), len(stream))
    r, out, need, used = pkg.hip_inflate_stream(stream, len(data) - 1, frame)
    assert (r, out, need, used) == (3, b"", len(data), len(stream))
    r, out, need, used = pkg.hip_inflate_stream(stream + b"behind", len(data) + 5, frame)
    assert (r, out, used) == (0, data, len(stream))
    assert pkg.hip_inflate_stream(stream[:-m.TRAILER[frame] - 1], len(data), frame)[0] == 1
    if frame != RAW:
        bad = bytearray(stream)
        bad[-1] ^= 1
        assert pkg.hip_inflate_stream(bytes(bad), len(data), frame)[0] == 1
