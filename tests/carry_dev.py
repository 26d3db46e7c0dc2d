"""What the GPU tests of the carry index and the carry decode share (test_gpu_stream_carry.py, test_gpu_carry_rows.py): one
call of either entry point held to the plain-Python model of tests/stream_carry_model.py -- every field of the summary, the
rows of the tables with a sentinel row either side of each, the bytes with 64 sentinel bytes either side.  No product code."""
import zlib

import numpy as np

import stream_carry_model as cm
import stream_index_model as m

GUARD = 64
SENT = 0xa5
RAW, ZLIB, GZIP = m.FRAME_RAW, m.FRAME_ZLIB, m.FRAME_GZIP
FRAMES = (RAW, ZLIB, GZIP)
X_FIELDS = ("nchunks", "out_bytes", "end_offset", "ncandidates", "hdr_bytes", "status")
S_FIELDS = ("out_bytes", "in_bytes", "bad_chunk", "nchunks", "check", "status")


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def u32(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32).copy()).cuda()


def u64(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


def fields(s, names):
    return {f: getattr(s, f) for f in names}


def index_check(torch, dev, stream, frame, max_chunks=None, max_chunk_in=0, carry=True):
    """one hipdeflate_stream_index_carry_dev (carry False: one hipdeflate_stream_index_dev, without the reach column) held
    to its model: the summary, the rows of the tables, and a sentinel row either side of each -> the model's answer.  (Rows
    behind the one that ended the chain are not looked at.)"""
    model, call = (cm.index_carry, dev.index_stream_carry_call) if carry else (m.index, dev.index_stream_call)
    want = model(stream, frame, max_chunks, max_chunk_in)
    rows = len(want[1])
    cap = max(rows, want[0]["ncandidates"]) if max_chunks is None else max_chunks          # (a chain has at most a row per candidate)
    kinds = ((torch.int64, None), (torch.int32, 0xffffffff), (torch.int32, 0xffffffff), (torch.int64, None), (torch.int32, 0xffffffff))
    kinds = kinds[:len(want) - 1]
    tabs = [torch.full((cap + 2,), -2, dtype=t, device="cuda") for t, _ in kinds]
    s = call(to_dev(torch, stream), frame, cap, max_chunk_in, *(t[1:] for t in tabs))
    assert fields(s, X_FIELDS) == want[0]
    for t, w, (_, mask) in zip(tabs, want[1:], kinds):
        got = t.cpu().tolist()
        assert got[0] == -2 and got[cap + 1] == -2
        if want[0]["status"] != 1:
            assert got[rows + 1:] == [-2] * (cap + 1 - rows)
        assert [v & mask if mask else v for v in got[1:rows + 1]] == w
    return want


def decode_check(torch, dev, stream, frame, in_off, in_len, out_size, out_off, reach, cap=None, plain=None):
    """one hipdeflate_stream_inflate_carry_dev held to the model's verdict, 64 sentinel bytes either side of the output.
    plain: the bytes of the rows where zlib does not decode them (the token lists' own: deflate_gen.expand)"""
    want, out = cm.decode_carry(stream, frame, in_off, in_len, out_size, out_off, reach, cap, plain=plain)
    room = (out_off[-1] + out_size[-1] if in_off else 0) if cap is None else cap
    room = min(room, 1 << 24)
    buf = torch.full((GUARD + room + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_carry_call(to_dev(torch, stream), frame, u64(torch, in_off), u32(torch, in_len), u32(torch, out_size),
                                      u64(torch, out_off), u32(torch, reach), len(in_off), buf[GUARD:], room if cap is None else cap)
    got = fields(s, S_FIELDS)
    if want["check"] is None:
        got["check"] = None
    assert got == want
    b = bytes(buf.cpu().numpy())
    assert b[:GUARD] == bytes([SENT]) * GUARD and b[GUARD + room:] == bytes([SENT]) * GUARD
    if want["status"] in (1, 3):                                               # nothing is decoded
        assert b[GUARD:GUARD + room] == bytes([SENT]) * room
    if want["status"] == 0:
        assert b[GUARD:GUARD + room] == out
    return want


def both(torch, dev, stream, frame, plain, max_chunk_in=0, zlib_ok=True):
    """the index, then the decode on its table: the stream is one the method takes whole.  zlib_ok False: a stream of the
    forms zlib refuses, whose bytes are `plain` by the token lists alone"""
    if zlib_ok:
        assert zlib.decompress(stream, m.WBITS[frame]) == plain
    x, *t = index_check(torch, dev, stream, frame, None, max_chunk_in)
    assert x["status"] == 0 and x["out_bytes"] == len(plain) and x["end_offset"] == len(stream)
    d = decode_check(torch, dev, stream, frame, *t, plain=None if zlib_ok else plain)
    assert d["status"] == 0
    return x, t
