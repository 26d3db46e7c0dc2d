"""What the tests of the block index and the block decode share (test_stream_blocks_model.py, test_gpu_stream_blocks.py): the
test streams, made once per process and never modified, and one call of either entry point held to the plain-Python model of
tests/stream_blocks_model.py -- every field of the summary, the rows of the tables with a sentinel row either side of each,
the bytes with 64 sentinel bytes either side.  No product code but the synthetic data's generator."""
import zlib

import numpy as np

import deflate_gen as dg
import hdtest
import stream_blocks_model as bm
import stream_carry_model as cm
import stream_index_model as m
from carry_dev import FRAMES, GUARD, GZIP, RAW, SENT, S_FIELDS, ZLIB, fields, to_dev, u32, u64

X_FIELDS = ("nrows", "npieces", "out_bytes", "end_offset", "end_bit", "ncandidates", "hdr_bytes", "status")
NBYTES = 600000
# name -> (data, level, memLevel): zlib.compressobj with no flush.  memLevel 8 gives 4 .. 9 blocks, memLevel 1 several hundred
SETS = {"text-1": ("text", 1, 8), "text-6": ("text", 6, 8), "fastq-6": ("fastq", 6, 8), "fastq-9": ("fastq", 9, 8),
        "text-6-m1": ("text", 6, 1), "fastq-1-m1": ("fastq", 1, 1)}
GPU_SETS = ("text-6", "fastq-9", "text-6-m1", "fastq-1-m1")
_cache = {}


def data(kind, n=NBYTES):
    if kind not in _cache:
        s = hdtest.synth()
        _cache[kind] = bytes((s.text_like if kind == "text" else s.fastq_like)(NBYTES, seed=7))[:NBYTES]
    return _cache[kind][:n]


def stream(name, frame=GZIP):
    """-> (stream, plain)"""
    key = (name, frame)
    if key not in _cache:
        kind, level, mem = SETS[name]
        _cache[key] = bm.plain_writer(data(kind), frame, level, mem)
    return _cache[key], data(SETS[name][0])


def small(frame=GZIP, n=30000):
    """a stream of a few dozen blocks that the model walks in milliseconds: the cuts, the flipped bits, the tampered tables"""
    key = ("small", frame, n)
    if key not in _cache:
        _cache[key] = bm.plain_writer(data("text", n), frame, 6, 1)
    return _cache[key], data("text", n)


def model(stream_, frame, max_rows=None, max_chunk_in=0, row_bytes=0):
    """index_blocks, once per argument set"""
    key = ("model", stream_, frame, max_rows, max_chunk_in, row_bytes)
    if key not in _cache:
        _cache[key] = bm.index_blocks(stream_, frame, max_rows, max_chunk_in, row_bytes)
    return _cache[key]


def corpus_stream(frame, limit=400000):
    """the valid cases of the hand-built corpus (tests/deflate_gen.py) as ONE stream: their blocks one behind another, the
    last one final -> (stream, plain, zlib takes it).  A case's distances stay inside the case's own bytes."""
    key = ("corpus", frame)
    if key not in _cache:
        blocks, total, zlib_ok = [], 0, True
        for c in dg.cached_corpus():
            if c.code != dg.OK or c.chunk or not c.blocks or not c.expected or total + len(c.expected) > limit:
                continue
            if any(b.kind == "btype3" for b in c.blocks):
                continue
            for b in c.blocks:
                nb = dg.Block(b.kind, b.tokens, b.data, False, lit_lens=b.lit_lens, dist_lens=b.dist_lens, hlit=b.hlit, hdist=b.hdist,
                              rle=b.rle, hclen=b.hclen, items=b.items, pre_lens=b.pre_lens, nlen=b.nlen, length=b.length)
                blocks.append(nb)
            total += len(c.expected)
            zlib_ok = zlib_ok and c.zlib
        blocks[-1].final = True
        plain = dg.expand(blocks)
        _cache[key] = (m.HEADER[frame] + dg.encode(blocks) + m.trailer(frame, plain), plain, zlib_ok)
    return _cache[key]


def index_check(torch, dev, stream_, frame, max_rows=None, max_chunk_in=0, row_bytes=0):
    """one hipdeflate_stream_index_blocks_dev held to its model: the summary, the rows of the tables, a sentinel row either
    side of each -> the model's answer"""
    want = model(stream_, frame, max_rows, max_chunk_in, row_bytes)
    rows = len(want[1])
    cap = want[0]["npieces"] + 2 if max_rows is None else max_rows          # (a chain has at most a row per piece)
    kinds = ((torch.int64, None), (torch.int32, 0xffffffff), (torch.int32, 0xffffffff), (torch.int64, None), (torch.int32, 0xffffffff))
    tabs = [torch.full((cap + 2,), -2, dtype=t, device="cuda") for t, _ in kinds]
    s = dev.index_stream_blocks_call(to_dev(torch, stream_), frame, cap, max_chunk_in, row_bytes, *(t[1:] for t in tabs))
    assert fields(s, X_FIELDS) == want[0]
    for t, w, (_, mask) in zip(tabs, want[1:], kinds):
        got = t.cpu().tolist()
        assert got[0] == -2 and got[cap + 1] == -2
        if want[0]["status"] != 1:
            assert got[rows + 1:] == [-2] * (cap + 1 - rows)
        assert [v & mask if mask else v for v in got[1:rows + 1]] == w
    return want


def decode_check(torch, dev, stream_, frame, in_off, in_len, out_size, out_off, reach, cap=None, plain=None):
    """one hipdeflate_stream_inflate_blocks_dev held to the model's verdict, 64 sentinel bytes either side of the output"""
    want, out = bm.decode_blocks(stream_, frame, in_off, in_len, out_size, out_off, reach, cap, plain=plain)
    room = (out_off[-1] + out_size[-1] if in_off else 0) if cap is None else cap
    room = min(room, 1 << 24)
    buf = torch.full((GUARD + room + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_blocks_call(to_dev(torch, stream_), frame, u64(torch, in_off), u32(torch, in_len), u32(torch, out_size),
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
    return want, b[GUARD:GUARD + room]


def both(torch, dev, stream_, frame, plain, max_chunk_in=0, row_bytes=0, zlib_ok=True, tail=0):
    """the index, then the decode on its table: the stream is one the method takes whole.  tail: bytes behind the trailer"""
    if zlib_ok:
        assert zlib.decompressobj(m.WBITS[frame]).decompress(stream_) == plain
    x, *t = index_check(torch, dev, stream_, frame, None, max_chunk_in, row_bytes)
    assert x["status"] == 0 and x["out_bytes"] == len(plain) and x["end_offset"] == len(stream_) - tail
    d, out = decode_check(torch, dev, stream_, frame, *t, plain=None if zlib_ok else plain)
    assert d["status"] == 0 and out == plain
    return x, t
