"""The device-resident calls share their scratch: d_stream serves the stream encode's window, the three stream decoders and the
fold; d_stream_slots the encode's slots and the carry decode's marker path; d_index and d_cand the member index, both stream
indexes and the verify -- each call with a layout of its own (7bgzf_amd/csrc/hd_scratch.hpp) over the same buffer, which is
freed and allocated anew whenever a call needs more.  So, in ONE process and context, a fixed interleaving of

    the member index and its decode, a ranged read, stream_deflate, inflate_stream, the full-flush index and its table decode,
    the carry index and the carry decode with a marker-path group between two fast-path groups, check_combine, and the two
    host-buffer forms

at 65, 1, 2049 and 3 rows in that order -- buffers reused by a smaller call, and behind a growth -- once on the default stream
and once on a side stream.  Every result is what zlib on the CPU gives for the input: the bytes, the summary fields, the check.
No case provokes a fault: every input is well formed and every call stays inside its buffers."""
import importlib
import os
import zlib

import numpy as np
import pytest

import hdtest
import member_index_model as mm
import stream_carry_model as cm
import stream_model as sm
from carry_dev import S_FIELDS, X_FIELDS, fields, to_dev, u32

pytestmark = pytest.mark.gpu

P = 96                                          # bytes a row: a chunk of the stream encode (a multiple of 16), a member, a piece
INDEXED = tuple(f for f in X_FIELDS if f != "ncandidates")    # (a marker in the coded bytes is a candidate too)
ROWS = (65, 1, 2049, 3)                         # a wavefront and a scan tile passed, and the smallest; small behind large
FRAME = {65: sm.FRAME_GZIP, 1: sm.FRAME_ZLIB, 2049: sm.FRAME_ZLIB, 3: sm.FRAME_GZIP}


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


def raw_deflate(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def flushed(pieces, frame, sync):
    """one compressor, a flush behind every piece but the last: Z_SYNC_FLUSH behind piece i where sync(i), else Z_FULL_FLUSH"""
    c = zlib.compressobj(6, zlib.DEFLATED, sm.WBITS[frame])
    out = b""
    for i, p in enumerate(pieces):
        out += c.compress(p)
        out += c.flush() if i == len(pieces) - 1 else c.flush(zlib.Z_SYNC_FLUSH if sync(i) else zlib.Z_FULL_FLUSH)
    return out


@pytest.fixture(scope="module")
def inputs():
    """per row count, made once and never modified: the data -- every piece starts with the second half of the one in front of
    it, so a row behind a sync flush reaches back -- and its three containers"""
    base = cm.words(np.random.default_rng(21), P // 2 * (max(ROWS) + 1))
    out = {}
    for n in ROWS:
        pieces = [base[j * (P // 2):j * (P // 2) + P] for j in range(n)]
        data, frame = b"".join(pieces), FRAME[n]
        assert sm.cut(data, P) == pieces
        k = -(-n // 3)                          # rows a group of the carry decode: [0, k) and [2k, n) by full flushes, [k, 2k) carry
        out[n] = dict(data=data, pieces=pieces, frame=frame, group=k * P,
                      members=b"".join(mm.gz_member("BC", raw_deflate(p), zlib.crc32(p), len(p)) for p in pieces),
                      full=flushed(pieces, frame, lambda i: False),
                      mixed=flushed(pieces, frame, lambda i: k - 1 <= i <= 2 * k - 2),
                      check=zlib.adler32(data) if frame == sm.FRAME_ZLIB else zlib.crc32(data))
        for s in (out[n]["full"], out[n]["mixed"]):
            assert zlib.decompress(s, sm.WBITS[frame]) == data
    return out


def host(t):
    return bytes(t.cpu().numpy())


def one_round(pkg, torch, dev, n, data, pieces, frame, group, members, full, mixed, check):
    size = len(data)
    decoded = dict(out_bytes=size, bad_chunk=n, nchunks=n, check=check, status=0)
    indexed = dict(nchunks=n, out_bytes=size, hdr_bytes=len(sm.HEADER[frame]), status=0)
    # the member index and its decode
    blob = to_dev(torch, members)
    d = dev.DeviceInflate(n)
    s = d.index(blob)
    assert (s.nmembers, s.out_bytes, s.end_offset, s.status) == (n, size, len(members), 0)
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d.run(blob, out, s)
    assert host(out) == data
    # a ranged read: the first bytes, a run over several members, the last byte
    begins, ends = [0, size // 3, size - 1], [min(size, 10), min(size, size // 3 + 3 * P + 5), size]
    got, dst_off, q_len, q_status, r = d.read_ranges(blob, begins, ends)
    touched = {m for b, e in zip(begins, ends) for m in range(b // P, (e - 1) // P + 1)}
    assert (r.status, r.nrefused, r.bad_member, r.out_bytes, r.nselected, r.sel_bytes) == (0, 0, n, sum(e - b for b, e in zip(begins, ends)),
                                                                                          len(touched), sum(len(pieces[m]) for m in touched))
    assert q_status.cpu().tolist() == [0, 0, 0] and q_len.cpu().tolist() == [e - b for b, e in zip(begins, ends)]
    got, at = host(got), dst_off.cpu().tolist()
    assert [got[o:o + e - b] for o, b, e in zip(at, begins, ends)] == [data[b:e] for b, e in zip(begins, ends)]
    # stream_deflate, and inflate_stream on its table
    strm, chunk_off, s = dev.deflate_stream(to_dev(torch, data), 6, frame, P)
    assert fields(s, S_FIELDS) == dict(decoded, out_bytes=strm.numel(), in_bytes=size)
    assert zlib.decompress(host(strm), sm.WBITS[frame]) == data
    strm = to_dev(torch, host(strm))
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_call(strm, frame, chunk_off, n, P, size, out, size)
    assert fields(s, S_FIELDS) == dict(decoded, in_bytes=strm.numel()) and host(out) == data
    # the full-flush index and the decode by its table
    strm = to_dev(torch, full)
    in_off, in_len, out_size, out_off, x = dev.index_stream(strm, frame, max_chunks=n)
    assert fields(x, INDEXED) == dict(indexed, end_offset=len(full)) and x.ncandidates >= n
    assert out_size.cpu().tolist() == [P] * n and out_off.cpu().tolist() == list(range(0, size, P))
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_table_call(strm, frame, in_off, in_len, out_size, out_off, n, out, size)
    assert fields(s, S_FIELDS) == dict(decoded, in_bytes=len(full)) and host(out) == data
    # the carry index and the carry decode: the rows of the middle group reach back, the groups either side take the fast path
    strm = to_dev(torch, mixed)
    in_off, in_len, out_size, out_off, reach, x = dev.index_stream_carry(strm, frame, max_chunks=n)
    assert fields(x, INDEXED) == dict(indexed, end_offset=len(mixed)) and x.ncandidates >= n
    assert out_size.cpu().tolist() == [P] * n
    k, back = group // P, reach.cpu().tolist()
    assert back[:k] == [0] * k and back[2 * k:] == [0] * (n - min(n, 2 * k)) and (n < 3 or min(back[k:2 * k]) > 0)
    pkg.lib().hipdeflate_test_carry_group(group)
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_carry_call(strm, frame, in_off, in_len, out_size, out_off, reach, n, out, size)
    pkg.lib().hipdeflate_test_carry_group(0)
    assert fields(s, S_FIELDS) == dict(decoded, in_bytes=len(mixed)) and host(out) == data
    # check_combine
    kind = sm.KIND[frame]
    parts = [zlib.adler32(p) if kind == sm.ADLER32 else zlib.crc32(p) for p in pieces]
    assert dev.check_combine(u32(torch, parts), u32(torch, [P] * n), kind) == check
    # the host-buffer forms, whose row table the index leaves in a buffer of the library
    assert pkg.hip_inflate_stream(full, size, frame) == (0, data, size, len(full))
    assert pkg.hip_inflate_stream_carry(mixed, size, frame) == (0, data, size, len(mixed))


@pytest.mark.parametrize("side", (False, True), ids=("default_stream", "side_stream"))
def test_interleaved_calls_share_their_scratch(pkg, torch, dev, inputs, side):
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(torch.cuda.Stream() if side else torch.cuda.current_stream()):
            for n in ROWS:
                one_round(pkg, torch, dev, n, **inputs[n])
            torch.cuda.synchronize()
    finally:
        pkg.lib().hipdeflate_test_carry_group(0)
    assert pkg.lib().hipdeflate_stall_count() == 0
