"""The block index and the block decode -- hipdeflate_stream_index_blocks_dev, hipdeflate_stream_inflate_blocks_dev,
hip_inflate_stream_blocks, hipdeflate_test_block_headers_dev and their device.py forms -- against the plain-Python model of
tests/stream_blocks_model.py.  Bit-exact: the five tables, every field of both summaries, the bytes, 64 sentinel bytes around
every output and one sentinel row around every table; hipdeflate_stall_count() stays 0.  No case provokes a fault: every
refusal is a verdict the contract of include/hipdeflate.h defines, each runs once, and none reads or writes outside its
buffers.  Every case decodes 600,000 bytes at the most.

Where the cases land (hd_blocks.hpp):
  * streams of zlib without a flush, 600,000 bytes of text and of FASTQ-like data: memLevel 8 (4 .. 9 blocks, most of them
    not byte-aligned, every one but the first reaching back) and memLevel 1 (several hundred blocks: rows of many pieces, the
    segmented maximum), in all three frames, a gzip header with every optional field, bytes behind the trailer;
  * row_bytes 1 (a row per piece), 4096, 65536 and the default; groups of 4096, 65536 and the default;
  * Z_FIXED and level 0 (one piece), Z_RLE, Z_HUFFMAN_ONLY, streams with sync and full flush points, the hand-built corpus as
    one stream, header-shaped decoys at all eight bit shifts in a stored payload;
  * the refusals the header names, cuts at every byte of the last 64, flipped bits, tampered tables."""
import ctypes
import importlib
import os
import zlib

import numpy as np
import pytest

import blocks_dev as bd
import deflate_gen as dg
import framed_gen
import hdtest
import stream_blocks_model as bm
import stream_carry_model as cm
import stream_index_model as m
from blocks_dev import FRAMES, GZIP, RAW, ZLIB, both, decode_check, index_check
from carry_dev import GUARD, SENT, fields, to_dev, u64

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


# ---- the filter alone ---------------------------------------------------------------------------------------------------------

def test_header_rule_through_its_test_entry(pkg, torch):
    rng = np.random.default_rng(21)
    blob = bytes(rng.integers(0, 256, 5000, dtype=np.uint8))
    s, _ = bd.small()
    for data, end in ((blob, 5000), (blob, 4091), (s, len(s) - 8)):
        pos = list(range(8 * end + 9))
        got = torch.full((len(pos) + 2,), -2, dtype=torch.int32, device="cuda")
        d_data, d_pos = to_dev(torch, data), u64(torch, pos)
        torch.cuda.synchronize()
        rc = pkg.lib().hipdeflate_test_block_headers_dev(d_data.data_ptr(), end, d_pos.data_ptr(), len(pos), got[1:].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        got = got.cpu().tolist()
        assert got[0] == -2 and got[-1] == -2
        want = [bm.header_rule(data, p, end) for p in pos]
        assert got[1:-1] == want
        assert [p for p in pos[1:] if want[p] == bm.YES] == bm.candidates(data, 0, end)[1:]


def test_candidate_list_of_the_two_passes_position_by_position(pkg, torch):
    """k_blocks_flag / k_blocks_write themselves: the granule's dwords moved on a byte at a time, the byte-wise load of the
    last 28 bytes, the mask below the first bit, more than one tile (64 KiB) and more than one scan tile of them"""
    rng = np.random.default_rng(22)
    blob = bytes(rng.integers(0, 256, 200000, dtype=np.uint8))
    s, _ = bd.stream("text-6-m1", RAW)
    for data, end, first in ((blob, 200000, 0), (blob, 199987, 8 * 16 + 3), (blob, 65536 + 27, 8 * 1023 + 7), (blob, 19, 0), (blob, 1, 5),
                             (s, len(s), 0), (s, 70001, 80)):
        want = [first] + [p for p in bm.candidates(data, 0, end)[1:] if p > first]
        d_data = to_dev(torch, data)
        got = torch.full((len(want) + 2,), -2, dtype=torch.int64, device="cuda")
        count = ctypes.c_uint64(0)
        torch.cuda.synchronize()
        rc = pkg.lib().hipdeflate_test_block_candidates_dev(d_data.data_ptr(), end, first, got[1:].data_ptr(), len(want), ctypes.byref(count),
                                                            None)
        assert rc == 0 and count.value == len(want), (end, first, count.value, len(want))
        got = got.cpu().tolist()
        assert got[0] == -2 and got[-1] == -2 and got[1:-1] == want, (end, first)
    assert len(bm.candidates(blob, 0, 200000)) > 500


# ---- the streams --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", bd.GPU_SETS)
def test_flushless_streams(torch, dev, name, frame):
    stream, plain = bd.stream(name, frame)
    x, t = both(torch, dev, stream, frame, plain)
    assert x["npieces"] >= 4 and t[0][0] == 8 * len(m.HEADER[frame])


@pytest.mark.parametrize("row_bytes", (1, 4096, 65536))
@pytest.mark.parametrize("name", ("fastq-9", "text-6-m1"))
def test_row_sizes(torch, dev, name, row_bytes):
    stream, plain = bd.stream(name, GZIP)
    x, t = both(torch, dev, stream, GZIP, plain, row_bytes=row_bytes)
    if row_bytes == 1:
        assert x["nrows"] == x["npieces"]
    else:
        assert x["nrows"] >= 4 and any(o & 7 for o in t[0]) and any(t[4])


@pytest.mark.parametrize("group", (4096, 65536))
def test_groups(pkg, torch, dev, group):
    stream, plain = bd.stream("text-6-m1", GZIP)
    x, *t = bd.model(stream, GZIP, row_bytes=4096)
    pkg.lib().hipdeflate_test_carry_group(group)
    d, out = decode_check(torch, dev, stream, GZIP, *t)
    assert d["status"] == 0 and out == plain


def test_gzip_header_fields_and_bytes_behind_the_trailer(torch, dev):
    raw, plain = bd.stream("text-6-m1", RAW)
    hdr = framed_gen.gzip_header(flg=framed_gen.FEXTRA | framed_gen.FNAME | framed_gen.FCOMMENT | framed_gen.FHCRC, xlen=5, name=31,
                                 comment=63)
    stream = hdr + raw + m.trailer(GZIP, plain) + b"behind the trailer"
    x, t = both(torch, dev, stream, GZIP, plain, row_bytes=65536, tail=18)
    assert x["hdr_bytes"] == len(hdr) and t[0][0] == 8 * len(hdr)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("strategy, level", ((zlib.Z_FIXED, 6), (zlib.Z_DEFAULT_STRATEGY, 0), (zlib.Z_RLE, 6), (zlib.Z_HUFFMAN_ONLY, 6)))
def test_strategies(torch, dev, strategy, level, frame):
    plain = bd.data("text", 200000)
    x, t = both(torch, dev, bm.plain_writer(plain, frame, level, 8, strategy), frame, plain, row_bytes=65536)
    assert (x["npieces"] == 1) == (strategy == zlib.Z_FIXED or level == 0)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("writer", (cm.pigz_writer, cm.sync_writer, lambda p, f: m.writer(p, f)[0]))
def test_streams_with_flush_points(torch, dev, writer, frame):
    plain = bd.data("text", 150000)
    both(torch, dev, writer(cm.cut(plain, [20000, 333, 50000]), frame), frame, plain, row_bytes=16384)


@pytest.mark.parametrize("frame", FRAMES)
def test_the_hand_built_corpus_as_one_stream(torch, dev, frame):
    stream, plain, zlib_ok = bd.corpus_stream(frame)
    both(torch, dev, stream, frame, plain, row_bytes=4096, zlib_ok=zlib_ok)


@pytest.mark.parametrize("frame", FRAMES)
def test_decoys_at_every_bit_shift(torch, dev, frame):
    stream, plain, at = bm.decoy_stream(frame, np.random.default_rng(8))
    x, t = both(torch, dev, stream, frame, plain, row_bytes=1)
    assert x["ncandidates"] >= 9 and not set(at) & set(t[0])


# ---- the refusals -------------------------------------------------------------------------------------------------------------

def test_table_too_small_and_the_sizing_call(torch, dev):
    stream, plain = bd.small()
    n = index_check(torch, dev, stream, GZIP, row_bytes=4096)[0]["nrows"]
    assert index_check(torch, dev, stream, GZIP, max_rows=3, row_bytes=4096)[0]["status"] == 3
    s = dev.index_stream_blocks_call(to_dev(torch, stream), GZIP, 0, 0, 4096, None, None, None, None, None)
    assert fields(s, bd.X_FIELDS) == bm.index_blocks(stream, GZIP, 0, 0, 4096)[0] and s.status == 3 and s.nrows == n


def test_a_merged_row_longer_than_max_chunk_in(torch, dev):
    stream, plain = bd.small()
    longest = max(bm.index_blocks(stream, GZIP, row_bytes=1)[2])
    assert index_check(torch, dev, stream, GZIP, None, (longest + 7) // 8 + 2, 1)[0]["status"] == 0
    assert index_check(torch, dev, stream, GZIP, None, (longest + 7) // 8 + 2, 8192)[0]["status"] == 1
    big, _ = bd.stream("text-6-m1", GZIP)
    x = index_check(torch, dev, big, GZIP, None, 12000, 65536)[0]
    assert x["status"] == 1


def test_cuts(torch, dev):
    stream, plain = bd.small()
    x, *t = bm.index_blocks(stream, GZIP, row_bytes=1)
    cuts = list(range(len(stream) - 64, len(stream))) + [(t[0][k] + 7) // 8 + d for k in (2, 5) for d in (0, 1, 4, 9)]
    seen = set()
    for cut in cuts:
        seen.add(index_check(torch, dev, stream[:cut], GZIP, row_bytes=4096)[0]["status"])
    assert seen == {1, 2} or seen == {2}


def test_flipped_bits(torch, dev):
    stream, plain = bd.small()
    x, *t = bm.index_blocks(stream, GZIP, row_bytes=1)
    third = t[0][3]
    for bit in (third + 1, third + 40, third + 2000, 8 * len(stream) - 20):
        s = bytearray(stream)
        s[bit >> 3] ^= 1 << (bit & 7)
        y, *u = index_check(torch, dev, bytes(s), GZIP, row_bytes=1)
        if y["status"] == 0:
            assert decode_check(torch, dev, bytes(s), GZIP, *u)[0]["status"] == 2
        elif u[0]:
            assert decode_check(torch, dev, bytes(s), GZIP, *u)[0]["status"] in (0, 2)      # the rows in front stay usable


def test_a_first_token_that_reaches_back(torch, dev):
    stream = dg.encode([dg.Block("dynamic", [(10, 4), 65, 66]), dg.Block("dynamic", [67] * 20, final=True)])
    x = index_check(torch, dev, stream, RAW, row_bytes=1)[0]
    assert x["status"] == 1 and x["nrows"] == 0


def test_tampered_tables(torch, dev):
    stream, plain = bd.small()
    x, *t = bm.index_blocks(stream, GZIP, row_bytes=4096)
    n = x["nrows"]
    seen = set()
    for col, row, delta in ((0, 2, 1), (0, 2, -1), (0, n - 1, 1), (1, 2, 1), (1, 2, -1), (1, n - 1, -1), (1, n - 1, 1), (2, 2, -1),
                            (2, n - 1, -1), (4, 2, -1), (4, n - 1, -1)):
        u = [list(c) for c in t]
        if col == 4 and u[col][row] == 0:
            continue
        u[col][row] += delta
        seen.add(decode_check(torch, dev, stream, GZIP, *u)[0]["status"])
    u = [list(c) for c in t]
    u[0][3] = u[0][2]                                          # rows overlapping
    assert decode_check(torch, dev, stream, GZIP, *u)[0]["status"] == 1
    assert {1, 2} <= seen                                      # (0: a last row stated one bit longer still ends in its final block)
    assert decode_check(torch, dev, stream, GZIP, *t, cap=x["out_bytes"] - 1)[0]["status"] == 3


# ---- the layers above ---------------------------------------------------------------------------------------------------------

def test_host_buffer_form_and_device_calls(pkg, torch, dev):
    for name, frame in (("fastq-9", GZIP), ("text-6-m1", ZLIB)):
        stream, plain = bd.stream(name, frame)
        assert zlib.decompress(stream, m.WBITS[frame]) == plain
        r, out, need, used = pkg.hip_inflate_stream_blocks(stream + b"xyz", len(plain), frame)
        assert (r, out, need, used) == (0, plain, len(plain), len(stream))
        assert pkg.hip_inflate_stream_blocks(stream, len(plain) - 1, frame)[::2] == (3, len(plain))
        assert pkg.hip_inflate_stream_blocks(stream[:-9], len(plain), frame)[0] == 1
        out, x = dev.inflate_stream_blocks(to_dev(torch, stream), frame)
        assert bytes(out.cpu().numpy()) == plain and fields(x, bd.X_FIELDS) == bd.model(stream, frame)[0]
        t = dev.index_stream_blocks(to_dev(torch, stream), frame, row_bytes=65536)
        assert t[5].status == 0 and t[0].numel() >= t[5].nrows == bd.model(stream, frame, row_bytes=65536)[0]["nrows"]


def test_the_existing_indexes_still_answer_one_row(torch, dev):
    stream, plain = bd.stream("fastq-9", GZIP)
    s = to_dev(torch, stream)
    *_, x = dev.index_stream(s, GZIP)
    assert (x.status, x.nchunks, x.out_bytes) == (0, 1, len(plain))
    *_, x = dev.index_stream_carry(s, GZIP)
    assert (x.status, x.nchunks, x.out_bytes) == (0, 1, len(plain))
    out, x = dev.inflate_stream_carry(s, GZIP)
    assert bytes(out.cpu().numpy()) == plain
