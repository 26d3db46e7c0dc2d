"""The plain-Python model of the block index and the block decode (tests/stream_blocks_model.py) held to zlib, without a GPU:
the header filter, the piece with its stop rule, the chain, the merge, the reach rule, and the decode's verdicts.  For every
row of every test stream the bits from in_off[i], shifted to a byte boundary, are inflated by zlib with the 32 KiB in front of
the row as its dictionary, and the first out_size[i] bytes must be the data's; the rows tile the payload bit for bit."""
import zlib

import numpy as np
import pytest

import blocks_dev as bd
import deflate_gen as dg
import deflate_tokens as dt
import stream_blocks_model as bm
import stream_carry_model as cm
import stream_index_model as m
from blocks_dev import FRAMES, GZIP, RAW, ZLIB


def held_to_zlib(stream, frame, plain, x, t, zlib_ok=True):
    """the table of a status-0 index: rows that tile the payload bit for bit, each one's bytes by zlib from its own bit"""
    in_off, in_len, out_size, out_off, reach = t
    end = len(stream) - m.TRAILER[frame]
    assert x["status"] == 0 and x["nrows"] == len(in_off) and x["out_bytes"] == len(plain)
    assert in_off[0] == 8 * x["hdr_bytes"] and in_off[-1] + in_len[-1] == x["end_bit"] and (x["end_bit"] + 7) >> 3 == end
    assert x["end_offset"] == len(stream)
    for i in range(len(in_off)):
        assert out_off[i] == sum(out_size[:i]) and reach[i] <= min(out_off[i], bm.WINDOW)
        if i:
            assert in_off[i] == in_off[i - 1] + in_len[i - 1]
        if zlib_ok and out_size[i]:
            d = zlib.decompressobj(-15, zdict=plain[max(0, out_off[i] - 32768):out_off[i]])
            assert d.decompress(bm.shifted(stream, in_off[i], end), out_size[i]) == plain[out_off[i]:out_off[i] + out_size[i]], i
    s, out = bm.decode_blocks(stream, frame, *t, plain=None if zlib_ok else plain)
    assert s["status"] == 0 and out == plain and s["in_bytes"] == len(stream)


# ---- the filter -------------------------------------------------------------------------------------------------------------

def test_pass_rate_on_random_bits_is_the_stated_one():
    r = float(bm.pass_rate())
    assert abs(r - bm.PASS_RATE) < 0.005e-4, r                 # 5.13e-4: one candidate per 244 bytes
    assert round(1 / (8 * r)) == 244


def test_candidate_list_against_a_brute_force_scan():
    rng = np.random.default_rng(3)
    blob = bytes(rng.integers(0, 256, 6000, dtype=np.uint8))
    for hdr, end in ((0, 6000), (10, 5992), (2, 37), (0, 3)):
        assert bm.candidates(blob, hdr, end) == bm.brute_candidates(blob, hdr, end), (hdr, end)
    n = len(bm.candidates(blob, 0, 6000)) - 1
    assert 6 <= n <= 50, n                                     # 24.6 expected
    s, _ = bd.small()
    assert bm.candidates(s, 10, len(s) - 8) == bm.brute_candidates(s, 10, len(s) - 8)


def test_filter_accepts_every_dynamic_header_of_the_corpus_the_oracle_accepts():
    seen = 0
    for c in dg.cached_corpus():
        if c.code != dg.OK or not c.blocks:
            continue
        for b in dt.read(c.stream, expand=False, wide=True).blocks:
            if b.kind != "dynamic":
                continue
            # the rule reads BFINAL 0: a final block's header is judged with that bit cleared
            s = bytearray(c.stream)
            s[b.start_bit >> 3] &= ~(1 << (b.start_bit & 7)) & 0xff
            assert bm.header_rule(bytes(s), b.start_bit, len(s)) == bm.YES, (c.name, b.start_bit)
            seen += 1
    assert seen > 500


# ---- the streams ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(bd.SETS))
def test_flushless_streams_of_zlib(name):
    stream, plain = bd.stream(name, GZIP)
    assert zlib.decompress(stream, 31) == plain
    for row_bytes in (0, 65536):
        x, *t = bd.model(stream, GZIP, row_bytes=row_bytes)
        held_to_zlib(stream, GZIP, plain, x, t)
        if row_bytes and name in bd.GPU_SETS:              # what the GPU tests stand on: the bit path and the marker path
            assert x["nrows"] >= 4 and any(o & 7 for o in t[0]) and any(t[4])
    x1, *t1 = bd.model(stream, GZIP, row_bytes=1)              # a row per piece
    assert x1["nrows"] == x1["npieces"] >= 4 and all(r > 0 for r in t1[4][1:])
    assert (x1["npieces"] > 500) == name.endswith("m1")
    held_to_zlib(stream, GZIP, plain, x1, t1)


@pytest.mark.parametrize("frame", (RAW, ZLIB))
@pytest.mark.parametrize("name", sorted(bd.SETS))
def test_flushless_streams_in_the_other_frames(name, frame):
    stream, plain = bd.stream(name, frame)
    assert zlib.decompress(stream, m.WBITS[frame]) == plain
    x, *t = bd.model(stream, frame)
    held_to_zlib(stream, frame, plain, x, t)
    assert t[0][0] == 8 * len(m.HEADER[frame])


@pytest.mark.parametrize("strategy, level, rows", ((zlib.Z_FIXED, 6, 1), (zlib.Z_DEFAULT_STRATEGY, 0, 1), (zlib.Z_RLE, 6, None),
                                                   (zlib.Z_HUFFMAN_ONLY, 6, None)))
@pytest.mark.parametrize("frame", FRAMES)
def test_strategies(strategy, level, rows, frame):
    plain = bd.data("text", 200000)
    stream = bm.plain_writer(plain, frame, level, 8, strategy)
    x, *t = bm.index_blocks(stream, frame, row_bytes=65536)
    held_to_zlib(stream, frame, plain, x, t)
    if rows:
        assert x["nrows"] == x["npieces"] == rows          # static or stored blocks only: one piece, one row
    else:
        assert x["nrows"] >= 3


@pytest.mark.parametrize("writer", (cm.pigz_writer, cm.sync_writer, lambda p, f: m.writer(p, f)[0]))
@pytest.mark.parametrize("frame", FRAMES)
def test_streams_with_flush_points_are_taken_too(writer, frame):
    plain = bd.data("text", 150000)
    stream = writer(cm.cut(plain, [20000, 333, 50000]), frame)
    x, *t = bm.index_blocks(stream, frame, row_bytes=16384)
    held_to_zlib(stream, frame, plain, x, t)
    assert x["nrows"] >= 3                                    # (five pieces of the writer; the short ones share a row)


@pytest.mark.parametrize("frame", FRAMES)
def test_the_hand_built_corpus_as_one_stream(frame):
    stream, plain, zlib_ok = bd.corpus_stream(frame)
    x, *t = bd.model(stream, frame, row_bytes=4096)
    assert x["npieces"] > 100 and x["nrows"] > 20
    held_to_zlib(stream, frame, plain, x, t, zlib_ok)


@pytest.mark.parametrize("frame", FRAMES)
def test_decoys_in_a_stored_payload_are_candidates_off_the_chain(frame):
    stream, plain, at = bm.decoy_stream(frame, np.random.default_rng(8))
    assert zlib.decompress(stream, m.WBITS[frame]) == plain
    hdr, refused, cand, pieces, end_bit, status = bm.chain(stream, frame)
    assert status == 0 and len(at) == 8 and sorted(set(a & 7 for a in at)) == list(range(8))
    on_chain = set(p[0] for p in pieces)
    for a in at:
        assert a in cand and a not in on_chain, a              # on the list, and nothing links to it
    x, *t = bm.index_blocks(stream, frame, row_bytes=1)
    held_to_zlib(stream, frame, plain, x, t)


# ---- the verdicts -----------------------------------------------------------------------------------------------------------

def test_table_too_small_and_the_sizing_call():
    stream, plain = bd.small()
    full = bm.index_blocks(stream, GZIP, row_bytes=4096)
    n = full[0]["nrows"]
    assert n >= 5
    x, *t = bm.index_blocks(stream, GZIP, max_rows=0, row_bytes=4096)
    assert x["status"] == 3 and x["nrows"] == n and x["out_bytes"] == 0 and t[0] == []
    x, *t = bm.index_blocks(stream, GZIP, max_rows=3, row_bytes=4096)
    assert x["status"] == 3 and x["nrows"] == n and t[0] == full[1][:3] and x["out_bytes"] == full[4][3]


def test_a_merged_row_longer_than_max_chunk_in_ends_the_chain():
    stream, plain = bd.small()
    full = bm.index_blocks(stream, GZIP, row_bytes=1)
    longest = max(full[2])
    x, *t = bm.index_blocks(stream, GZIP, max_chunk_in=(longest + 7) // 8 + 2, row_bytes=1)
    assert x["status"] == 0
    x, *t = bm.index_blocks(stream, GZIP, max_chunk_in=(longest + 7) // 8 + 2, row_bytes=8192)
    assert x["status"] == 1 and x["nrows"] < full[0]["nrows"] and x["end_bit"] in full[1] and len(t[0]) == x["nrows"]


def test_cuts_are_status_2_and_flips_status_1_or_2():
    stream, plain = bd.small()
    for cut in list(range(len(stream) - 64, len(stream))) + [len(stream) // 2, len(stream) // 3]:
        x = bm.index_blocks(stream[:cut], GZIP, row_bytes=4096)[0]
        assert x["status"] in (1, 2) and x["status"] == (2 if cut < len(stream) - 8 else x["status"]), cut
    x, *t = bm.index_blocks(stream, GZIP, row_bytes=1)
    third = t[0][3]
    for bit in (third + 1, third + 40, third + 2000, 8 * len(stream) - 20):
        s = bytearray(stream)
        s[bit >> 3] ^= 1 << (bit & 7)
        y, *u = bm.index_blocks(bytes(s), GZIP, row_bytes=1)
        # the rows in front stay usable -- but for the one that ended in front of a header that no longer reads as one
        assert u[0][:2] == t[0][:2]
        if bit >= 8 * (len(stream) - 8):
            assert y["status"] == 0
        if y["status"] == 0:                                   # a token that still decodes, the trailer: the check finds it
            assert bm.decode_blocks(bytes(s), GZIP, *u)[0]["status"] == 2
        else:
            assert y["status"] in (1, 2)


def test_a_first_token_that_reaches_back_is_status_1_with_no_rows():
    blocks = [dg.Block("dynamic", [(10, 4), 65, 66]), dg.Block("dynamic", [67] * 20, final=True)]
    stream = dg.encode(blocks)
    x, *t = bm.index_blocks(stream, RAW, row_bytes=1)
    assert x["status"] == 1 and x["nrows"] == 0 and x["npieces"] == 1 and x["end_bit"] == 0 and t[0] == []


def test_tampered_tables_are_status_1_or_2():
    stream, plain = bd.small()
    x, *t = bm.index_blocks(stream, GZIP, row_bytes=4096)
    n = x["nrows"]
    for col, row, delta, want in ((0, 2, 1, 1), (0, 2, -1, 1), (0, n - 1, 1, None), (1, 2, 1, 1), (1, 2, -1, 2), (1, n - 1, -1, 2),
                                  (2, 2, -1, 1), (2, n - 1, -1, 2), (4, 2, None, 2)):
        u = [list(c) for c in t]
        u[col][row] = u[col][row] + delta if delta is not None else u[col][row] - 1
        s, _ = bm.decode_blocks(stream, GZIP, *u)
        assert s["status"] == want or (want is None and s["status"] in (1, 2)), (col, row, delta, s)
    u = [list(c) for c in t]
    u[0][3] = u[0][2]                                          # rows overlapping
    assert bm.decode_blocks(stream, GZIP, *u)[0]["status"] == 1
