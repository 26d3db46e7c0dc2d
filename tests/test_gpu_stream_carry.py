"""The carry index and the carry decode -- hipdeflate_stream_index_carry_dev, hipdeflate_stream_inflate_carry_dev,
hip_inflate_stream_carry and their device.py forms -- against the plain-Python model of tests/stream_carry_model.py.
Bit-exact: the five tables, every field of both summaries, the bytes, 64 sentinel bytes around every output and one sentinel
row around every table; hipdeflate_stall_count() stays 0.  No case provokes a fault: every refusal is a verdict the contract
of include/hipdeflate.h defines, each runs once, and none reads or writes outside its buffers.

Where the cases land (hd_carry.hpp):
  * both writers (one compressor with Z_SYNC_FLUSH; pigz's primed pieces), every frame, levels 1 and 6, pieces of 1, 100,
    4,096, 40,000, 10 and 70,000 bytes: rows shorter and longer than the 32 KiB tail, a short row between two long ones;
  * 5,000 rows of 16 bytes and 40,000 rows of one byte with a match 32768 back behind them: marker chains through many short
    rows of k_carry_tails, more rows than a scan tile;
  * rows of 32767 .. 65537 bytes with markers at their start and at their end: the edges of the tail and of both rings;
  * hand-built rows: a reach of 32768 and of out_off exactly, overlapping matches whose source starts in the window, copies of
    copies of markers, markers across block boundaries and behind stored blocks, a row of size 0;
  * the refusals the header names; groups of 4,096 and 65,536 bytes; a group that takes the fast path between two that do not."""
import importlib
import os
import zlib

import numpy as np
import pytest

import deflate_gen as dg
import hdtest
import stream_carry_model as cm
import stream_index_model as m
from carry_dev import FRAMES, GZIP, RAW, ZLIB, X_FIELDS, both, decode_check, fields, index_check, to_dev

pytestmark = pytest.mark.gpu

WRITERS = (cm.sync_writer, cm.pigz_writer)
W = cm.WINDOW


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


_text = {}


def text(n, seed=11):
    """n bytes of words, shared and never modified"""
    if seed not in _text:
        _text[seed] = cm.words(np.random.default_rng(seed), 320000)
    assert n <= len(_text[seed])
    return _text[seed][:n]


# ---- both writers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", (1, 6))
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("writer", WRITERS)
def test_writers(torch, dev, writer, frame, level):
    data = text(200000)
    pieces = cm.cut(data, [1, 100, 4096, 40000, 10, 70000])
    x, t = both(torch, dev, writer(pieces, frame, level), frame, data)
    assert t[2] == [len(p) for p in pieces] and max(t[4]) > 0


@pytest.mark.parametrize("writer", WRITERS)
def test_five_thousand_rows_of_16_bytes(torch, dev, writer):
    data = text(5000 * 16)
    x, t = both(torch, dev, writer(cm.cut(data, [16]), GZIP), GZIP, data, max_chunk_in=4096)
    assert x["nchunks"] == 5000 and sum(1 for r in t[4] if r) > 2500                 # (a row of literals alone reaches nowhere)


def test_forty_thousand_rows_of_one_byte_then_a_match_a_window_back(torch, dev):
    data = text(40000, seed=12)
    one = {c: dg.encode([dg.Block("static", [c])], chunk=True) for c in set(data)}          # a one-byte row per value, coded once
    plain = data + data[40000 - W:40000 - W + 258] + b"!" + data[40000 + 259 - W:40000 + 359 - W]
    body = b"".join(one[c] for c in data) + dg.encode([dg.Block("static", [(258, W), 33, (100, W)], final=True)])
    stream = m.HEADER[ZLIB] + body + m.trailer(ZLIB, plain)
    x, t = both(torch, dev, stream, ZLIB, plain, max_chunk_in=4096)
    assert x["nchunks"] == 40001 and t[4][-1] == W and t[4][:-1] == [0] * 40000


# ---- the edges of the tail and of the rings ----------------------------------------------------------------------------------

def filler(rng, n, final=False):
    """n bytes in stored blocks"""
    data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    return [dg.Block("stored", data=data[i:i + 65535]) for i in range(0, n, 65535)]


def edge_row(rng, size):
    """a row of `size` bytes behind at least a window of others: 258 markers at its start; 258 at its end -- named directly
    where the row is short enough for that, else copied from markers placed 32768 in front of them"""
    at = [0, size - 258] if size - 258 < W else [0, 32500, 32500 + W]
    blocks, pos = [], 0
    for p in at:
        blocks += filler(rng, p - pos) + [dg.Block("static" if p else "dynamic", [(258, W)])]
        pos = p + 258
    return blocks + filler(rng, size - pos)


def test_row_sizes_around_the_tail_and_ring_edges(torch, dev):
    rng = np.random.default_rng(5)
    sizes = (32767, 32768, 32769, 65535, 65536, 65537)
    rows = [filler(rng, 40000)] + [edge_row(rng, s) for s in sizes] + [[dg.Block("static", [(100, W), 7], final=True)]]
    stream, plain = cm.compose_rows(rows, GZIP)
    x, t = both(torch, dev, stream, GZIP, plain)
    assert t[2] == [40000] + list(sizes) + [101] and t[4] == [0] + [W] * 7


# ---- hand-built rows ---------------------------------------------------------------------------------------------------------

def hand_built():
    rng = np.random.default_rng(6)
    lead = filler(rng, 40000)
    lits = [int(v) for v in rng.integers(0, 256, 300)]
    last = [dg.Block("static", [(3, 1), 1], final=True)]
    cases = {
        "reach 32768": [filler(rng, W), [dg.Block("static", [(10, W), 5])], last],
        "reach out_off": [[dg.Block("static", lits[:40])], [dg.Block("dynamic", [(5, 40), 9, (7, 46)])], last],
        "overlap 1": [lead, [dg.Block("static", [(258, 1), 65, (258, 200)])], last],
        "overlap 3": [lead, [dg.Block("static", [65, (258, 3), (258, 258)])], last],
        "overlap 64": [lead, [dg.Block("dynamic", lits[:10] + [(258, 64), (100, 64)])], last],
        "overlap 258": [lead, [dg.Block("static", lits[:100] + [(258, 258), (258, 100)])], last],
        "copy of a copy": [lead, [dg.Block("static", [(258, W)])] + filler(rng, 20000 - 258) + [dg.Block("static", [(258, 20000)])]
                           + filler(rng, 25000 - 258) + [dg.Block("dynamic", [(258, 25000), (258, 258)])], last],
        "across dynamic blocks": [lead, [dg.Block("dynamic", lits[:50] + [(100, W)]), dg.Block("dynamic", [(100, 100)] + lits[50:90]),
                                         dg.Block("dynamic", [(200, 150), (30, 30000)])], last],
        "stored between": [lead, [dg.Block("static", [(50, 30000)]), dg.Block("stored", data=bytes(lits)), dg.Block("static", [(50, W)])],
                           last],
        # distances above 32768 - 258 with tokens behind them: what is placed behind such a match shares ring slots with its source
        "far match then literals": [lead, filler(rng, 33000) + [dg.Block("static", [(258, W - 1), 200, 201, 202, (258, W - 2), 203, (3, W)]
                                                                         + lits[:80] + [(258, W - 100), (200, W - 30)] + lits[80:160])], last],
        "size 0": [lead, [dg.Block("static", [(50, 30000)])], [], [dg.Block("static", [])], [dg.Block("dynamic", [(50, W), 1])], last],
    }
    return cases


@pytest.mark.parametrize("name", sorted(hand_built()))
def test_hand_built_rows(torch, dev, name):
    rows = hand_built()[name]
    stream, plain = cm.compose_rows(rows, ZLIB)
    x, t = both(torch, dev, stream, ZLIB, plain)
    assert x["nchunks"] == len(rows) and max(t[4]) > 0
    if name == "reach 32768":
        assert t[4][1] == W == t[3][1]
    if name == "reach out_off":
        assert t[4][1] == 40 == t[3][1]
    if name == "size 0":
        assert t[2][2:4] == [0, 0] and t[4][1] > 0 and t[4][4] == W


# ---- refusals, each once ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three_rows():
    """a 3-row stream of one compressor, per frame, with the model's table"""
    out = {}
    for frame in FRAMES:
        stream = cm.sync_writer(cm.cut(text(9000), [3000]), frame)
        x, *t = cm.index_carry(stream, frame)
        assert x["status"] == 0 and x["nchunks"] == 3 and t[4][0] == 0 and min(t[4][1:]) > 0
        out[frame] = (stream, t)
    return out


def test_row_0_reaches_back(torch, dev):
    body = dg.encode([dg.Block("static", [65, (3, 2), 66])], chunk=True) + dg.encode([dg.Block("static", [67], final=True)])
    x = index_check(torch, dev, body, RAW)
    assert x[0]["status"] == 1 and x[0]["nchunks"] == 0 and x[0]["end_offset"] == 0
    # ... and a later row over the start of the stream: the rows in front stay usable
    rows = [dg.encode([dg.Block("static", list(range(40)))], chunk=True), dg.encode([dg.Block("static", [65, (3, 42)])], chunk=True),
            dg.encode([dg.Block("static", [67], final=True)])]
    x = index_check(torch, dev, b"".join(rows), RAW)
    assert x[0] == {"nchunks": 1, "out_bytes": 40, "end_offset": len(rows[0]), "ncandidates": 3, "hdr_bytes": 0, "status": 1}
    assert index_check(torch, dev, b"".join(rows), RAW, max_chunks=2)[0] == x[0]
    assert index_check(torch, dev, b"".join(rows), RAW, max_chunks=1)[0]["status"] == 3


def test_tampered_tables(torch, dev, three_rows):
    stream, t = three_rows[GZIP]

    def run(k, i, v, **kw):
        u = [list(c) for c in t]
        u[k][i] = v
        return decode_check(torch, dev, stream, GZIP, *u, **kw)
    assert run(4, 1, t[3][1] + 1)["status"] == 1
    v = run(4, 1, t[4][1] - 1)
    assert (v["status"], v["bad_chunk"]) == (2, 1)
    v = run(4, 2, 32769)
    assert (v["status"], v["bad_chunk"]) == (1, 2)
    v = run(1, 1, t[1][1] - 1)
    assert (v["status"], v["bad_chunk"]) == (2, 1)
    v = run(3, 2, t[3][2] + 1)
    assert (v["status"], v["bad_chunk"]) == (1, 1)
    v = run(4, 0, 1)
    assert (v["status"], v["bad_chunk"]) == (1, 0)
    assert run(4, 1, t[4][1], cap=8999)["status"] == 3
    assert decode_check(torch, dev, stream, GZIP, [], [], [], [], [])["status"] == 1


@pytest.mark.parametrize("frame,at", ((GZIP, -8), (GZIP, -4), (ZLIB, -1)))
def test_wrong_trailer(torch, dev, three_rows, frame, at):
    """a wrong CRC-32, a wrong ISIZE, a wrong Adler-32"""
    stream, t = three_rows[frame]
    bad = bytearray(stream)
    bad[at] ^= 0x10
    v = decode_check(torch, dev, bytes(bad), frame, *t)
    assert (v["status"], v["bad_chunk"]) == (2, 3)


def test_every_truncation_of_a_three_row_stream(torch, dev):
    stream = cm.sync_writer(cm.cut(text(240), [80]), GZIP)
    assert len(stream) < 400 and cm.index_carry(stream, GZIP)[0]["nchunks"] == 3
    for n in range(len(stream)):
        x = index_check(torch, dev, stream[:n], GZIP)
        assert x[0]["status"] in (1, 2), n


def test_index_status_3_and_the_sizing_call(torch, dev, three_rows):
    stream, t = three_rows[ZLIB]
    x = index_check(torch, dev, stream, ZLIB, max_chunks=0)
    assert x[0]["status"] == 3 and x[0]["nchunks"] == 3
    s = dev.index_stream_carry_call(to_dev(torch, stream), ZLIB, 0, 0, None, None, None, None, None)
    assert (s.status, s.nchunks) == (3, 3)
    x = index_check(torch, dev, stream, ZLIB, max_chunks=2)
    assert x[0]["status"] == 3 and x[0]["out_bytes"] == 6000 and x[5] == t[4][:2]
    *tabs, s = dev.index_stream_carry(to_dev(torch, stream), ZLIB, max_chunks=None)
    assert s.status == 0 and [v & 0xffffffff for v in tabs[4].cpu().tolist()[:3]] == t[4]


# ---- groups -------------------------------------------------------------------------------------------------------------------

def test_groups_do_not_change_the_bytes(torch, dev, pkg):
    data = text(300 * 1024)
    stream = cm.pigz_writer(cm.cut(data, [10000]), GZIP)
    for group in (4096, 65536, 0):
        pkg.lib().hipdeflate_test_carry_group(group)
        both(torch, dev, stream, GZIP, data)


def test_a_fast_path_group_between_two_carried_ones(torch, dev, pkg):
    """rows of 8 KiB, groups of 64 KiB: rows 8..15 each stand alone (full flushes), the groups either side carry the window"""
    data = text(24 * 8192)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = b""
    for i in range(24):
        stream += c.compress(data[i * 8192:(i + 1) * 8192])
        stream += c.flush() if i == 23 else c.flush(zlib.Z_FULL_FLUSH if 7 <= i < 16 else zlib.Z_SYNC_FLUSH)
    reach = cm.index_carry(stream, RAW)[5]
    assert max(reach[8:16]) == 0 and min(reach[1:8]) > 0 and min(reach[17:]) > 0
    pkg.lib().hipdeflate_test_carry_group(65536)
    both(torch, dev, stream, RAW, data)


# ---- the other entry points -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("writer", WRITERS)
def test_host_buffer_form(pkg, writer):
    data = text(100000)
    stream = writer(cm.cut(data, [30000]), GZIP)
    r, out, need, used = pkg.hip_inflate_stream_carry(stream + b"behind the trailer", len(data), GZIP)
    assert (r, out, need, used) == (0, data, len(data), len(stream))
    r, out, need, used = pkg.hip_inflate_stream_carry(stream, len(data) - 1, GZIP)
    assert (r, need, used) == (3, len(data), len(stream))
    assert pkg.hip_inflate_stream_carry(stream[:-9], len(data), GZIP)[0] == 1
    bad = bytearray(stream)
    bad[-8] ^= 1
    assert pkg.hip_inflate_stream_carry(bytes(bad), len(data), GZIP)[0] == 1


def test_device_form_and_bytes_behind_the_trailer(torch, dev, pkg):
    data = text(100000)
    stream = cm.pigz_writer(cm.cut(data, [30000]), ZLIB)
    out, x = dev.inflate_stream_carry(to_dev(torch, stream + b"more"), ZLIB)
    assert bytes(out.cpu().numpy()) == data and x.end_offset == len(stream) and x.status == 0
    with pytest.raises(pkg.HipDeflateError):
        dev.inflate_stream_carry(to_dev(torch, stream[:-5]), ZLIB)


# ---- equality with the existing path --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", FRAMES)
def test_equals_the_existing_path_on_own_full_flush_streams(torch, dev, frame):
    data = text(3 * 65536 + 1)
    strm, _, _ = dev.deflate_stream(to_dev(torch, data), 6, frame, 65536)
    strm = to_dev(torch, bytes(strm.cpu().numpy()))
    n = 8
    old = [torch.full((n,), -2, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int32, torch.int64)]
    new = [torch.full((n,), -2, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int32, torch.int64, torch.int32)]
    a = dev.index_stream_call(strm, frame, n, 0, *old)
    b = dev.index_stream_carry_call(strm, frame, n, 0, *new)
    assert fields(a, X_FIELDS) == fields(b, X_FIELDS) and a.status == 0 and a.nchunks == 5
    for o, w in zip(old, new):
        assert o.cpu().tolist() == w.cpu().tolist()
    assert new[4].cpu().tolist() == [0] * 5 + [-2] * 3
    want, _ = dev.inflate_stream_auto(strm, frame)
    got, _ = dev.inflate_stream_carry(strm, frame)
    assert bytes(got.cpu().numpy()) == bytes(want.cpu().numpy()) == data
