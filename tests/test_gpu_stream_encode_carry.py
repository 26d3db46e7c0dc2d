"""The stream encoder whose chunks carry the window -- hipdeflate_stream_deflate_carry_dev, hip_deflate_stream_carry and their
device.py forms -- against tests/stream_encode_carry_model.py: per chunk, the tokens read out of the device's stream are the
tokens the CPU twin's one-block parse of (history || chunk) makes behind the seam.  Bit-exact, no tolerances.

Every stream made here is held to the form first (carry()): zlib, in the frame's wrapper, returns the input -- which holds the
trailer too, so a check value that took in history bytes fails there --, chunk_off ascends, every chunk ends in 00 00 ff ff
and the summary is complete.  No case provokes a fault; every refusal is one the header defines.

Where the cases land (hd_deflate_wg.hpp parse_wg<..., PRIMED>, launch_wg; hd_api.hip stream_deflate_impl):
  * chunk 1040: prime rounds down to 1024 and the source lies 16 bytes into a piece of the input;
  * 16 KiB: history + chunk = 48 pieces, the ring holds both whole (the bulk path);
  * 48 KiB: the whole window with a chunk longer than it; 64 and 96 KiB: 96 and 128 pieces pass through the ring of 64 (the
    filler path: chunk pieces take the places of history pieces while parsers still read them);
  * last chunks of 1 .. 1025 bytes: the block's edge rules in (history || chunk) coordinates;
  * a repeat at distance exactly 32768; chunks that are all history; the seam between two windows of chunks; 520 chunks: the
    parse beside its emit kernel, in one sub-batch and in three."""
import importlib
import os
import zlib

import numpy as np
import pytest

import hdtest
import stream_encode_carry_model as cm

pytestmark = pytest.mark.gpu

RAW, ZLIB, GZIP = 0, 4, 5            # include/hipdeflate.h HD_FRAME_RAW / _ZLIB / _GZIP
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
HDR = {RAW: 0, ZLIB: 2, GZIP: 10}
GUARD, SENT = 64, 0xa5
FIELDS = ("out_bytes", "in_bytes", "bad_chunk", "nchunks", "check", "status")
# chunk_bytes -> bytes of input: the fewest chunks that reach the full window, and a short last one
SHAPES = {1040: 5 * 1040 + 5, 16 << 10: (64 << 10) + 1023, 48 << 10: (96 << 10) + 6, 64 << 10: (128 << 10) + 63, 96 << 10: (192 << 10) + 64}
TAILS = (1, 5, 6, 63, 64, 1023, 1025)


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    assert (p.FRAME_RAW, p.FRAME_ZLIB, p.FRAME_GZIP) == (RAW, ZLIB, GZIP)
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


_data, _streams = {}, {}


def data_of(kind, n):
    """n bytes of one master buffer per kind (never modified)"""
    if kind not in _data:
        s, m = hdtest.synth(), 1100 << 10
        if kind == "text":
            _data[kind] = bytes(s.text_like(m, seed=21))
        elif kind == "fastq":
            _data[kind] = bytes(s.fastq_like(m, seed=22))
        else:
            _data[kind] = bytes(s.random_bytes(32 << 10, seed=23))
    assert n <= len(_data[kind])
    return _data[kind][:n]


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def fields(s):
    return {f: getattr(s, f) for f in FIELDS}


def check_form(data, frame, chunk, stream, off, s):
    """what every stream of this encoder is held to"""
    n, nchunks = len(data), (len(data) + chunk - 1) // chunk
    want = zlib.adler32(data) if frame == ZLIB else zlib.crc32(data)
    assert fields(s) == dict(out_bytes=len(stream), in_bytes=n, bad_chunk=nchunks, nchunks=nchunks, check=want, status=0)
    d = zlib.decompressobj(WBITS[frame])
    assert d.decompress(stream) == data and d.eof and d.unused_data == b""
    assert len(off) == nchunks + 1 and off[0] == HDR[frame] and all(a + 5 <= b for a, b in zip(off, off[1:]))
    assert all(stream[o - 4:o] == b"\x00\x00\xff\xff" for o in off[1:])
    assert stream[off[-1]:off[-1] + 2] == b"\x03\x00" and off[-1] + 2 + (8 if frame == GZIP else 4 if frame == ZLIB else 0) == len(stream)


def carry(torch, dev, data, level, frame, chunk, key=None):
    """(stream, chunk_off) of one device.deflate_stream_carry, held to the form; key: made once and shared"""
    if key is not None and key in _streams:
        return _streams[key]
    got, tab, s = dev.deflate_stream_carry(to_dev(torch, data), level, frame, chunk)
    r = bytes(got.cpu().numpy()), tab.cpu().tolist()
    check_form(data, frame, chunk, r[0], r[1], s)
    if key is not None:
        _streams[key] = r
    return r


def plain(torch, dev, data, level, frame, chunk):
    got, tab, _ = dev.deflate_stream(to_dev(torch, data), level, frame, chunk)
    return bytes(got.cpu().numpy()), tab.cpu().tolist()


def check_chunk_tokens(data, level, chunk, stream, off, i):
    """chunk i of the device's stream: its tokens are the model's, and they rebuild the chunk behind its history"""
    s, prime, n = cm.span(data, i, chunk)
    toks, out = cm.stream_tokens(stream[off[i]:off[i + 1]], history=data[s - prime:s])
    assert out == data[s:s + n], (i, level, chunk)
    want = cm.expected_tokens(data, i, chunk, level)
    if toks != want:
        k = next((j for j, (a, b) in enumerate(zip(toks, want)) if a != b), min(len(toks), len(want)))
        raise AssertionError("chunk %d (level %d, chunk_bytes %d, prime %d): token %d is %r, the model's %r (%d / %d tokens)"
                             % (i, level, chunk, prime, k, toks[k:k + 1], want[k:k + 1], len(toks), len(want)))
    return toks


# ---- token identity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", sorted(SHAPES))
@pytest.mark.parametrize("level", [3, 4, 5, 6])
@pytest.mark.parametrize("kind", ["text", "fastq"])
def test_tokens_are_the_one_block_parse_behind_the_seam(torch, dev, kind, level, chunk):
    data = data_of(kind, SHAPES[chunk])
    stream, off = carry(torch, dev, data, level, RAW, chunk, key=(kind, level, chunk))
    reaching = 0
    for i in range(len(off) - 1):
        toks = check_chunk_tokens(data, level, chunk, stream, off, i)
        reaching += sum(1 for p, ln, v in toks if ln and v > p)
    assert reaching > 0                                    # the history is used
    # chunk 0 has no history: its bytes are the independent form's
    ind, ioff = plain(torch, dev, data, level, RAW, chunk)
    assert stream[off[0]:off[1]] == ind[ioff[0]:ioff[1]]
    assert len(stream) < len(ind)
    if level == 6:                                         # levels 7..9 are level 6
        assert carry(torch, dev, data, 9, RAW, chunk)[0] == stream


def test_prime_reaches_the_window_in_steps_of_a_piece(torch, dev):
    """chunks of 1040 bytes up to the first whose history is the whole window: prime(i) = 1024 i up to 31744, then 32768"""
    chunk, n = 1040, 34 * 1040 + 5
    data = data_of("text", n)
    stream, off = carry(torch, dev, data, 6, RAW, chunk)
    assert [cm.prime_of(i, chunk) for i in (31, 32, 33, 34)] == [31744, 32768, 32768, 32768]
    for i in (1, 2, 30, 31, 32, 33, 34):
        check_chunk_tokens(data, 6, chunk, stream, off, i)


@pytest.mark.parametrize("tail", TAILS)
def test_short_last_chunks(torch, dev, tail):
    chunk = 16 << 10
    for kind, level in (("text", 6), ("fastq", 3)):
        data = data_of(kind, 2 * chunk + tail)
        stream, off = carry(torch, dev, data, level, RAW, chunk)
        assert len(off) == 4
        for i in range(3):
            check_chunk_tokens(data, level, chunk, stream, off, i)


def test_distance_edge(torch, dev):
    """one random 32 KiB chunk four times over, in chunks of 32 KiB: every later chunk is matches at distance 32768 exactly"""
    chunk = 32 << 10
    data = data_of("random", chunk) * 4
    stream, off = carry(torch, dev, data, 6, GZIP, chunk)
    for i in (1, 2, 3):
        toks, out = cm.stream_tokens(stream[off[i]:off[i + 1]], history=data[(i - 1) * chunk:i * chunk])
        assert out == data[i * chunk:(i + 1) * chunk]
        dists = [v for p, ln, v in toks if ln]
        assert dists and max(dists) == 32768 and sum(ln for p, ln, v in toks if ln and v == 32768) > chunk * 9 // 10
        assert off[i + 1] - off[i] <= chunk // 16


# ---- reach and gain ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [3, 4, 5, 6])
def test_reach_and_gain(torch, dev, pkg, level):
    chunk, reps = 16 << 10, 8
    data = data_of("random", chunk) * reps
    stream, off = carry(torch, dev, data, level, GZIP, chunk)
    assert all(off[i + 1] - off[i] <= chunk // 16 for i in range(1, reps)), [b - a for a, b in zip(off, off[1:])]
    strm = to_dev(torch, stream)
    in_off, in_len, out_size, out_off, reach, x = dev.index_stream_carry(strm, GZIP)
    assert (x.status, x.nchunks, x.out_bytes) == (0, reps + 1, len(data))     # (the 03 00 is a row of its own, of no bytes)
    assert in_off[:reps + 1].cpu().tolist() == off
    reach = reach[:reps].cpu().tolist()
    assert all(0 < reach[i] <= cm.prime_of(i, chunk) for i in range(1, reps)), reach
    out, _ = dev.inflate_stream_carry(strm, GZIP)
    assert bytes(out.cpu().numpy()) == data
    # the decode by chunk table stops at the first chunk that reaches back
    tab = torch.from_numpy(np.array(off, dtype=np.int64)).cuda()
    room = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_call(strm, GZIP, tab, reps, chunk, len(data), room, len(data))
    assert (s.status, s.bad_chunk) == (2, 1)


# ---- identity where there is no history ---------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [RAW, ZLIB, GZIP])
def test_one_chunk_or_none_is_the_independent_form(torch, dev, frame):
    chunk = 16 << 10
    for n in (0, 1, chunk - 16, chunk):
        for level in (3, 6):
            data = data_of("text", n)
            assert carry(torch, dev, data, level, frame, chunk) == plain(torch, dev, data, level, frame, chunk)


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("chunk", sorted(SHAPES))
def test_levels_without_a_window_are_the_independent_form(torch, dev, level, chunk):
    for kind, frame in (("text", GZIP), ("fastq", ZLIB)):
        data = data_of(kind, SHAPES[chunk])
        assert carry(torch, dev, data, level, frame, chunk) == plain(torch, dev, data, level, frame, chunk)
    for n in (0, 1, chunk):
        assert carry(torch, dev, data_of("text", n), level, RAW, chunk) == plain(torch, dev, data_of("text", n), level, RAW, chunk)


# ---- windows of chunks, the parse beside its emit kernel ----------------------------------------------------------------

@pytest.mark.parametrize("frame", [ZLIB, GZIP])
def test_window_seam(torch, dev, pkg, frame):
    chunk = 16 << 10
    data = data_of("text", 10 * chunk)
    one = carry(torch, dev, data, 6, frame, chunk)
    try:
        pkg.lib().hipdeflate_test_stream_window(3)
        cut = carry(torch, dev, data, 6, frame, chunk)
    finally:
        pkg.lib().hipdeflate_test_stream_window(0)
    assert cut == one
    for i in (3, 6, 9):                                    # the first chunk of a window is primed like any other
        check_chunk_tokens(data, 6, chunk, cut[0], cut[1], i)


def test_beside_schedule(torch, dev, pkg):
    chunk, nchunks = 2 << 10, 520
    data = data_of("text", nchunks * chunk)
    whole = carry(torch, dev, data, 6, GZIP, chunk)
    try:
        pkg.lib().hipdeflate_test_beside(3, 200)           # sub-batches of 200, 200 and 120 chunks
        walked = carry(torch, dev, data, 6, GZIP, chunk)
    finally:
        pkg.lib().hipdeflate_test_beside(3, 0)
    assert walked == whole
    for i in (0, 1, 33, 511, 519):
        check_chunk_tokens(data, 6, chunk, whole[0], whole[1], i)


# ---- room, refusals, the host form ------------------------------------------------------------------------------------------

def call(torch, dev, data, level, frame, chunk, cap, table=True):
    """one deflate_stream_carry_call into `cap` bytes between guards -> (summary, the room's bytes, chunk_off)"""
    nchunks = (len(data) + chunk - 1) // chunk
    buf = torch.full((GUARD + cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    tab = torch.full((nchunks + 3,), -2, dtype=torch.int64, device="cuda") if table else None
    s = dev.deflate_stream_carry_call(to_dev(torch, data), level, frame, chunk, buf[GUARD:], cap, tab[1:] if table else None)
    got = bytes(buf.cpu().numpy())
    assert got[:GUARD] == bytes([SENT]) * GUARD and got[GUARD + cap:] == bytes([SENT]) * GUARD
    off = tab.cpu().tolist() if table else None
    assert off is None or (off[0] == -2 and off[-1] == -2)
    return s, got[GUARD:GUARD + cap], off[1:-1] if table else None


def test_room(torch, dev, pkg):
    chunk = 4096
    data = data_of("text", 65 * chunk + 7)
    stream, off = carry(torch, dev, data, 6, GZIP, chunk)
    need = len(stream)
    s, got, tab = call(torch, dev, data, 6, GZIP, chunk, need)
    assert (s.status, s.out_bytes) == (0, need) and got == stream and tab == off
    s, _, tab = call(torch, dev, data, 6, GZIP, chunk, need - 1)
    assert (s.status, s.out_bytes, s.nchunks, s.in_bytes) == (3, need, 66, len(data)) and tab == off
    try:                                                   # ... and where the room ends inside a window
        pkg.lib().hipdeflate_test_stream_window(3)
        for cap in (need - 1, need // 2, 16, 0):
            s, _, _ = call(torch, dev, data, 6, GZIP, chunk, cap, table=cap != 16)
            assert (s.status, s.out_bytes) == (3, need)
    finally:
        pkg.lib().hipdeflate_test_stream_window(0)
    s = dev.deflate_stream_carry_call(to_dev(torch, data), 6, GZIP, chunk, None, 0, None)      # the sizing call
    assert (s.status, s.out_bytes) == (3, need)
    # the bound suffices where nothing can be coded: chunks as stored blocks + flush
    noise = bytes(hdtest.synth().random_bytes(5 * chunk + 100, seed=31))
    bound = pkg.lib().hipdeflate_stream_bound(len(noise), chunk, 6, GZIP)
    s, got, _ = call(torch, dev, noise, 6, GZIP, chunk, bound)
    assert s.status == 0 and len(noise) < s.out_bytes <= bound and zlib.decompress(got[:s.out_bytes], 31) == noise


def test_refuses_what_the_independent_call_refuses(torch, dev, pkg):
    src = to_dev(torch, bytes(4096))
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    for level, frame, chunk, a, b in ((6, pkg.FRAME_BGZF, 4096, src, dst), (6, GZIP | pkg.FRAME_LATENCY, 4096, src, dst),
                                      (6, GZIP, 24, src, dst), (6, GZIP, 0, src, dst), (6, GZIP, (64 << 20) + 16, src, dst),
                                      (6, GZIP, 4096, src[1:], dst), (6, GZIP, 4096, src, dst[8:])):
        for f in (dev.deflate_stream_carry_call, dev.deflate_stream_call):
            with pytest.raises(pkg.HipDeflateError, match="101"):
                f(a, level, frame, chunk, b, b.numel(), None)
    with pytest.raises(ValueError):
        dev.deflate_stream_carry(src, 6, GZIP, 24)


def test_host_form(torch, dev, pkg):
    chunk = 16 << 10
    data = data_of("fastq", 5 * chunk + 63)
    for frame in (RAW, ZLIB, GZIP):
        stream, _ = carry(torch, dev, data, 6, frame, chunk)
        assert pkg.hip_deflate_stream_carry(data, 6, frame, chunk) == (0, stream)
        assert pkg.hip_deflate_stream_carry(data, 6, frame, chunk, cap=len(stream)) == (0, stream)
        assert pkg.hip_deflate_stream_carry(data, 6, frame, chunk, cap=len(stream) - 1) == (1, b"")
    assert pkg.hip_deflate_stream_carry(data, 1, GZIP, chunk) == pkg.hip_deflate_stream(data, 1, GZIP, chunk)
    assert pkg.hip_deflate_stream_carry(b"", 6, GZIP, chunk) == pkg.hip_deflate_stream(b"", 6, GZIP, chunk)
