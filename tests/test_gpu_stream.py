"""The single-stream path -- hipdeflate_stream_deflate_dev / _inflate_dev, hipdeflate_check_combine_dev, hip_deflate_stream
and their device.py forms -- against the plain-Python model of tests/stream_model.py.  Bit-exact, no tolerances: the
stream's bytes, the chunk table, every field of the summary, and 64 sentinel bytes in front of and behind every output.
No case provokes a fault: every refused table and every bad trailer is a case the contract of include/hipdeflate.h
defines, each runs once, and none reads or writes outside its buffers.

Where the cases land (hd_stream.hpp, hd_api.hip):
  * fold: part counts at the seams of a wavefront (63 / 64 / 65), a workgroup (255 / 256 / 257), a scan tile and a few
    workgroups (4095 / 4096 / 4097) and of the fold's grid of 256 workgroups (65535 / 65536 / 65537: a lane's second trip);
    lengths mixing 0, 1, 0xffff and 0xffffffff, so that the suffix sums pass 2^32 and 2^35.
  * encode: each axis -- frame, level, chunk, length -- against a default of the others; lengths around one chunk and
    around 64 chunks; windows of 1, 3 and 64 chunks (the running offset and the running check cross windows; Adler-32 and
    CRC-32 carry differently); a level-1 chunk longer than HD_SEG_LIMIT (segments inside a chunk); room one byte short.
  * decode: the round trip, streams zlib wrote with Z_FULL_FLUSH, and every verdict the header names."""
import ctypes
import importlib
import os
import zlib

import numpy as np
import pytest

import hdtest
import stream_model as sm

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0xa5
RAW, ZLIB, GZIP = sm.FRAME_RAW, sm.FRAME_ZLIB, sm.FRAME_GZIP
CHUNK = 4096
DEFAULT_N = 65 * CHUNK + 7
SEG_LIMIT = 320 << 10                # include/hipdeflate_params.h HD_SEG_LIMIT
FIELDS = ("out_bytes", "in_bytes", "bad_chunk", "nchunks", "check", "status")


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


_data, _model = {}, {}


def data_of(n, seed=0):
    """n bytes of one shared master buffer: text, a DNA-like stretch, noise and a run taking turns every 1500 bytes, so
    that chunks of every size hold matches, literals and what only a stored block takes"""
    if seed not in _data:
        s, m, seg = hdtest.synth(), 5 << 20, 1500
        kinds = [np.frombuffer(bytes(s.text_like(m // 4, seed=seed + 1)), dtype=np.uint8),
                 np.frombuffer(bytes(s.fastq_like(m // 4, seed=seed + 2)), dtype=np.uint8),
                 np.frombuffer(bytes(s.random_bytes(m // 4, seed=seed + 3)), dtype=np.uint8), np.zeros(m // 4, dtype=np.uint8)]
        rows = m // 4 // seg
        _data[seed] = np.stack([k[:rows * seg].reshape(rows, seg) for k in kinds], axis=1).tobytes()
    assert n <= len(_data[seed])
    return _data[seed][:n]


def model(n, level, frame, chunk, seed=0):
    """the model's stream, computed once per case and shared (never modified)"""
    key = (n, level, frame, chunk, seed)
    if key not in _model:
        _model[key] = sm.encode(data_of(n, seed), level, frame, chunk)
    return _model[key]


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def u32(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32).copy()).cuda()


def u64(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


def fields(s):
    return {f: getattr(s, f) for f in FIELDS}


def encode_check(torch, dev, data, level, frame, chunk, want, cap=None, table=True):
    """one hipdeflate_stream_deflate_dev held to `want` = (stream, chunk_off, summary) of the model; cap: dst_cap"""
    stream, off, summary = want
    need = len(stream)
    cap = need if cap is None else cap
    summary = dict(summary, status=3 if cap < need else 0)
    buf = torch.full((GUARD + cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    tab = torch.full((len(off) + 2,), -2, dtype=torch.int64, device="cuda") if table else None
    s = dev.deflate_stream_call(to_dev(torch, data), level, frame, chunk, buf[GUARD:], cap, tab[1:] if table else None)
    assert fields(s) == summary
    got = bytes(buf.cpu().numpy())
    assert got[:GUARD] == bytes([SENT]) * GUARD and got[GUARD + cap:] == bytes([SENT]) * GUARD
    if cap >= need:
        assert got[GUARD:GUARD + need] == stream
    if table:
        assert tab.cpu().tolist() == [-2] + off + [-2]
    return s


def decode_check(torch, dev, stream, frame, off, chunk, out_bytes, cap=None, shift=0):
    """one hipdeflate_stream_inflate_dev held to the model's verdict; out starts `shift` bytes off an aligned guard"""
    want, out = sm.decode(stream, frame, off, chunk, out_bytes, cap)
    cap = out_bytes if cap is None else cap
    buf = torch.full((GUARD + shift + cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = dev.inflate_stream_call(to_dev(torch, stream), frame, u64(torch, off), len(off) - 1, chunk, out_bytes,
                                buf[GUARD + shift:], cap)
    got = fields(s)
    if want["check"] is None:
        got["check"] = None
    assert got == want
    b = bytes(buf.cpu().numpy())
    assert b[:GUARD + shift] == bytes([SENT]) * (GUARD + shift) and b[GUARD + shift + cap:] == bytes([SENT]) * GUARD
    if want["status"] in (1, 3):                                               # nothing is inflated
        assert b[GUARD + shift:GUARD + shift + cap] == bytes([SENT]) * cap
    if want["status"] == 0:
        assert b[GUARD + shift:GUARD + shift + out_bytes] == out
    return want


# ---- the fold --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [sm.CRC32, sm.ADLER32])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537])
def test_fold(torch, dev, pkg, n, kind):
    rng = np.random.default_rng(n + kind)
    checks = [int(v) for v in rng.integers(0, 2 ** 32, n)]
    lens = [int(v) for v in rng.choice([0, 1, 0xffff, 0xffffffff], n)]
    if n >= 63:
        assert sum(lens) > 2 ** 35
    if n == 0:
        result = ctypes.c_uint32(99)
        assert pkg.lib().hipdeflate_check_combine_dev(None, None, 0, kind, result, None) == 0
        assert result.value == (1 if kind == sm.ADLER32 else 0)
        return
    assert dev.check_combine(u32(torch, checks), u32(torch, lens), kind) == sm.fold(checks, lens, kind)


def test_fold_of_real_parts_is_zlibs_checksum(torch, dev):
    data = data_of(DEFAULT_N)
    parts = sm.cut(data, 1000) + [b""]
    lens = u32(torch, [len(p) for p in parts])
    assert dev.check_combine(u32(torch, [zlib.crc32(p) for p in parts]), lens, sm.CRC32) == zlib.crc32(data)
    assert dev.check_combine(u32(torch, [zlib.adler32(p) for p in parts]), lens, sm.ADLER32) == zlib.adler32(data)


# ---- encode ----------------------------------------------------------------------------------------------------------

ENCODE_CASES = (
    [(DEFAULT_N, 6, f, CHUNK) for f in (RAW, ZLIB, GZIP)] +
    [(DEFAULT_N, lv, GZIP, CHUNK) for lv in (0, 1, 2, 3)] +
    [(65 * c + 7, 6, GZIP, c) for c in (16, 48, 0xff00)] +
    [(n, 6, GZIP, CHUNK) for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 64 * CHUNK)] +
    [(0, 6, RAW, CHUNK), (0, 6, ZLIB, CHUNK), (1, 1, ZLIB, 16), (65 * 48 + 7, 2, ZLIB, 48)])


@pytest.mark.parametrize("n,level,frame,chunk", ENCODE_CASES)
def test_encode(torch, dev, n, level, frame, chunk):
    want = model(n, level, frame, chunk)
    encode_check(torch, dev, data_of(n), level, frame, chunk, want)
    d = zlib.decompressobj(sm.WBITS[frame])                                    # (the model's stream is one stream to zlib)
    assert d.decompress(want[0]) == data_of(n) and d.eof


@pytest.mark.parametrize("frame", [ZLIB, GZIP])
def test_encode_windows_give_identical_bytes(torch, dev, pkg, frame):
    want = model(DEFAULT_N, 6, frame, CHUNK)
    try:
        for window in (1, 3, 64):
            pkg.lib().hipdeflate_test_stream_window(window)
            encode_check(torch, dev, data_of(DEFAULT_N), 6, frame, CHUNK, want)
    finally:
        pkg.lib().hipdeflate_test_stream_window(0)


def test_encode_level1_segments_inside_a_chunk(torch, dev):
    chunk = SEG_LIMIT + 16
    n = 2 * chunk + chunk // 2
    want = model(n, 1, GZIP, chunk)
    encode_check(torch, dev, data_of(n), 1, GZIP, chunk, want)
    assert zlib.decompress(want[0], 31) == data_of(n)


def test_encode_room(torch, dev, pkg):
    want = model(DEFAULT_N, 6, GZIP, CHUNK)
    need = len(want[0])
    s = encode_check(torch, dev, data_of(DEFAULT_N), 6, GZIP, CHUNK, want, cap=need - 1)
    assert (s.status, s.out_bytes) == (3, need)
    assert encode_check(torch, dev, data_of(DEFAULT_N), 6, GZIP, CHUNK, want, cap=need).status == 0
    try:                                                                       # ... and where the room ends inside a window
        pkg.lib().hipdeflate_test_stream_window(3)
        for cap in (need - 1, need // 2, 16, 0):
            assert encode_check(torch, dev, data_of(DEFAULT_N), 6, GZIP, CHUNK, want, cap=cap, table=cap != 16).out_bytes == need
    finally:
        pkg.lib().hipdeflate_test_stream_window(0)
    bound = pkg.lib().hipdeflate_stream_bound(DEFAULT_N, CHUNK, 6, GZIP)
    assert need <= bound
    assert encode_check(torch, dev, data_of(DEFAULT_N), 6, GZIP, CHUNK, want, cap=bound).status == 0


def test_encode_refuses_what_the_header_rules_out(torch, dev, pkg):
    src = to_dev(torch, bytes(4096))
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    for level, frame, chunk, a, b in ((6, pkg.FRAME_BGZF, 4096, src, dst), (6, GZIP | pkg.FRAME_LATENCY, 4096, src, dst),
                                      (6, GZIP, 24, src, dst), (6, GZIP, 0, src, dst), (6, GZIP, (64 << 20) + 16, src, dst),
                                      (6, GZIP, 4096, src[1:], dst), (6, GZIP, 4096, src, dst[8:])):
        with pytest.raises(pkg.HipDeflateError, match="101"):
            dev.deflate_stream_call(a, level, frame, chunk, b, b.numel(), None)


def test_device_and_host_forms(torch, dev, pkg):
    for frame in (RAW, ZLIB, GZIP):
        data = data_of(DEFAULT_N)
        stream, off, summary = model(DEFAULT_N, 6, frame, CHUNK)
        got, tab, s = dev.deflate_stream(to_dev(torch, data), 6, frame, CHUNK)
        assert bytes(got.cpu().numpy()) == stream and tab.cpu().tolist() == off and fields(s) == summary
        assert bytes(dev.inflate_stream(got, tab, CHUNK, len(data), frame).cpu().numpy()) == data
        assert pkg.hip_deflate_stream(data, 6, frame, CHUNK) == (0, stream)
        assert pkg.hip_deflate_stream(data, 6, frame, CHUNK, cap=len(stream)) == (0, stream)
        assert pkg.hip_deflate_stream(data, 6, frame, CHUNK, cap=len(stream) - 1) == (1, b"")
    assert pkg.hip_deflate_stream(b"", 6, GZIP, CHUNK) == (0, model(0, 6, GZIP, CHUNK)[0])


# ---- decode ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,level,frame,chunk", ENCODE_CASES)
def test_round_trip(torch, dev, n, level, frame, chunk):
    stream, off, summary = model(n, level, frame, chunk)
    want = decode_check(torch, dev, stream, frame, off, chunk, n, shift=3 if frame == ZLIB else 0)
    assert (want["status"], want["check"]) == (0, summary["check"])


def test_round_trip_of_segmented_chunks(torch, dev):
    chunk = SEG_LIMIT + 16
    n = 2 * chunk + chunk // 2
    stream, off, _ = model(n, 1, GZIP, chunk)
    assert decode_check(torch, dev, stream, GZIP, off, chunk, n)["status"] == 0


@pytest.mark.parametrize("frame", [RAW, ZLIB, GZIP])
def test_foreign_stream(torch, dev, frame):
    data = data_of(DEFAULT_N, seed=5)
    stream, off = sm.foreign(data, frame, CHUNK)
    assert decode_check(torch, dev, stream, frame, off, CHUNK, len(data))["status"] == 0
    stream, off = sm.foreign(b"", frame, CHUNK)
    assert decode_check(torch, dev, stream, frame, off, CHUNK, 0)["status"] == 0


def flip(b, i):
    return b[:i] + bytes([b[i] ^ 0x55]) + b[i + 1:]


def test_decode_verdicts(torch, dev):
    n = DEFAULT_N
    stream, off, summary = model(n, 6, GZIP, CHUNK)
    nc = summary["nchunks"]

    def verdict(st=stream, o=off, frame=GZIP, ob=n, cap=None):
        w = decode_check(torch, dev, st, frame, o, CHUNK, ob, cap)
        return w["status"], w["bad_chunk"]
    assert verdict(st=flip(stream, len(stream) - 6)) == (2, nc)                # one flipped byte in the trailer: the CRC
    assert verdict(st=flip(stream, len(stream) - 2)) == (2, nc)                # ... ISIZE
    k = 17
    assert verdict(st=flip(stream, (off[k] + off[k + 1]) // 2))[0] == 2        # one flipped byte inside chunk k
    assert verdict(o=off[:k] + [off[k + 1], off[k]] + off[k + 2:]) == (1, k)   # a table that descends
    assert verdict(o=off[:-1] + [len(stream) + 5]) == (1, nc - 1)              # a table that reaches past nbytes
    assert verdict(o=off[:-2] + [len(stream) + 5, len(stream) + 9]) == (1, nc - 2)
    assert verdict(st=flip(stream, 0)) == (1, nc)                              # a wrong header byte
    assert verdict(st=flip(stream, off[-1])) == (1, nc)                        # a missing 03 00
    assert verdict(cap=n - 1) == (3, nc)                                       # out_cap one short
    assert verdict(ob=n + CHUNK) == (1, nc)                                    # out_bytes that nchunks does not allow
    assert verdict(st=stream[:16], o=[10], ob=0) == (1, 0)                     # too short for its two ends
    zs, zoff, zsum = model(n, 6, ZLIB, CHUNK)
    assert verdict(st=flip(zs, len(zs) - 1), o=zoff, frame=ZLIB) == (2, zsum["nchunks"])
    assert verdict(st=flip(zs, 1), o=zoff, frame=ZLIB) == (1, zsum["nchunks"])  # FCHECK
    rs, roff, rsum = model(n, 6, RAW, CHUNK)
    assert verdict(st=rs, o=roff, frame=RAW) == (0, rsum["nchunks"])


def test_inflate_stream_names_the_bad_chunk(torch, dev, pkg):
    stream, off, _ = model(DEFAULT_N, 6, GZIP, CHUNK)
    with pytest.raises(pkg.HipDeflateError, match="bad_chunk 66 of 66"):
        dev.inflate_stream(to_dev(torch, flip(stream, len(stream) - 6)), off, CHUNK, DEFAULT_N, GZIP)


def test_no_stalls_at_the_end(pkg):
    assert pkg.lib().hipdeflate_stall_count() == 0
