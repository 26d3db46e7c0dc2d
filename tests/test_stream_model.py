"""Pins tests/stream_model.py, the plain-Python model the GPU tests of the single-stream path compare against: both
checksum folds against zlib on real concatenations, the GF(2) arithmetic by its properties where no real buffer reaches,
and the assembled stream through zlib's own inflate in all three wrappers."""
import zlib

import numpy as np
import pytest

import hdtest
import stream_model as sm

PART_LENS = [0, 1, 15, 16, 17, 65535]
_text = {}


def text(n, skip=0):
    """n bytes of one seeded text, made once (the generator's set-up is a second)"""
    if "t" not in _text:
        _text["t"] = bytes(hdtest.synth().text_like(1 << 16, seed=11)) + bytes(hdtest.synth().fastq_like(1 << 15, seed=12))
    return _text["t"][skip:skip + n]


def parts_for(nparts, seed):
    rng = np.random.default_rng(seed)
    lens = [PART_LENS[int(k)] for k in rng.integers(0, len(PART_LENS), nparts)]
    if nparts > 12:                                   # keep the long ones few: the test is about seams, not bytes
        lens = [n if n < 65535 or i % 9 == 0 else 17 for i, n in enumerate(lens)]
    return [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]


@pytest.mark.parametrize("nparts", list(range(1, 71)))
def test_folds_equal_zlib_on_concatenations(nparts):
    parts = parts_for(nparts, nparts)
    whole, lens = b"".join(parts), [len(p) for p in parts]
    crcs, adlers = [zlib.crc32(p) for p in parts], [zlib.adler32(p) for p in parts]
    assert sm.crc_fold(crcs, lens) == zlib.crc32(whole)
    assert sm.crc_fold_np(crcs, lens) == zlib.crc32(whole)
    assert sm.adler_fold(adlers, lens) == zlib.adler32(whole)
    assert sm.fold(crcs, lens, sm.CRC32) == zlib.crc32(whole) and sm.fold(adlers, lens, sm.ADLER32) == zlib.adler32(whole)


def test_every_listed_length_meets_every_other():
    rng = np.random.default_rng(5)
    for a in PART_LENS:
        for b in PART_LENS:
            parts = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (a, b, a)]
            whole, lens = b"".join(parts), [len(p) for p in parts]
            assert sm.crc_fold([zlib.crc32(p) for p in parts], lens) == zlib.crc32(whole)
            assert sm.adler_fold([zlib.adler32(p) for p in parts], lens) == zlib.adler32(whole)


def test_parts_of_length_zero_are_identities_whatever_their_check():
    parts = [b"abc", b"", b"defg", b""]
    lens = [len(p) for p in parts]
    assert sm.crc_fold([zlib.crc32(parts[0]), 0xdeadbeef, zlib.crc32(parts[2]), 7], lens) == zlib.crc32(b"abcdefg")
    assert sm.adler_fold([zlib.adler32(parts[0]), 0xdeadbeef, zlib.adler32(parts[2]), 7], lens) == zlib.adler32(b"abcdefg")
    assert sm.crc_fold([], []) == 0 and sm.adler_fold([], []) == 1 and sm.crc_fold_np([5], [0]) == 0


def test_gf_arithmetic_where_no_buffer_reaches():
    one = 1 << 31
    assert sm.gf_xpow(0) == one and sm.gf_xpow(1) == 1 << 30
    assert sm.gf_xpow(2 ** 32 - 1) == one                                     # x generates the whole multiplicative group
    for a, b in [(2 ** 32 - 3, 2 ** 32 + 5), (2 ** 32, 2 ** 32), (2 ** 61 - 1, 2 ** 61 + 12345), (2 ** 61, 2 ** 32 - 1),
                 (2 ** 63 + 1, 2 ** 61 + 7)]:
        assert sm.gf_xpow(a + b) == sm.gf_mul(sm.gf_xpow(a), sm.gf_xpow(b))
    for n in (0, 1, 2 ** 32 + 1, 2 ** 61 + 3, 2 ** 64 - 1):
        assert sm.gf_xpow8(n) == sm.gf_xpow(8 * n)
    assert sm.POW2[0] == 1 << 30 and all(sm.POW2[k + 1] == sm.gf_mul(sm.POW2[k], sm.POW2[k]) for k in range(63))
    # x^8n is what appending n zero bytes does to a CRC: crc32_combine with an all-zero tail
    a = b"hipdeflate"
    assert sm.crc_fold([zlib.crc32(a), zlib.crc32(bytes(1000))], [len(a), 1000]) == zlib.crc32(a + bytes(1000))


def test_vector_fold_equals_scalar_fold_on_wide_suffixes():
    rng = np.random.default_rng(9)
    lens = [int(v) for v in rng.choice([0, 1, 0xffff, 0xffffffff], 200)]
    checks = [int(v) for v in rng.integers(0, 2 ** 32, 200)]
    assert sum(lens) > 2 ** 35
    assert sm.crc_fold_np(checks, lens) == sm.crc_fold(checks, lens)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 6])
@pytest.mark.parametrize("chunk", [16, 48, 4096])
def test_assembled_stream_is_one_stream_to_zlib(level, chunk):
    data = text(3 * 4096 + 7 if chunk == 4096 else 5 * chunk + 7, skip=chunk + 100 * level)
    for frame in (sm.FRAME_RAW, sm.FRAME_ZLIB, sm.FRAME_GZIP):
        stream, off, s = sm.encode(data, level, frame, chunk)
        d = zlib.decompressobj(sm.WBITS[frame])
        assert d.decompress(stream) == data and d.eof and d.unused_data == b""
        assert s["nchunks"] == len(off) - 1 == (len(data) + chunk - 1) // chunk
        assert s["check"] == (zlib.adler32(data) if frame == sm.FRAME_ZLIB else zlib.crc32(data))
        assert stream[off[-1]:off[-1] + 2] == b"\x03\x00" and len(stream) == off[-1] + 2 + sm.TRAILER[frame] == s["out_bytes"]
        # ... and the model's own decoder takes it back, chunk by chunk
        v, out = sm.decode(stream, frame, off, chunk, len(data))
        assert (v["status"], v["bad_chunk"], v["check"], out) == (0, s["nchunks"], s["check"], data)


def test_empty_input_and_foreign_streams():
    for frame in (sm.FRAME_RAW, sm.FRAME_ZLIB, sm.FRAME_GZIP):
        stream, off, s = sm.encode(b"", 6, frame, 4096)
        assert zlib.decompress(stream, sm.WBITS[frame]) == b"" and off == [len(sm.HEADER[frame])] and s["nchunks"] == 0
        assert s["check"] == (1 if frame == sm.FRAME_ZLIB else 0)
        data = text(3 * 4096 + 100, skip=(1 << 16) - 5000)
        fs, foff = sm.foreign(data, frame, 4096)
        assert zlib.decompress(fs, sm.WBITS[frame]) == data
        v, out = sm.decode(fs, frame, foff, 4096, len(data))
        assert (v["status"], out) == (0, data)
        fs0, foff0 = sm.foreign(b"", frame, 4096)
        assert sm.decode(fs0, frame, foff0, 4096, 0)[0]["status"] == 0


def test_decode_verdicts():
    data = text(5 * 4096 + 9, skip=333)
    stream, off, s = sm.encode(data, 6, sm.FRAME_GZIP, 4096)
    n = s["nchunks"]

    def status(st=stream, o=off, ob=len(data), cap=None):
        v = sm.decode(st, sm.FRAME_GZIP, o, 4096, ob, cap)[0]
        return v["status"], v["bad_chunk"]
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x55]) + b[i + 1:]
    assert status(st=flip(stream, len(stream) - 6)) == (2, n)                  # the CRC of the trailer
    assert status(st=flip(stream, len(stream) - 1)) == (2, n)                  # ISIZE
    assert status(o=off[:2] + [off[3], off[2]] + off[4:]) == (1, 2)            # a table that descends
    assert status(o=off[:-1] + [len(stream) + 5]) == (1, n - 1)                # ... that reaches past nbytes
    assert status(st=flip(stream, 0)) == (1, n)                                # a wrong header byte
    assert status(st=flip(stream, off[-1])) == (1, n)                          # a missing 03 00
    assert status(cap=len(data) - 1) == (3, n)
    assert status(ob=len(data) + 4096) == (1, n)                               # out_bytes that nchunks does not allow
    st2, bc = status(st=flip(stream, (off[2] + off[3]) // 2))
    assert st2 == 2 and bc in (2, n)                                           # inside chunk 2: the chunk, or else the check
