"""Plain-Python model of the single-stream path (include/hipdeflate.h, "one stream from a device buffer"):
  * the two folds -- the CRC-32 / Adler-32 of a concatenation from the checks and lengths of its parts, in the
    order-independent form the device uses (every part moved over the bytes behind it, the contributions added);
  * the stream: header | the CPU twin's flush form of every chunk | 03 00 | trailer, with its chunk table and summary;
  * the decoder's verdicts on a stream and a table, in the order the header gives them.
No GPU, no product code: hdtest's oracle (the twin, the flush-rule inflate) and zlib's checksums."""
import zlib

import numpy as np

import hdtest

POLY = 0xedb88320
ADLER_MOD = 65521
CRC32, ADLER32 = 0, 1
FRAME_RAW, FRAME_ZLIB, FRAME_GZIP = 0, 4, 5
HEADER = {FRAME_RAW: b"", FRAME_ZLIB: bytes.fromhex("78da"), FRAME_GZIP: bytes.fromhex("1f8b0800000000000200")}
TRAILER = {FRAME_RAW: 0, FRAME_ZLIB: 4, FRAME_GZIP: 8}
WBITS = {FRAME_RAW: -15, FRAME_ZLIB: 15, FRAME_GZIP: 31}
KIND = {FRAME_RAW: CRC32, FRAME_ZLIB: ADLER32, FRAME_GZIP: CRC32}
INFLATE_MAX_IN = 1 << 28             # include/hipdeflate_params.h HD_INFLATE_MAX_IN


# ---- GF(2)[x] / P, reflected bit order: x^0 is bit 31 ---------------------------------------------------------------

def gf_mul(a, b):
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def gf_xpow(n):
    """x^n mod P for any n >= 0 (hd_host_util.h gf_xpow)"""
    p, sq = 1 << 31, 1 << 30
    while n:
        if n & 1:
            p = gf_mul(sq, p)
        sq = gf_mul(sq, sq)
        n >>= 1
    return p


POW2 = [gf_xpow(1 << k) for k in range(64)]      # x^(2^k): the device's table


def gf_xpow8(n):
    """x^(8 n): x^n, squared three times"""
    p = gf_xpow(n)
    for _ in range(3):
        p = gf_mul(p, p)
    return p


def suffixes(lens):
    """S_i: the bytes behind part i"""
    out, s = [0] * len(lens), 0
    for i in range(len(lens) - 1, -1, -1):
        out[i] = s
        s += int(lens[i])
    return out


def crc_fold(checks, lens):
    """XOR over i of check[i] * x^(8 S_i); a part of length 0 is an identity"""
    r = 0
    for c, n, s in zip(checks, lens, suffixes(lens)):
        if n:
            r ^= gf_mul(int(c), gf_xpow8(s))
    return r


def adler_fold(checks, lens):
    """A = 1 + sum (a_i - 1), B = sum b_i + sum (a_i - 1) (S_i mod 65521), both mod 65521"""
    a, b = 1, 0
    for c, n, s in zip(checks, lens, suffixes(lens)):
        if n:
            a1 = ((int(c) & 0xffff) - 1) % ADLER_MOD
            a += a1
            b += (int(c) >> 16) % ADLER_MOD + a1 * (s % ADLER_MOD)
    return ((b % ADLER_MOD) << 16) | (a % ADLER_MOD)


def _gf_mul_np(a, b):
    a, b = a.astype(np.uint64), b.astype(np.uint64).copy()
    p = np.zeros_like(a)
    for i in range(32):
        p ^= np.where((a >> np.uint64(31 - i)) & np.uint64(1), b, np.uint64(0))
        b = (b >> np.uint64(1)) ^ np.where(b & np.uint64(1), np.uint64(POLY), np.uint64(0))
    return p


def crc_fold_np(checks, lens):
    """crc_fold over arrays: the same formula, all parts at once (tests/test_stream_model.py holds it to crc_fold)"""
    s = suffixes(lens)
    keep = [i for i, n in enumerate(lens) if n]
    if not keep:
        return 0
    S = np.array([s[i] for i in keep], dtype=np.uint64)
    c = np.array([int(checks[i]) for i in keep], dtype=np.uint64)
    p = np.full(len(keep), 1 << 31, dtype=np.uint64)
    for k in range(max(int(v).bit_length() for v in S.tolist())):
        bit = (S >> np.uint64(k)) & np.uint64(1)
        if bit.any():
            p = np.where(bit, _gf_mul_np(p, np.full(len(keep), POW2[k], dtype=np.uint64)), p)
    for _ in range(3):
        p = _gf_mul_np(p, p)
    return int(np.bitwise_xor.reduce(_gf_mul_np(c, p)))


def fold(checks, lens, kind):
    if kind == ADLER32:
        return adler_fold(checks, lens)
    return crc_fold_np(checks, lens) if len(lens) > 64 else crc_fold(checks, lens)


# ---- the stream ------------------------------------------------------------------------------------------------------

def cut(data, chunk):
    return [data[i:i + chunk] for i in range(0, len(data), chunk)]


def part_check(part, kind):
    return zlib.adler32(part) if kind == ADLER32 else zlib.crc32(part)


def trailer(frame, check, nbytes):
    if frame == FRAME_ZLIB:
        return check.to_bytes(4, "big")
    if frame == FRAME_GZIP:
        return check.to_bytes(4, "little") + (nbytes & 0xffffffff).to_bytes(4, "little")
    return b""


def assemble(frame, coded, check, nbytes):
    """header | the coded chunks | 03 00 | trailer -> (stream, chunk_off: nchunks + 1 entries)"""
    off, pos = [], len(HEADER[frame])
    for c in coded:
        off.append(pos)
        pos += len(c)
    off.append(pos)
    return HEADER[frame] + b"".join(coded) + b"\x03\x00" + trailer(frame, check, nbytes), off


def encode(data, level, frame, chunk, dst_cap=None):
    """what hipdeflate_stream_deflate_dev answers -> (stream, chunk_off, summary as a dict)"""
    data = bytes(data)
    parts = cut(data, chunk)
    coded = []
    for p in parts:
        r, b = hdtest.oracle_twin_flush(p, level)
        assert r == 0
        coded.append(b)
    kind = KIND[frame]
    check = fold([part_check(p, kind) for p in parts], [len(p) for p in parts], kind)
    stream, off = assemble(frame, coded, check, len(data))
    status = 3 if dst_cap is not None and dst_cap < len(stream) else 0
    return stream, off, {"out_bytes": len(stream), "in_bytes": len(data), "bad_chunk": len(parts), "nchunks": len(parts),
                         "check": check, "status": status}


def header_ok(frame, stream):
    if frame == FRAME_GZIP:
        return stream[:4] == bytes.fromhex("1f8b0800")
    if frame == FRAME_ZLIB:
        cmf, flg = stream[0], stream[1]
        return (cmf & 15) == 8 and (cmf >> 4) <= 7 and not (flg & 0x20) and ((cmf << 8) | flg) % 31 == 0
    return True


def decode(stream, frame, chunk_off, chunk, out_bytes, out_cap=None):
    """what hipdeflate_stream_inflate_dev answers -> (summary as a dict, output or None); nchunks = len(chunk_off) - 1.
    summary["check"] is None where the header leaves it unspecified (a bad chunk) or nothing was inflated."""
    stream, n = bytes(stream), len(chunk_off) - 1
    hdr, trl = len(HEADER[frame]), TRAILER[frame]
    out_cap = out_bytes if out_cap is None else out_cap

    def verdict(status, bad, check=None, done=False):
        return {"out_bytes": out_bytes if done else 0, "in_bytes": len(stream) if done else 0, "bad_chunk": bad, "nchunks": n,
                "check": check, "status": status}

    # status 1: the arguments, then the table entry by entry (the lowest entry at fault)
    if (out_bytes + chunk - 1) // chunk != n or len(stream) < hdr + 2 + trl:
        return verdict(1, n), None
    limit = len(stream) - 2 - trl
    faults = []
    for i in range(n):
        o, nx = chunk_off[i], chunk_off[i + 1]
        if o < hdr or o >= nx or nx > limit or nx - o >= INFLATE_MAX_IN:
            faults.append(i)
    o = chunk_off[n]
    if o < hdr or o != limit or stream[o:o + 2] != b"\x03\x00" or not header_ok(frame, stream):
        faults.append(n)
    if faults:
        return verdict(1, min(faults)), None
    if out_cap < out_bytes:
        return verdict(3, n), None
    # status 2: the lowest bad chunk, else the whole stream's check / ISIZE
    outs, bad = [], None
    for i in range(n):
        want = min(chunk, out_bytes - i * chunk)
        r, b = hdtest.oracle_inflate_flushed(stream[chunk_off[i]:chunk_off[i + 1]], want)
        if (r != 0 or len(b) != want) and bad is None:
            bad = i
        outs.append(b if r == 0 and len(b) == want else bytes(want))
    if bad is not None:
        return verdict(2, bad, None, True), None
    out = b"".join(outs)
    kind = KIND[frame]
    check = fold([part_check(p, kind) for p in outs], [len(p) for p in outs], kind)
    t = stream[len(stream) - trl:]
    ok = True
    if frame == FRAME_ZLIB:
        ok = t == check.to_bytes(4, "big")
    elif frame == FRAME_GZIP:
        ok = t == check.to_bytes(4, "little") + (out_bytes & 0xffffffff).to_bytes(4, "little")
    return verdict(0 if ok else 2, n, check, True), out


def foreign(data, frame, chunk, level=6):
    """a stream of another writer, cut the same way: zlib with Z_FULL_FLUSH behind every chunk -> (stream, chunk_off)"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[frame])
    stream, off = b"", []
    for i, p in enumerate(cut(bytes(data), chunk)):
        b = c.compress(p) + c.flush(zlib.Z_FULL_FLUSH)
        if i == 0:                                   # the header comes out with the first bytes
            first = len(stream)
            stream += b
            off.append(first + len(header_of(frame, b)))
        else:
            off.append(len(stream))
            stream += b
    if not off:
        stream = c.flush()                           # header | 03 00 | trailer
        return stream, [len(stream) - 2 - TRAILER[frame]]
    off.append(len(stream))
    stream += c.flush()
    return stream, off


def header_of(frame, b):
    return b[:{FRAME_RAW: 0, FRAME_ZLIB: 2, FRAME_GZIP: 10}[frame]]
