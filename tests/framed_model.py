"""The model of hipdeflate_batch_inflate_framed* and hipdeflate_batch_inflate_size*: what one member answers.

The header and trailer rules are restated from lib/libdeflate/gzip_decompress.c:30-133 and zlib_decompress.c:31-91 (paths
relative to the reference); the stream goes through the oracle's hdo_inflate, which is verdict-identical to libdeflate and
returns the stream's length in bits.  tests/test_framed_model.py holds this model to the reference's own functions.
"""
import ctypes
import zlib

import numpy as np

import hdtest

RAW, ZLIB, GZIP = 0, 4, 5            # HD_FRAME_RAW, HD_FRAME_ZLIB, HD_FRAME_GZIP
OK, BAD_DATA, INSUFFICIENT_SPACE = 0, 1, 3
MAX_IN = 1 << 28                     # HD_INFLATE_MAX_IN
FOOTER = {RAW: 0, ZLIB: 4, GZIP: 8}
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT, FRESERVED = 1, 2, 4, 8, 16, 0xe0


def open_member(m, frame):
    """-> the offset of the DEFLATE payload inside member `m`, or None where the header rules refuse it"""
    n = len(m)
    if frame == RAW:
        return 0
    if frame == ZLIB:
        if n < 6:                                                        # ZLIB_MIN_OVERHEAD
            return None
        hdr = (m[0] << 8) | m[1]
        if hdr % 31 or ((hdr >> 8) & 15) != 8 or (hdr >> 12) > 7 or (hdr >> 5) & 1:
            return None
        return 2
    assert frame == GZIP
    if n < 18:                                                           # GZIP_MIN_OVERHEAD
        return None
    if m[0] != 0x1f or m[1] != 0x8b or m[2] != 8:
        return None
    flg = m[3]
    if flg & FRESERVED:
        return None
    pos = 10
    if flg & FEXTRA:
        xlen = m[10] | (m[11] << 8)
        pos = 12
        if n - pos < xlen + 8:
            return None
        pos += xlen
    for bit in (FNAME, FCOMMENT):
        if flg & bit:
            # `while (*in_next++ != 0 && in_next != in_end)`: behind the NUL, or at the end where there is none
            z = m.find(b"\0", pos)
            pos = n if z < 0 else z + 1
            if n - pos < 8:
                return None
    if flg & FHCRC:
        pos += 2
        if n - pos < 8:
            return None
    return pos


def oracle_inflate_bits(stream, cap):
    """hdo_inflate -> (code, output, bits of stream consumed)"""
    src = hdtest.as_u8(stream)
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    n = ctypes.c_size_t(cap)
    bits = ctypes.c_uint64(0)
    r = hdtest.oracle().hdo_inflate(hdtest._ptr(dst), ctypes.byref(n), hdtest._ptr(src), ctypes.c_size_t(len(src)),
                                    ctypes.byref(bits))
    return r, (dst[:n.value].tobytes() if r == 0 else b""), bits.value


def framed(member, frame, cap):
    """-> (status, out_len, in_used, check, output): hipdeflate_batch_inflate_framed* for one member and `cap` bytes of room"""
    m = bytes(member)
    fail = lambda code: (code, 0, 0, 0, b"")
    if len(m) >= MAX_IN:
        return fail(BAD_DATA)
    pos = open_member(m, frame)
    if pos is None:
        return fail(BAD_DATA)
    foot = FOOTER[frame]
    r, out, bits = oracle_inflate_bits(m[pos:len(m) - foot], cap)
    if r:
        return fail(r)
    used = (bits + 7) // 8
    t = m[pos + used:pos + used + foot]
    if frame == ZLIB:
        check = zlib.adler32(out)
        if int.from_bytes(t, "big") != check:
            return fail(BAD_DATA)
    else:
        check = zlib.crc32(out)
        if frame == GZIP and (int.from_bytes(t[:4], "little") != check or int.from_bytes(t[4:], "little") != len(out) & 0xffffffff):
            return fail(BAD_DATA)
    return OK, len(out), pos + used + foot, check, out


def size(member, frame, room=1 << 16):
    """-> (status, out_size, in_used): hipdeflate_batch_inflate_size* for one member -- the framed verdict in unlimited room
    (the room is grown until the stream fits; 2^32 bytes is where it stops fitting) without the check value"""
    m = bytes(member)
    if len(m) >= MAX_IN:
        return BAD_DATA, 0, 0
    pos = open_member(m, frame)
    if pos is None:
        return BAD_DATA, 0, 0
    foot = FOOTER[frame]
    while True:
        r, out, bits = oracle_inflate_bits(m[pos:len(m) - foot], room)
        if r != INSUFFICIENT_SPACE or room >= (1 << 32) - 1:
            break
        room = min(room * 16, (1 << 32) - 1)
    if r:
        return r, 0, 0
    used = (bits + 7) // 8
    if frame == GZIP and int.from_bytes(m[pos + used + 4:pos + used + 8], "little") != len(out) & 0xffffffff:
        return BAD_DATA, 0, 0
    return OK, len(out), pos + used + foot
