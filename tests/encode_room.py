"""The output room of every encode path, restated from the headers (the room half of the contract; what the members
hold is encode_contracts.py's).

include/hipdeflate.h: member i of a batch goes to out + i*out_stride, at most min(out_stride, out_cap) bytes are
written, status 1 = does not fit.  What "fits" means for each form:

  * payload room R = min(stride, cap), clamped to 65536 for BGZF, minus the frame's header and trailer bytes;
  * a member fits iff R >= need(block, level, form), and a member that fits is byte for byte the unlimited-room
    member of the form chosen for that room:
      level 0                           HD_STORED_SIZE(n), + 5 in flush form;
      levels 1..2, n > HD_SEG_LIMIT     HD_SEG_WORST(n, flush), whatever the data (the segmented form);
      latency form, levels 1..2,        the latency member when R >= HD_SEGN_WORST(n, HD_LAT_SEG_BYTES(level),
        n > HD_LAT_SEG_BYTES(level)     flush), else the ordinary member and its need (the twin's twin());
      otherwise, non-flush              the member's length;
      otherwise, flush                  ceil(end bit of the last data block / 8) + 5: the flush suffix (3 header
                                        bits, alignment, 00 00 ff ff: 4 or 5 bytes) is reserved at 5;
  * the device batch path at levels >= HD_WG_LEVEL refuses a block longer than min(stride, cap) (no length known
    to the host); the host batch path sizes the parse by the longest block instead;
  * the device batch path in latency form takes the latency member of a block longer than HD_SEG_LIMIT or none
    (the twin and the per-block codecs fall back to HD_SEG_BYTES segments there).

Nothing here calls a kernel; the twin is called only through `Block` (one unlimited-room call per form).
"""
import collections
import os
import re

import numpy as np

import deflate_tokens
import encode_contracts as ec
import hdtest

_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hipdeflate.h")
_FRAME_IDS = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+HD_FRAME_(\w+)\s+(0x[0-9a-fA-F]+|\d+)",
                                                               open(_H).read())}
RAW, BGZF, MIGZ, RAW_FLUSH, ZLIB, GZIP = (_FRAME_IDS[k] for k in ("RAW", "BGZF", "MIGZ", "RAW_FLUSH", "ZLIB", "GZIP"))
LATENCY = _FRAME_IDS["LATENCY"]
# header / trailer bytes of each frame (hipdeflate.h HD_FRAME_*: 18 B header + CRC32 + ISIZE, 20 B + the same, ...)
FRAME_BYTES = {RAW: (0, 0), RAW_FLUSH: (0, 0), BGZF: (18, 8), MIGZ: (20, 8), ZLIB: (2, 4), GZIP: (10, 8)}
FRAME_NAMES = {RAW: "raw", RAW_FLUSH: "raw_flush", BGZF: "bgzf", MIGZ: "migz", ZLIB: "zlib", GZIP: "gzip"}
BGZF_MAX = 65536
FLUSH_RESERVE = 5
LAT_SEG, SEG_LIMIT, SEG_BYTES, WG_LEVEL = ec.LAT_SEG, ec.SEG_LIMIT, ec.SEG_BYTES, ec.WG_LEVEL
stored_size, seg_worst = ec.stored_size, ec.seg_worst


def payload_room(frame, stride, cap):
    r = min(stride, cap)
    if frame == BGZF:
        r = min(r, BGZF_MAX)
    hdr, trl = FRAME_BYTES[frame]
    return r - hdr - trl


def flush_need(member):
    """ceil(end bit of the last data block / 8) + 5 for a member in flush form (data blocks, then the empty stored
    block a full flush ends in)"""
    st = deflate_tokens.read(member, expand=False, stop_at_final=False)
    assert st.blocks and st.blocks[-1].sync_flush, "not a flush-form member"
    data = st.blocks[:-1]
    end = data[-1].end_bit if data else 0
    return (end + 7) // 8 + FLUSH_RESERVE


Choice = collections.namedtuple("Choice", "fits member kind")     # kind: 'ordinary' | 'latency' | None (refused)


class Block:
    """One block at one level in one of the two stream forms (flush or not): the unlimited-room members of the
    ordinary and (levels 1..2, long blocks) the latency form, and what each needs."""

    def __init__(self, data, level, flush):
        self.data, self.level, self.flush = bytes(data), level, flush
        n = len(self.data)
        big = 2 * n + 65536 + 1024
        twin = hdtest.oracle_twin_flush if flush else hdtest.oracle_twin
        r, self.ordinary = twin(self.data, level, cap=big)
        assert r == 0, ("twin refused an unlimited room", n, level, flush)
        sfx = FLUSH_RESERVE if flush else 0
        self.stored_need = stored_size(n) + sfx
        if level <= 0:
            self.need = self.stored_need
        elif level < WG_LEVEL and n > SEG_LIMIT:
            self.need = seg_worst(n, SEG_BYTES, flush)
        elif flush:
            self.need = flush_need(self.ordinary)
        else:
            self.need = len(self.ordinary)
        self.latency = None
        self.need_lat = None
        if 1 <= level < WG_LEVEL and n > LAT_SEG[level]:
            self.need_lat = seg_worst(n, LAT_SEG[level], flush)
            r, self.latency = (hdtest.codec_twin_flush if flush else hdtest.codec_twin)(self.data, level, cap=big)
            assert r == 0

    def choose(self, room, latency=False, device=False):
        """what a path makes of the block at payload room `room`: the twin / the per-block codecs (device False) or
        the device batch path (device True, room = what min(stride, cap) leaves)"""
        if latency and self.latency is not None:
            if room >= self.need_lat:
                return Choice(True, self.latency, "latency")
            if device and len(self.data) > SEG_LIMIT:
                return Choice(False, None, None)
        if room >= self.need:
            return Choice(True, self.ordinary, "ordinary")
        return Choice(False, None, None)

    def edge_rooms(self, latency=False):
        """payload rooms at which the verdict or the form can change"""
        n = len(self.data)
        sfx = FLUSH_RESERVE if self.flush else 0
        rooms = {self.need - 1, self.need, self.need + 1, self.stored_need - 1, self.stored_need + 1}
        if latency and self.need_lat is not None:
            rooms |= {self.need_lat - 1, self.need_lat}
        if 1 <= self.level < WG_LEVEL and n > SEG_LIMIT:
            w = seg_worst(n, SEG_BYTES, self.flush)
            # (HD_SEG_LIMIT itself: the largest room a throughput launch codes without segments)
            rooms |= {w - 1, w + 1, SEG_LIMIT, SEG_LIMIT + 1}
        if latency:
            # the per-call codecs' route thresholds (hd_api.hip deflate_one: need_lat, need_st = stored + sfx + 8)
            need_st = stored_size(n) + sfx + 8
            rooms |= {need_st - 1, need_st}
        return sorted(r for r in rooms if r >= 0)


def bgzf_clamp_rooms():
    """total rooms (stride / cap) around the BGZF clamp: 65536 itself, just below it and far above it"""
    return [BGZF_MAX - 1, BGZF_MAX, BGZF_MAX + 16, 2 * BGZF_MAX + 48]


def frame_member(frame, payload, data, crc=None):
    """the framed member of a payload, as the oracle frames it (test_encode_zlib_and_gzip_frames)"""
    o = hdtest.oracle()
    p = hdtest.as_u8(payload)
    crc = hdtest.oracle_crc32(data) if crc is None else crc
    buf = np.zeros(len(payload) + 64, dtype=np.uint8)
    ptr = buf.ctypes.data_as(hdtest.ctypes.c_void_p)
    pp = p.ctypes.data_as(hdtest.ctypes.c_void_p)
    if frame in (RAW, RAW_FLUSH):
        return bytes(payload)
    if frame == BGZF:
        n = o.hdo_bgzf_frame(ptr, len(buf), pp, len(p), crc, len(data))
    elif frame == MIGZ:
        n = o.hdo_migz_frame(ptr, len(buf), pp, len(p), crc, len(data))
    elif frame == ZLIB:
        d = hdtest.as_u8(data)
        n = o.hdo_zlib_frame(ptr, len(buf), pp, len(p), o.hdo_adler32(1, d.ctypes.data_as(hdtest.ctypes.c_void_p), len(d)))
    else:
        n = o.hdo_gzip_frame(ptr, len(buf), pp, len(p), 0, crc, len(data))
    return bytes(buf[:n])
