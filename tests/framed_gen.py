"""Members for the framed inflate and the size pass: raw DEFLATE streams, RFC 1950 and RFC 1952 members, valid and not.

Every stream of tests/deflate_gen.py (corpus() and lat_corpus(), valid and fault cases) in each of the three frames, and
streams made by zlib under every shape of header and trailer the reference's wrappers tell apart (gzip_decompress.c:30-133,
zlib_decompress.c:31-91).  Used by tests/test_framed_model.py (the model against the reference) and
tests/test_gpu_framed_inflate.py (the device against the model).
"""
import struct
import zlib

import numpy as np

import deflate_gen
import hdtest
from framed_model import FCOMMENT, FEXTRA, FHCRC, FNAME, GZIP, RAW, ZLIB

NAME_LENS = [0, 1, 63, 64, 65, 300]
XLENS = [0, 1, 65535]


class Member:
    """one member: `plain` is what it decodes to where it is valid by construction, None where the model must say"""
    __slots__ = ("name", "frame", "data", "plain", "zlib")

    def __init__(self, name, frame, data, plain=None, zlib_ok=True):
        self.name, self.frame, self.data, self.plain = name, frame, bytes(data), plain
        self.zlib = zlib_ok              # False: a form libdeflate takes and zlib does not (deflate_gen's libdeflate_only)


def _text(k, n):
    """n bytes without a NUL, different for every k"""
    return bytes(33 + (i * 7 + k) % 90 for i in range(n))


def gzip_header(flg=0, xlen=0, name=0, comment=0, nul=True, id1=0x1f, id2=0x8b, cm=8, k=0):
    """ten bytes and the optional fields FLG asks for: an extra field of xlen bytes, a name and a comment of that many bytes
    before their NUL (nul=False: no NUL), the header's CRC-16 (zlib verifies it, the reference skips it)"""
    h = bytes([id1, id2, cm, flg]) + struct.pack("<IBB", 0x5eed0000 + k, 2, 3)
    if flg & FEXTRA:
        h += struct.pack("<H", xlen) + _text(k, xlen)
    if flg & FNAME:
        h += _text(k + 1, name) + (b"\0" if nul else b"")
    if flg & FCOMMENT:
        h += _text(k + 2, comment) + (b"\0" if nul else b"")
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def gzip_member(stream, plain, **kw):
    return gzip_header(**kw) + bytes(stream) + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def zlib_header(cinfo=7, flevel=2, fdict=0, cm=8, fcheck_off=0):
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (fdict << 5)
    flg += (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, (flg + fcheck_off) & 0xff])


def zlib_member(stream, plain, **kw):
    return zlib_header(**kw) + bytes(stream) + struct.pack(">I", zlib.adler32(plain))


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(bytes(data)) + c.flush()


def _unique_cases():
    seen, out = set(), []
    for c in deflate_gen.cached_corpus() + deflate_gen.cached_lat_corpus():
        if c.stream not in seen:             # (the cap - 1 twin of a valid case is the same stream)
            seen.add(c.stream)
            out.append(c)
    return out


def corpus_members():
    """every stream of deflate_gen once per frame; the gzip headers cycle through the sixteen flag combinations, the name
    lengths and small extra fields, so that the payloads start at every offset mod 4"""
    out = []
    for k, c in enumerate(_unique_cases()):
        good = c.code == deflate_gen.OK
        plain = c.expected if good else b""
        out.append(Member("raw/" + c.name, RAW, c.stream, c.expected if good else None, c.zlib))
        out.append(Member("zlib/" + c.name, ZLIB, zlib_member(c.stream, plain, cinfo=k % 8), c.expected if good else None, c.zlib))
        flg = 2 * (k % 16)                   # FHCRC, FEXTRA, FNAME, FCOMMENT: bits 1..4
        out.append(Member("gzip/" + c.name, GZIP,
                          gzip_member(c.stream, plain, flg=flg | (k >> 4 & 1), xlen=(k * 5) % 23, name=NAME_LENS[k % 6],
                                      comment=NAME_LENS[(k // 6) % 6], k=k), c.expected if good else None, c.zlib))
    return out


def _samples():
    s = hdtest.synth()
    return [("empty", b""), ("one", b"a"), ("text5000", bytes(s.text_like(5000, seed=5))),
            ("fastq70000", bytes(s.fastq_like(70000, seed=6))), ("random1000", bytes(s.random_bytes(1000, seed=7))),
            ("zeros100k", bytes(100000))]


def header_members():
    out = []
    samples = [(nm, d, raw_deflate(d, 1 + i % 9)) for i, (nm, d) in enumerate(_samples())]
    for nm, d, z in samples:
        out.append(Member("raw/zlib_" + nm, RAW, z, d))
        out.append(Member("zlib/zlib_" + nm, ZLIB, zlib.compress(d), d))
        out.append(Member("gzip/zlib_" + nm, GZIP, gzip_member(z, d), d))
    nm, d, z = samples[2]
    # the sixteen FEXTRA / FNAME / FCOMMENT / FHCRC combinations with every extra length and every name length
    seen = set()
    for combo in range(16):
        for xlen in XLENS:
            for ln in NAME_LENS:
                m = gzip_member(z, d, flg=2 * combo, xlen=xlen, name=ln, comment=NAME_LENS[(NAME_LENS.index(ln) + 1) % 6], k=combo)
                if m not in seen:
                    seen.add(m)
                    out.append(Member("gzip/combo%d_x%d_n%d" % (combo, xlen, ln), GZIP, m, d))
    out.append(Member("gzip/name70000", GZIP, gzip_member(z, d, flg=FNAME, name=70000), d))
    out.append(Member("gzip/comment70000_hcrc", GZIP, gzip_member(z, d, flg=FCOMMENT | FHCRC, comment=70000), d))
    for ln in range(4):                      # the payload at every offset mod 4
        out.append(Member("gzip/payload_mod4_%d" % ln, GZIP, gzip_member(z, d, flg=FNAME, name=ln), d))
    # what the header rules refuse
    for bit in (0x20, 0x40, 0x80):
        out.append(Member("gzip/reserved_%02x" % bit, GZIP, gzip_member(z, d, flg=bit)))
    out.append(Member("gzip/bad_id1", GZIP, gzip_member(z, d, id1=0x1e)))
    out.append(Member("gzip/bad_id2", GZIP, gzip_member(z, d, id2=0x8a)))
    out.append(Member("gzip/bad_cm", GZIP, gzip_member(z, d, cm=7)))
    out.append(Member("gzip/ftext", GZIP, gzip_member(z, d, flg=1), d))
    out.append(Member("gzip/name_no_nul_payload_follows", GZIP, gzip_member(z, d, flg=FNAME, name=20, nul=False)))
    out.append(Member("gzip/name_no_nul_at_all", GZIP, gzip_header(flg=FNAME, name=40, nul=False) + _text(9, 30)))
    out.append(Member("gzip/comment_no_nul_at_all", GZIP, gzip_header(flg=FNAME | FCOMMENT, name=3, comment=500, nul=False) + _text(9, 30)))
    tiny_g, tiny_z = gzip_member(b"\x03\x00", b""), zlib_member(b"\x03\x00", b"")
    out.append(Member("gzip/tiny20", GZIP, tiny_g, b""))
    out.append(Member("gzip/tiny18", GZIP, tiny_g[:18]))
    out.append(Member("gzip/tiny17", GZIP, tiny_g[:17]))
    out.append(Member("gzip/empty", GZIP, b""))
    out.append(Member("zlib/tiny8", ZLIB, tiny_z, b""))
    out.append(Member("zlib/tiny6", ZLIB, tiny_z[:6]))
    out.append(Member("zlib/tiny5", ZLIB, tiny_z[:5]))
    out.append(Member("zlib/empty", ZLIB, b""))
    out.append(Member("raw/empty", RAW, b""))
    # a header that ends 7 and 8 bytes before the end, by each optional field
    for left in (7, 8, 9, 10):
        out.append(Member("gzip/extra_leaves_%d" % left, GZIP, gzip_header(flg=FEXTRA, xlen=30) + _text(left, left)))
        out.append(Member("gzip/name_leaves_%d" % left, GZIP, gzip_header(flg=FNAME, name=30) + _text(left, left)))
        out.append(Member("gzip/comment_leaves_%d" % left, GZIP, gzip_header(flg=FCOMMENT, comment=30) + _text(left, left)))
        out.append(Member("gzip/hcrc_leaves_%d" % left, GZIP, gzip_header(flg=FHCRC) + _text(left, left)))
        out.append(Member("gzip/all_leave_%d" % left, GZIP,
                          gzip_header(flg=FEXTRA | FNAME | FCOMMENT | FHCRC, xlen=5, name=64, comment=65) + _text(left, left)))
    h = bytearray(gzip_header())
    h[3] = FEXTRA
    out.append(Member("gzip/xlen_past_end", GZIP, bytes(h) + b"\xff\xff" + z + bytes(8)))
    # zlib headers
    for cinfo in range(9):
        out.append(Member("zlib/cinfo%d" % cinfo, ZLIB, zlib_member(z, d, cinfo=cinfo), d if cinfo <= 7 else None))
    out.append(Member("zlib/fdict", ZLIB, zlib_member(z, d, fdict=1)))
    out.append(Member("zlib/fcheck_plus1", ZLIB, zlib_member(z, d, fcheck_off=1)))
    out.append(Member("zlib/fcheck_minus1", ZLIB, zlib_member(z, d, fcheck_off=-1)))
    out.append(Member("zlib/cm7", ZLIB, zlib_member(z, d, cm=7)))
    # trailers: one bit flipped, in every field
    g, zl = gzip_member(z, d, flg=FNAME, name=5), zlib_member(z, d)
    for bit in range(64):
        m = bytearray(g)
        m[len(m) - 8 + bit // 8] ^= 1 << (bit % 8)
        out.append(Member("gzip/%s_bit%d" % ("crc" if bit < 32 else "isize", bit % 32), GZIP, m))
    for bit in range(32):
        m = bytearray(zl)
        m[len(m) - 4 + bit // 8] ^= 1 << (bit % 8)
        out.append(Member("zlib/adler_bit%d" % bit, ZLIB, m))
    out.append(Member("gzip/trailer_cut1", GZIP, g[:-1]))
    out.append(Member("zlib/trailer_cut1", ZLIB, zl[:-1]))
    out.append(Member("raw/stream_cut1", RAW, z[:-1]))
    for extra in (1, 7, 100):
        junk = bytes((i * 37 + extra) & 0xff for i in range(extra))
        out.append(Member("gzip/garbage%d" % extra, GZIP, g + junk, d))
        out.append(Member("zlib/garbage%d" % extra, ZLIB, zl + junk, d))
        out.append(Member("raw/garbage%d" % extra, RAW, z + junk, d))
    # two members back to back, handed over as one: the first is decoded, in_used says where the second starts
    for frame, (a, b) in pairs().items():
        out.append(Member("%s/pair" % {RAW: "raw", ZLIB: "zlib", GZIP: "gzip"}[frame], frame, a[0] + b[0], a[1]))
    return out


def pairs():
    """frame -> ((first member, its contents), (second member, its contents))"""
    s = hdtest.synth()
    d1, d2 = bytes(s.text_like(3000, seed=21)), bytes(s.fastq_like(4097, seed=22))
    z1, z2 = raw_deflate(d1, 6), raw_deflate(d2, 9)
    return {RAW: ((z1, d1), (z2, d2)), ZLIB: ((zlib_member(z1, d1), d1), (zlib_member(z2, d2), d2)),
            GZIP: ((gzip_member(z1, d1, flg=FNAME | FHCRC, name=6), d1), (gzip_member(z2, d2, flg=FEXTRA, xlen=3), d2))}


_cached = None


def members():
    """every member, once per process"""
    global _cached
    if _cached is None:
        _cached = corpus_members() + header_members()
    return _cached


def pack(ms, seed=1):
    """the members in one buffer, member i at an offset that is i mod 16 (mod 16), other bytes between and behind them
    -> (blob uint8 array, in_off uint64 array, in_len uint32 array)"""
    rng = np.random.default_rng(seed)
    parts, offs, pos = [], [], 0
    for i, m in enumerate(ms):
        gap = (i % 16 - pos) % 16
        parts.append(rng.integers(1, 256, gap, dtype=np.uint8).tobytes())
        pos += gap
        offs.append(pos)
        parts.append(m.data)
        pos += len(m.data)
    parts.append(rng.integers(1, 256, 64, dtype=np.uint8).tobytes())
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return blob, np.array(offs, dtype=np.uint64), np.array([len(m.data) for m in ms], dtype=np.uint32)
