"""The model of the device member index (tests/member_index_model.py) held to what it restates: the oracle's
_read_gz_header on hand-framed members of the five kinds, bgzf_scan on BGZF files, and the verdicts of hd7bgzf -d on the
corrupt files of tests/test_host_cli.py::test_decode_prescan_rejects_corrupt_headers_like_the_reference.  No GPU."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import hdtest
import member_index_model as mm

KINDS = ["BC", "MZ", "IG1", "IG2", "MG"]


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def zlib_bgzf(data, level=6, block=0xff00):
    """a BGZF file as bgzip writes it, its blocks coded by zlib"""
    pkg = hdtest.pkg()
    out = []
    for o in range(0, len(data), block):
        chunk = data[o:o + block]
        out.append(mm.gz_member("BC", raw_deflate(chunk, level), zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + pkg.BGZF_EOF


def test_header_and_exports_name_the_device_index():
    """include/hipdeflate.h declares the two entry points and the package lists them (fails without the feature)"""
    text = open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()
    for name in ("hipdeflate_index_members_dev", "hipdeflate_verify_members_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in hdtest.pkg().EXPORTS, name
    assert "hipdeflate_member_summary" in text
    s = hdtest.pkg().MemberSummary()
    assert ctypes.sizeof(s) == 32 and type(s).status.offset == 24


@pytest.mark.parametrize("kind", KINDS)
def test_model_agrees_with_the_oracles_read_gz_header(kind):
    o = hdtest.oracle()
    rng = np.random.default_rng(KINDS.index(kind))
    for k in range(24):
        chunk = bytes(hdtest.synth().fastq_like(100 + 517 * k, seed=k))
        payload = raw_deflate(chunk)
        m = mm.gz_member(kind, payload, zlib.crc32(chunk), len(chunk), fname=b"n%d" % k if k & 1 else b"",
                         fcomment=b"c" * (k % 7) if k & 2 else b"", fhcrc=bool(k & 4))
        eo, el, bl = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        n = o.hdo_read_gz_header(m, len(m), ctypes.byref(eo), ctypes.byref(el), ctypes.byref(bl))
        pad = bytes(rng.integers(0, 256, k, dtype=np.uint8))
        cls, hdr, total = mm.member_len(m + pad, 0)
        assert (cls, hdr, total) == (mm.OK, n, bl.value) and total == len(m) and hdr == len(m) - len(payload) - 8, (kind, k)
        rows, status, end = mm.walk(m)
        assert status == mm.OK and end == len(m) and rows == [(hdr, total - hdr, len(chunk), 0, zlib.crc32(chunk))]


def test_model_walks_mixed_kinds_like_the_oracle():
    o = hdtest.oracle()
    blob, want, offs = b"", [], 0
    for k in range(40):
        chunk = bytes(hdtest.synth().text_like(300 + 211 * k, seed=k))
        payload = raw_deflate(chunk)
        m = mm.gz_member(KINDS[k % 5], payload, zlib.crc32(chunk), len(chunk), fname=b"chunk%03d" % k if k % 2 else b"")
        eo, el, bl = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        n = o.hdo_read_gz_header(m, min(len(m), 128), ctypes.byref(eo), ctypes.byref(el), ctypes.byref(bl))
        assert n > 0 and bl.value == len(m)
        want.append((len(blob) + n, len(m) - n, len(chunk), offs, zlib.crc32(chunk)))
        offs += len(chunk)
        blob += m
    assert mm.walk(blob) == (want, mm.OK, len(blob))
    assert mm.summary(blob, 39) == (want[:39], 40, sum(r[2] for r in want[:39]), len(blob), mm.TOO_SMALL)
    assert mm.summary(blob, 40)[1:] == (40, offs, len(blob), mm.OK)


@pytest.mark.parametrize("nbytes", [0, 1, 0xff00 - 1, 0xff00, 0xff00 + 1, 5 * 0xff00 + 77])
def test_model_agrees_with_bgzf_scan(nbytes):
    pkg = hdtest.pkg()
    for level in (0, 6):
        blob = zlib_bgzf(bytes(hdtest.synth().fastq_like(nbytes, seed=nbytes % 97)) if nbytes else b"", level)
        rows, status, end = mm.walk(blob)
        assert status == mm.OK and end == len(blob)
        assert [r[:3] for r in rows] == pkg.bgzf_scan(blob)
        assert rows[-1][:3] == (len(blob) - 10, 10, 0)                    # the EOF member
        assert [r[3] for r in rows] == [min(i * 0xff00, nbytes) for i in range(len(rows))]


@pytest.mark.parametrize("bad", ["bsize_small", "bsize_tiny", "no_extra", "cut"])
def test_model_verdicts_on_the_corrupt_files_of_the_host_cli(bad):
    """hd7bgzf -d answers "not BGZF or corrupted" for the first three and fails on the fourth; bgzf_scan raises on all"""
    pkg = hdtest.pkg()
    good = zlib_bgzf(bytes(hdtest.synth().fastq_like(3 * 0xff00, seed=4)), 1)
    full = mm.walk(good)[0]
    blob = bytearray(good)
    if bad == "bsize_small":
        blob[16:18] = struct.pack("<H", 20)
    elif bad == "bsize_tiny":
        blob[16:18] = struct.pack("<H", 1)
    elif bad == "no_extra":
        blob[3] = 0
    else:
        blob = blob[: len(blob) // 2]
    with pytest.raises(pkg.HipDeflateError):
        pkg.bgzf_scan(bytes(blob))
    rows, status, end = mm.walk(bytes(blob))
    if bad == "cut":
        keep = [r for r in full if r[0] + r[1] <= len(blob)]
        assert 0 < len(keep) < len(full) and rows == keep
        assert (status, end) == (mm.CUT, keep[-1][0] + keep[-1][1])
    else:
        assert (rows, status, end) == ([], mm.BAD, 0)


def test_model_tells_cut_from_bad_at_every_byte():
    chunk = b"hello, member index " * 20
    m = mm.gz_member("BC", raw_deflate(chunk), zlib.crc32(chunk), len(chunk), fname=b"name", fhcrc=True)
    first = mm.gz_member("MZ", raw_deflate(chunk), zlib.crc32(chunk), len(chunk))
    for cut in range(1, len(m)):
        rows, status, end = mm.walk(first + m[:cut])
        assert len(rows) == 1 and (status, end) == (mm.CUT, len(first)), cut
    for at, val in ((0, 0x1e), (1, 0), (2, 7), (3, 0x24), (3, 0x08), (12, ord("X")), (16, 5)):
        g = bytearray(m)
        g[at] = val
        if at == 16:
            g[17] = 0                        # BSIZE + 1 = 6: below header + trailer
        assert mm.walk(first + bytes(g))[1:] == (mm.BAD, len(first)), at
    assert mm.walk(first + b"\x1f")[1:] == (mm.CUT, len(first))
    assert mm.walk(first + b"\x1f\x8b\x09")[1:] == (mm.BAD, len(first))
    assert mm.walk(b"") == ([], mm.OK, 0)
