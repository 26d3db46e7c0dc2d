"""The model of hipdeflate_index_members_any_dev (tests/member_any_model.py) held to what it restates: the member index's
model on every file that states its lengths, the loop over zlib.decompressobj(31) on files of plain members, gzip.decompress
for the bytes, framed_model's header rules -- and the classification of every cut and corruption that
tests/test_gpu_member_any.py runs on the device (tests/member_any_cases.py).  No GPU."""
import ctypes
import gzip
import os
import re
import struct
import zlib

import pytest

import framed_model
import hdtest
import member_any_cases as mc
import member_any_model as am
import member_index_model as mim
import test_member_index_model as tmi


def test_header_and_exports_name_the_call():
    """include/hipdeflate.h declares the two entry points and the package lists them (fails without the feature)"""
    text = open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()
    for name in ("hipdeflate_index_members_any_dev", "hip_inflate_members"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in hdtest.pkg().EXPORTS, name
    s = hdtest.pkg().MemberAnySummary()
    assert ctypes.sizeof(s) == 48 and type(s).status.offset == 40


def status0_files_of_the_member_index_model():
    """the status-0 files tests/test_member_index_model.py builds: every kind with every optional field, the mixed file, BGZF"""
    for kind in tmi.KINDS:
        for k in range(0, 24, 5):
            chunk = mc.text(100 + 517 * k, seed=k)
            yield mim.gz_member(kind, tmi.raw_deflate(chunk), zlib.crc32(chunk), len(chunk), fname=b"n%d" % k if k & 1 else b"",
                                fcomment=b"c" * (k % 7) if k & 2 else b"", fhcrc=bool(k & 4))
    blob = b""
    for k in range(40):
        chunk = mc.text(300 + 211 * k, seed=k)
        blob += mim.gz_member(tmi.KINDS[k % 5], tmi.raw_deflate(chunk), zlib.crc32(chunk), len(chunk), fname=b"chunk%03d" % k if k % 2 else b"")
    yield blob
    for nbytes in (0, 1, 0xff00, 5 * 0xff00 + 77):
        for level in (0, 6):
            yield tmi.zlib_bgzf(mc.text(nbytes, seed=nbytes % 97), level)
    yield b""


def test_equals_the_member_index_model_on_its_status0_files():
    n = 0
    for blob in status0_files_of_the_member_index_model():
        rows, count, out_bytes, end, status = mim.summary(blob, 1 << 20)
        assert status == mim.OK
        got_rows, s = am.summary(blob, 1 << 20)
        assert got_rows == rows and (s["nmembers"], s["out_bytes"], s["end_offset"], s["status"]) == (count, out_bytes, end, 0)
        assert s["nsized"] == 0 and s["ncandidates"] >= count
        if count > 1:
            assert am.summary(blob, count - 1)[1]["status"] == am.TOO_SMALL == mim.summary(blob, count - 1)[4]
        n += 1
    assert n > 20


@pytest.mark.parametrize("build", [lambda: mc.counts(65), lambda: mc.counts(257), mc.empty_members, mc.every_alignment, lambda: mc.header("all_four"),
                                   lambda: mc.header("fname_5000"), lambda: mc.ending_bits("static"), lambda: mc.ending_bits("dynamic"),
                                   lambda: mc.ending_bits("stored"), lambda: mc.straddle(65536, 3), lambda: mc.decoy(2), mc.decoy_joins_chain])
def test_plain_members_like_the_zlib_loop_and_gzip(build):
    c = build()
    rows, s = c.check_model()
    data, cuts = mc.gunzip_all(c.blob)
    assert s["status"] == 0 and s["end_offset"] == len(c.blob)
    assert [r[0] + r[1] for r in rows] == cuts[1:] and gzip.decompress(c.blob) == data
    out = 0
    for (in_off, in_len, size, out_off, crc), start, end in zip(rows, cuts, cuts[1:]):
        m = c.blob[start:end]
        assert in_off - start == framed_model.open_member(m, framed_model.GZIP)              # the header rules of the framed call
        chunk = zlib.decompress(c.blob[in_off:in_off + in_len - 8], -15)
        assert (size, out_off, crc) == (len(chunk), out, zlib.crc32(chunk)) and data[out:out + size] == chunk
        assert framed_model.size(m, framed_model.GZIP) == (framed_model.OK, size, len(m))
        out += size


def test_every_case_answers_what_it_states():
    """the classification of everything the device test runs: counts, headers, decoys, mixed kinds, cuts, corruptions,
    the bound, the resumed walks"""
    cases = [mc.counts(n) for n in mc.COUNTS if n <= 257] + [mc.header(h) for h in mc.HEADERS] + [mc.decoy(1), mc.decoy_magics(), mc.mixed(),
             mc.pure_bgzf()] + [c for _, c in mc.cuts()] + [mc.corrupt(k) for k in mc.CORRUPT] + [mc.bounded(k) for k in mc.BOUNDED] + \
            [c for _, c in mc.resumes()] + [mc.straddle(1024, k) for k in mc.STRADDLES]
    for c in cases:
        c.check_model()
    assert len(cases) > 90


def test_statuses_three_and_four_and_the_sizing_call():
    c = mc.counts(65)
    rows, s = c.model(cap=64)
    assert len(rows) == 64 and (s["nmembers"], s["status"], s["end_offset"]) == (65, am.TOO_SMALL, len(c.blob))
    assert s["out_bytes"] == sum(r[2] for r in rows)
    rows, s = c.model(cap=0)
    assert rows == [] and (s["nmembers"], s["out_bytes"], s["status"]) == (65, 0, am.TOO_SMALL)
    c = mc.bounded("one_longer")
    rows, s = c.model()
    assert s["status"] == am.TOO_LONG and len(rows) == 1 and s["end_offset"] == rows[0][0] + rows[0][1]
    assert am.summary(b"", 4)[1] == {"nmembers": 0, "out_bytes": 0, "end_offset": 0, "ncandidates": 0, "nsized": 0, "status": 0}


def test_a_known_kind_with_a_bad_length_does_not_fall_through():
    chunk = b"a stated length that is wrong " * 4
    good = mc.coded("BC", chunk)
    bad = good[:16] + struct.pack("<H", 20) + good[18:]                                      # BSIZE + 1 below header + trailer
    first = mc.small(0, seed=1)
    assert am.walk(first + bad)[1:] == (am.BAD, len(first))
    assert gzip.decompress(bad) == chunk                                                     # rule B would have taken it
    unknown = good[:12] + b"BD" + good[14:]                                                  # no known kind: sized by decoding
    rows, status, end = am.walk(first + unknown)
    assert status == am.OK and len(rows) == 2 and rows[1][2] == len(chunk)
