"""The device member index -- hipdeflate_index_members_dev, hipdeflate_verify_members_dev, DeviceInflate -- against the
plain Python walk of tests/member_index_model.py.  Bit-exact, no tolerances: the summary, every table entry, and a
sentinel in every entry the call must not touch.  No case provokes a fault: each corrupt blob is a case the contract of
include/hipdeflate.h defines, and each runs once.

Most cases frame arbitrary bytes as members (the index reads headers and trailers, never payloads); accidental magics
inside them are welcome.  Cuts are made by passing a smaller nbytes over the WHOLE blob in device memory: a read behind
nbytes would find the rest of the member there and answer "ok".

Where the cases land (hd_index.hpp):
  * member counts 63 / 64 / 65 and 2047 / 2048 / 2049: a wavefront and a tile (SCAN_TILE) of the rank scan and of the
    out_off scan, and the rounds of k_index_jump on either side of a power of two; 70,000 tiny members: more than
    65,536 candidates, dozens in one thread's 1 KiB bitmap word of k_index_write, several workgroups of k_index_links.
  * FNAME of 0..70 bytes in the first member moves every later header through all offsets mod 16 and mod 64: the magic
    straddles a lane's 16 bytes (the extra dword of index_load20); the boundary sweep puts it across 1 KiB (a wavefront's
    load), 64 KiB (a wavefront's share of a tile) and 256 KiB (a workgroup's tile); every nbytes mod 16 runs the byte-wise
    tail of index_load20.
  * decoys: candidates whose links form chains of their own, end at nbytes, point past it, into a true header, or at a
    true member -- k_index_jump marks from candidate 0 only, so a path that JOINS the true chain marks nothing before
    the joint.
  * ISIZE 0xffffffff: the 64-bit out_off scan past 2^32 (wave_incl_scan64)."""
import importlib
import os
import struct
import zlib

import numpy as np
import pytest

import hdtest
import member_index_model as mm

pytestmark = pytest.mark.gpu

S64 = 0x5a5a5a5a5a5a5a5a
S32 = 0x5a5a5a5a
GUARD = 8                                       # table entries behind max_members that must stay untouched too
KINDS = ["BC", "MZ", "IG1", "IG2", "MG"]
HDR = {"BC": 18, "MZ": 20, "IG1": 32, "IG2": 20, "MG": 16}


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


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def framed(kind, nbytes_payload, rng, isize=None, **kw):
    """a member around arbitrary payload bytes: for the index alone"""
    payload = bytes(rng.integers(0, 256, nbytes_payload, dtype=np.uint8))
    return mm.gz_member(kind, payload, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 70000)) if isize is None else isize, **kw)


def coded(kind, chunk, level=6, **kw):
    """a member that inflates to chunk"""
    return mm.gz_member(kind, raw_deflate(chunk, level), zlib.crc32(chunk), len(chunk), **kw)


def zlib_bgzf(pkg, data, level=6):
    return b"".join(coded("BC", data[o:o + 0xff00], level) for o in range(0, len(data), 0xff00)) + pkg.BGZF_EOF


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def sentinel_tables(dev, torch, cap):
    d = dev.DeviceInflate(cap + GUARD)
    d.max_members = cap
    for t in (d.in_off, d.out_off):
        t.fill_(S64)
    for t in (d.in_len, d.out_size, d.crc_want):
        t.fill_(S32)
    return d


def check_index(dev, torch, blob, cap=None, nbytes=None, slack=3):
    """index blob[:nbytes] into a table of `cap` entries (default: the members the model finds + slack) and hold the
    summary, the rows and the sentinels to the model -> (summary, DeviceInflate, device blob)"""
    nbytes = len(blob) if nbytes is None else nbytes
    rows_all = mm.walk(blob, nbytes)[0]
    cap = len(rows_all) + slack if cap is None else cap
    rows, n, out_bytes, end, status = mm.summary(blob, cap, nbytes)
    d = sentinel_tables(dev, torch, cap)
    t = to_dev(torch, blob)
    s = d.index(t[:nbytes])
    assert (s.nmembers, s.out_bytes, s.end_offset, s.status) == (n, out_bytes, end, status), \
        ((s.nmembers, s.out_bytes, s.end_offset, s.status), (n, out_bytes, end, status))
    k = len(rows)
    want = np.array(rows, dtype=np.uint64).reshape(k, 5)
    got = [x.cpu().numpy() for x in (d.in_off, d.in_len, d.out_size, d.out_off, d.crc_want)]
    for col, (g, wide) in enumerate(zip(got, (True, False, False, True, False))):
        g = g.view(np.uint64 if wide else np.uint32)
        assert np.array_equal(g[:k].astype(np.uint64), want[:, col]), ("column", col)
        assert np.all(g[k:] == (S64 if wide else S32)), ("sentinel of column", col)
    return s, d, t


def tiny_file(pkg, n, seed, kinds=("BC",)):
    """n members: n - 1 tiny coded ones (1..40 input bytes) and the EOF member"""
    rng = np.random.default_rng(seed)
    src = bytes(rng.integers(97, 101, 64, dtype=np.uint8))
    parts = []
    for i in range(n - 1):
        ln = 1 + (i * 7 + seed) % 40
        parts.append(coded(kinds[i % len(kinds)], src[i % 20:i % 20 + ln]))
    return b"".join(parts) + pkg.BGZF_EOF


# ---- member counts ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049])
def test_member_counts(pkg, torch, dev, n):
    blob = tiny_file(pkg, n, seed=n, kinds=KINDS)
    s, _, _ = check_index(dev, torch, blob)
    assert s.nmembers == n and s.status == 0
    check_index(dev, torch, blob, cap=n, slack=0)                  # a table of exactly n entries is enough


def test_seventy_thousand_tiny_members_and_decode(pkg, torch, dev):
    blob = tiny_file(pkg, 70001, seed=5)
    s, d, t = check_index(dev, torch, blob)
    assert s.nmembers == 70001
    out = torch.full((s.out_bytes + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    d.max_members = s.nmembers
    assert d.run(t, out).nmembers == 70001
    assert bytes(out.cpu().numpy()) == _gunzip_all(blob) + b"\x5a" * 16


def _gunzip_all(blob):
    out, rest = [], blob
    while rest:
        z = zlib.decompressobj(31)
        out.append(z.decompress(rest))
        rest = z.unused_data
    return b"".join(out)


@pytest.mark.parametrize("level", [0, 1, 6])
def test_our_own_files(pkg, torch, dev, level):
    data = bytes(hdtest.synth().fastq_like(37 * 0xff00 + 1234, seed=20 + level))
    blob = pkg.bgzf_compress_bytes(data, level)
    s, _, _ = check_index(dev, torch, blob)
    assert s.nmembers == 39 and s.out_bytes == len(data)
    assert [r[:3] for r in mm.walk(blob)[0]] == pkg.bgzf_scan(blob)


def test_migz_members_of_one_mib(pkg, torch, dev):
    data = bytes(hdtest.synth().text_like(3 * (1 << 20) + 300000, seed=7))
    offs = [0, 1 << 20, 2 << 20, 3 << 20]
    lens = [1 << 20, 1 << 20, 1 << 20, 300000]
    slot = ((1 << 20) + (1 << 17) + 4096 + 15) & ~15
    for level in (0, 6):
        members, _, st = pkg.batch_deflate(data, offs, lens, level, pkg.FRAME_MIGZ, slot=slot)
        assert not np.any(st)
        blob = b"".join(members)
        s, d, t = check_index(dev, torch, blob)
        assert s.nmembers == 4 and s.out_bytes == len(data)
        out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        d.max_members = 4
        d.run(t, out)
        assert bytes(out.cpu().numpy()) == data


# ---- alignment ----------------------------------------------------------------------------------------------------


def test_every_header_alignment_and_every_length_mod_16(pkg, torch, dev):
    rng = np.random.default_rng(16)
    starts16, starts64, len16 = set(), set(), set()
    for fn in range(71):
        parts = [framed("BC", 40, rng, fname=b"n" * fn)]
        for k in range(6):
            parts.append(framed(KINDS[(fn + k) % 5], 30 + 16 * k + (fn * 5 + k) % 13, rng, fhcrc=bool(k & 1)))
        parts.append(framed("MG", fn % 16 + 3, rng))
        blob = b"".join(parts)
        s, _, _ = check_index(dev, torch, blob)
        assert s.nmembers == 8 and s.status == 0
        o = 0
        for p in parts:
            starts16.add(o % 16)
            starts64.add(o % 64)
            o += len(p)
        len16.add(len(blob) % 16)
    assert len(starts16) == 16 and len(starts64) == 64 and len(len16) == 16


@pytest.mark.parametrize("boundary", [1024, 65536, 262144, 524288])
def test_magic_across_wavefront_and_workgroup_granules(pkg, torch, dev, boundary):
    rng = np.random.default_rng(boundary)
    for k in (0, 1, 2, 3, 4, 15, 16, 17):
        first = framed("MZ", boundary - k - 28, rng)               # the second member starts at boundary - k
        blob = first + framed("BC", 100, rng) + framed("IG2", 50, rng) + pkg.BGZF_EOF
        assert len(first) == boundary - k
        s, _, _ = check_index(dev, torch, blob)
        assert s.nmembers == 4 and s.status == 0


# ---- decoys -------------------------------------------------------------------------------------------------------


def test_bgzf_stored_inside_bgzf_two_deep(pkg, torch, dev):
    data = bytes(hdtest.synth().fastq_like(5 * 0xff00 + 99, seed=3))
    inner = pkg.bgzf_compress_bytes(data, 6)
    mid = pkg.bgzf_compress_bytes(inner, 0)
    outer = pkg.bgzf_compress_bytes(mid, 0)
    assert inner[:100] in outer                                       # the inner headers are there verbatim
    s, d, t = check_index(dev, torch, outer)
    out = torch.empty(s.out_bytes, dtype=torch.uint8, device="cuda")
    d.max_members = s.nmembers
    d.run(t, out)
    assert bytes(out.cpu().numpy()) == mid


def test_stored_payload_of_nothing_but_magics(pkg, torch, dev):
    data = b"\x1f\x8b\x08\x04" * (3 * 0xff00 // 4 + 100)
    blob = pkg.bgzf_compress_bytes(data, 0)
    s, d, t = check_index(dev, torch, blob)
    assert s.nmembers == 5 and s.out_bytes == len(data)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    d.max_members = 5
    d.run(t, out)
    assert bytes(out.cpu().numpy()) == data


def decoy_file(pkg):
    """four members of arbitrary payload + the EOF member, with decoy BC / MZ headers planted in the payloads"""
    rng = np.random.default_rng(44)
    kinds = ["BC", "MZ", "IG2", "MG"]
    raws = [bytearray(rng.integers(32, 127, 400, dtype=np.uint8).tobytes()) for _ in kinds]
    start, raw_at, o = [], [], 0
    for k, r in zip(kinds, raws):
        start.append(o)
        raw_at.append(o + HDR[k])
        o += HDR[k] + len(r) + 8
    start.append(o)                                                   # the EOF member
    nbytes = o + 28

    def plant(i, at, target, kind="BC"):
        p = raw_at[i] + at
        total = target - p
        assert 28 <= total <= 65536
        if kind == "BC":
            h = bytes.fromhex("1f8b08040000000000ff0600") + b"BC\x02\x00" + struct.pack("<H", total - 1)
        else:
            h = bytes.fromhex("1f8b08040000000000ff0800") + b"MZ\x04\x00" + struct.pack("<I", total - 28)
        raws[i][at:at + len(h)] = h
        return p
    plant(0, 10, start[1])                           # joins the true chain at member 1
    plant(0, 100, raw_at[1] + 200)                   # decoy -> the MZ decoy below -> true member 3
    plant(1, 200, start[3], "MZ")
    plant(0, 200, raw_at[1] + 20)                    # decoy -> the decoy below, whose link is bad
    plant(1, 20, start[2] + 5)                       # into the middle of a true header
    plant(1, 60, nbytes)                             # ends exactly at nbytes
    plant(2, 30, nbytes + 1000)                      # past nbytes
    plant(2, 90, start[4], "MZ")                     # at the EOF member
    plant(2, 150, nbytes + 1)
    plant(3, 40, nbytes)                             # exactly at nbytes again, from the last data member
    plant(3, 100, nbytes - 1)                        # into the EOF member's trailer
    blob = b"".join(mm.gz_member(k, bytes(r), 0x11111111 * (i + 1), 1000 + i) for i, (k, r) in enumerate(zip(kinds, raws)))
    blob += pkg.BGZF_EOF
    assert len(blob) == nbytes and [blob.find(b"\x1f\x8b\x08\x04", x) for x in start] == start
    return blob, start


def test_decoy_links_of_every_kind(pkg, torch, dev):
    blob, start = decoy_file(pkg)
    assert blob.count(b"\x1f\x8b\x08\x04") >= 5 + 11
    s, d, _ = check_index(dev, torch, blob)
    assert s.nmembers == 5 and s.status == 0
    assert [int(x) for x in d.in_off[:5].cpu()] == [start[0] + 18, start[1] + 20, start[2] + 20, start[3] + 16, start[4] + 18]
    # the same file behind a first byte that is no member: a false path that reaches the end proves nothing
    s, _, _ = check_index(dev, torch, b"\0" + blob)
    assert (s.nmembers, s.status, s.end_offset) == (0, 1, 0)


# ---- wide sums ----------------------------------------------------------------------------------------------------


def test_out_off_passes_four_gib(pkg, torch, dev):
    rng = np.random.default_rng(9)
    blob = b"".join(framed(KINDS[k % 5], 20 + k, rng, isize=0xffffffff) for k in range(70))
    s, d, _ = check_index(dev, torch, blob)
    assert s.out_bytes == 70 * 0xffffffff and int(d.out_off[69]) == 69 * 0xffffffff


# ---- verdicts -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bad", ["bsize_small", "bsize_tiny", "no_extra", "cut"])
def test_corrupt_files_of_the_host_cli(pkg, torch, dev, bad):
    data = bytes(hdtest.synth().fastq_like(3 * 0xff00, seed=4))
    blob = bytearray(pkg.bgzf_compress_bytes(data, 1))
    nbytes = len(blob)
    if bad == "bsize_small":
        blob[16:18] = struct.pack("<H", 20)
    elif bad == "bsize_tiny":
        blob[16:18] = struct.pack("<H", 1)
    elif bad == "no_extra":
        blob[3] = 0
    else:
        nbytes = len(blob) // 2
    s, _, _ = check_index(dev, torch, bytes(blob), nbytes=nbytes)
    if bad == "cut":
        assert s.status == 2 and s.nmembers >= 1 and 0 < s.end_offset < nbytes
    else:
        assert (s.status, s.nmembers, s.end_offset) == (1, 0, 0)
    with pytest.raises(pkg.HipDeflateError):
        pkg.bgzf_scan(bytes(blob[:nbytes]))


def test_last_member_cut_at_every_byte_of_header_and_trailer(pkg, torch, dev):
    rng = np.random.default_rng(2)
    for kind in KINDS:
        head = framed("BC", 100, rng) + framed("MZ", 77, rng)
        last = framed(kind, 64, rng, fname=b"name", fcomment=b"note", fhcrc=True)
        hdr = HDR[kind] + 5 + 5 + 2
        for cut in list(range(1, hdr + 1)) + list(range(len(last) - 8, len(last))):
            s, _, _ = check_index(dev, torch, head + last, nbytes=len(head) + cut)
            assert (s.status, s.nmembers, s.end_offset) == (2, 2, len(head)), (kind, cut)


def test_garbage_behind_the_eof_member(pkg, torch, dev):
    blob = tiny_file(pkg, 10, seed=1)
    for tail, status in ((b"garbage", 1), (b"\0", 1), (b"\x1f\x8b", 2), (b"\x1f\x8b\x08\x04" + bytes(8), 1),
                         (bytes.fromhex("1f8b08040000000000ffff7f"), 2), (bytes.fromhex("1f8b080c0000000000ff0000") + b"abc", 2)):
        s, _, _ = check_index(dev, torch, blob + tail)
        assert (s.status, s.nmembers, s.end_offset) == (status, 10, len(blob)), tail


def test_named_candidates_of_no_known_kind(pkg, torch, dev):
    """k_index_links refuses an extra field of no known kind BEFORE it scans a name (member_parse<false>), k_index_verdict
    keeps member_len()'s order (member_parse<true>): the verdicts are the model's either way"""
    data = b"\x1f\x8b\x08\x0c" * (3 * 0xff00 // 4 + 100)              # FNAME set, no zero byte anywhere, XLEN = 0x8b1f
    blob = pkg.bgzf_compress_bytes(data, 0)
    s, d, t = check_index(dev, torch, blob)
    assert s.nmembers == 5 and s.out_bytes == len(data)
    assert bytes(dev.inflate_container(t).cpu().numpy()) == data
    small = tiny_file(pkg, 10, seed=3)
    unknown = bytes.fromhex("1f8b081c0000000000ff0400") + b"XXXX"      # FNAME + FCOMMENT behind an extra field nobody knows
    for tail, status in ((unknown + b"name without end", 2), (unknown + b"name\0note without end", 2),
                         (unknown + b"name\0note\0" + bytes(20), 1)):
        s, _, _ = check_index(dev, torch, small + tail)
        assert (s.status, s.nmembers, s.end_offset) == (status, 10, len(small)), tail
    # named members of every kind in a row: each scan starts behind the zero byte of its own XLEN
    rng = np.random.default_rng(12)
    blob = b"".join(framed(KINDS[k % 5], 30 + k, rng, fname=b"n" * (k % 7 + 1), fcomment=b"c" * (k % 3)) for k in range(40))
    s, _, _ = check_index(dev, torch, blob)
    assert (s.status, s.nmembers) == (0, 40)


def test_a_file_of_no_bytes_through_run(pkg, torch, dev):
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    d = dev.DeviceInflate(4)
    s = d.run(empty, torch.empty(0, dtype=torch.uint8, device="cuda"))
    assert (s.status, s.nmembers, s.out_bytes, s.end_offset) == (0, 0, 0, 0)
    assert dev.inflate_container(empty).numel() == 0


def test_table_one_too_small_and_empty_input_and_a_first_byte_that_is_no_member(pkg, torch, dev):
    blob = tiny_file(pkg, 100, seed=8)
    s, _, _ = check_index(dev, torch, blob, cap=99)
    assert (s.status, s.nmembers, s.end_offset) == (3, 100, len(blob))
    s, _, _ = check_index(dev, torch, blob, cap=0)
    assert (s.status, s.nmembers, s.out_bytes) == (3, 100, 0)
    s, _, _ = check_index(dev, torch, blob, nbytes=0)
    assert (s.status, s.nmembers, s.out_bytes, s.end_offset) == (0, 0, 0, 0)
    s, _, _ = check_index(dev, torch, b"\x1e" + blob[1:])
    assert (s.status, s.nmembers, s.end_offset) == (1, 0, 0)
    s, _, _ = check_index(dev, torch, b"BAM\x01" * 1000)
    assert (s.status, s.nmembers, s.end_offset) == (1, 0, 0)


# ---- end to end ---------------------------------------------------------------------------------------------------


def container_files(pkg):
    data = bytes(hdtest.synth().fastq_like(21 * 0xff00 + 4321, seed=31))
    files = [("own level 1", pkg.bgzf_compress_bytes(data, 1), data), ("own level 6", pkg.bgzf_compress_bytes(data, 6), data),
             ("zlib 6", zlib_bgzf(pkg, data), data)]
    mixed = [bytes(hdtest.synth().text_like(2000 + 900 * k, seed=k)) for k in range(25)]
    files.append(("five kinds", b"".join(coded(KINDS[k % 5], c, fname=b"f%d" % k if k % 2 else b"", fcomment=b"c" if k % 3 == 0 else b"",
                                               fhcrc=k % 4 == 0) for k, c in enumerate(mixed)), b"".join(mixed)))
    ref = hdtest.ref()
    if ref is not None:                                               # the reference's own writer (bgzf_compress.c), where it was built
        members = []
        for o in range(0, len(data), 0xff00):
            r, m = hdtest.call_enc(ref.bgzf_compress, data[o:o + 0xff00], 6, cap=65536)
            assert r == 0
            members.append(m)
        files.append(("reference", b"".join(members) + pkg.BGZF_EOF, data))
    return files


def test_device_inflate_run_end_to_end(pkg, torch, dev):
    stalls = pkg.lib().hipdeflate_stall_count()
    for name, blob, data in container_files(pkg):
        s, d, t = check_index(dev, torch, blob)
        assert s.status == 0 and s.out_bytes == len(data), name
        d.max_members = s.nmembers
        out = torch.full((len(data) + 64,), 0x5a, dtype=torch.uint8, device="cuda")
        s2 = d.run(t, out)
        assert (s2.nmembers, s2.out_bytes) == (s.nmembers, s.out_bytes), name
        assert d.verify(s.nmembers) == s.nmembers, name
        assert bytes(out.cpu().numpy()) == data + b"\x5a" * 64, name
        assert bytes(dev.inflate_container(t).cpu().numpy()) == data, name
        if name != "five kinds":
            assert pkg.bgzf_decompress_bytes(blob) == data, name
    assert pkg.lib().hipdeflate_stall_count() == stalls == 0


@pytest.mark.parametrize("what", ["crc", "isize"])
def test_verify_names_the_member_whose_trailer_disagrees(pkg, torch, dev, what):
    data = bytes(hdtest.synth().fastq_like(300 * 0xff00, seed=6))
    good = pkg.bgzf_compress_bytes(data, 1)
    rows = mm.walk(good)[0]
    for k in (0, 63, 257, 299):
        blob = bytearray(good)
        end = rows[k][0] + rows[k][1]
        blob[end - 8 if what == "crc" else end - 4] ^= 1
        d = dev.DeviceInflate(len(rows))
        t = to_dev(torch, blob)
        out = torch.empty(d.index(t).out_bytes, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.HipDeflateError, match=r"member %d:" % k):
            d.run(t, out)
        assert d.verify(len(rows)) == k
        with pytest.raises(pkg.HipDeflateError):
            pkg.bgzf_decompress_bytes(bytes(blob))
    # two members wrong: the first one is named
    blob = bytearray(good)
    for k in (290, 17):
        blob[rows[k][0] + rows[k][1] - 8] ^= 0x80
    d = dev.DeviceInflate(len(rows))
    t = to_dev(torch, blob)
    with pytest.raises(pkg.HipDeflateError, match="member 17:"):
        d.run(t, torch.empty(len(data), dtype=torch.uint8, device="cuda"))


# ---- the bar ------------------------------------------------------------------------------------------------------


def test_index_takes_at_most_a_tenth_of_the_inflate(pkg, torch):
    """tools/member_index_bench.py on 4 GiB (the tool's own default, when it is run to write profiles/member_index_timing.txt, is 16 GiB): the
    index reads about a fifth of the bytes the inflate moves and has no dependent chain per byte, the inflate runs near
    3 % of HBM peak -- a tenth of its time leaves the scan an order of magnitude above its floor and excludes any serial
    walk over the members."""
    import sys
    sys.path.insert(0, os.path.join(hdtest.ROOT, "tools"))
    bench = importlib.import_module("member_index_bench")
    res = bench.measure(gib=4.0, reps=5, tile_mib=16)
    print(bench.report(res))
    assert res["members"] == res["uncompressed_bytes"] // 0xff00 + 1 and res["candidates"] >= res["members"]
    assert res["index_ms_median"] * 10 <= res["inflate_ms_median"], res
