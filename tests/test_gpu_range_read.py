"""The ranged read -- hipdeflate_read_ranges_dev, DeviceInflate.read_ranges, device.read_ranges -- against the plain
Python plan of tests/range_read_model.py.  Bit-exact, no tolerances: q_len, q_status, dst_off, the whole summary, the
bytes of every accepted query, and 64 sentinel bytes in front of dst and behind out_bytes.  No case provokes a fault:
every refused query and every bad trailer is a case the contract of include/hipdeflate.h defines, and each runs once.

Where the cases land (hd_range.hpp):
  * member counts 63 / 64 / 65 and 2047 / 2048 / 2049: a wavefront and a SCAN_TILE of the coverage, rank and scratch
    scans; query counts 255 / 256 / 257 and 2047 / 2048 / 2049: a workgroup of k_range_resolve, a tile of the q_len and
    piece scans.
  * ranges that end on a member's last byte, start on its first, or are shifted by one: the +1 / -1 of the difference
    array one member off would select, or miss, a neighbour -- nselected and sel_bytes are compared with the model.
  * begin mod 16 x short lengths, dst off alignment, lengths around HD_RANGE_PIECE: the heads, tails and piece seams of
    k_range_gather's compact_wide copies.
  * a table whose out_off passes 2^33: 64-bit positions throughout; a range of 2^32 bytes: q_status 2."""
import importlib
import os
import zlib

import numpy as np
import pytest

import hdtest
import member_index_model as mm
import range_read_model as rm

pytestmark = pytest.mark.gpu

KINDS = ["BC", "MZ", "IG1", "IG2", "MG"]
GUARD = 64
SENT = 0xa5


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


def coded(kind, chunk, level=6, **kw):
    """a member that inflates to chunk"""
    return mm.gz_member(kind, raw_deflate(chunk, level), zlib.crc32(chunk), len(chunk), **kw)


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def tiny_file(pkg, n, seed, kinds=("BC",)):
    """n members: n - 1 tiny coded ones (1..40 input bytes) and the EOF member -> (blob, contents)"""
    rng = np.random.default_rng(seed)
    src = bytes(rng.integers(97, 101, 64, dtype=np.uint8))
    parts, chunks = [], []
    for i in range(n - 1):
        ln = 1 + (i * 7 + seed) % 40
        chunks.append(src[i % 20:i % 20 + ln])
        parts.append(coded(kinds[i % len(kinds)], chunks[-1]))
    return b"".join(parts) + pkg.BGZF_EOF, b"".join(chunks)


def u64(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


class File:
    """a container file on the device with the tables of its members, made once per file: by the device index (and held
    to the model's rows), or from hand-made rows"""

    def __init__(self, torch, dev, blob, data, rows=None):
        self.blob, self.data = to_dev(torch, blob), data
        if rows is None:
            rows = mm.walk(blob)[0]
            self.d = dev.DeviceInflate(len(rows))
            s = self.d.index(self.blob)
            assert (s.status, s.nmembers, s.out_bytes) == (0, len(rows), len(data))
            got = np.stack([t.cpu().numpy().astype(np.int64) & m for t, m in (
                (self.d.in_off, -1), (self.d.in_len, 0xffffffff), (self.d.out_size, 0xffffffff), (self.d.out_off, -1),
                (self.d.crc_want, 0xffffffff))], axis=1)
            assert np.array_equal(got, np.array(rows, dtype=np.int64).reshape(len(rows), 5))
        else:
            self.d = dev.DeviceInflate(len(rows))
            for col, t in enumerate((self.d.in_off, self.d.in_len, self.d.out_size, self.d.out_off, self.d.crc_want)):
                a = np.array([r[col] for r in rows], dtype=np.uint64)
                t.copy_(torch.from_numpy((a.view(np.int64) if t.dtype == torch.int64 else a.astype(np.uint32).view(np.int32)).copy()))
        self.rows = rows


def check(torch, f, kind, begins, ends, shift=0, cap=None, null_dst=False, plan=None):
    """one call on file f, everything held to the model; dst starts `shift` bytes off a 64-byte-aligned guard.
    cap: dst_cap (default out_bytes) -> (plan, summary, bytes of dst)"""
    p = rm.plan(f.rows, kind, begins, ends) if plan is None else plan
    nq = len(begins)
    cap = p["out_bytes"] if cap is None else cap
    buf = torch.full((GUARD + shift + max(cap, p["out_bytes"]) + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    dst = None if null_dst else buf[GUARD + shift:]
    dst_off, q_len, q_status, s = f.d.ranges_call(f.blob, u64(torch, begins), u64(torch, ends), kind, len(f.rows), dst, cap)
    assert q_len.cpu().numpy().view(np.uint32).tolist() == p["q_len"]
    assert q_status.cpu().tolist() == p["q_status"]
    assert dst_off.cpu().tolist() == p["dst_off"]
    assert (s.out_bytes, s.nrefused) == (p["out_bytes"], p["nrefused"])
    assert (s.nselected, s.sel_bytes) == (p["nselected"], p["sel_bytes"]), ((s.nselected, s.sel_bytes), p["selected"][:10])
    got = bytes(buf.cpu().numpy())
    body = got[GUARD + shift:GUARD + shift + p["out_bytes"]]
    if p["out_bytes"] > cap or null_dst:
        assert s.status == (3 if p["out_bytes"] > cap else 0) and s.bad_member == len(f.rows)
        assert got == bytes([SENT]) * len(got)                          # dst is not touched
        return p, s, body
    assert got[:GUARD + shift] == bytes([SENT]) * (GUARD + shift), "bytes in front of dst"
    assert got[GUARD + shift + p["out_bytes"]:] == bytes([SENT]) * (len(got) - GUARD - shift - p["out_bytes"]), "bytes behind out_bytes"
    return p, s, body


def check_bytes(f, p, body, skip=()):
    for q, (b, e) in enumerate(p["spans"]):
        if q not in skip:
            assert body[p["dst_off"][q]:p["dst_off"][q] + p["q_len"][q]] == f.data[b:e], ("query", q, (b, e))


def read(torch, f, kind, begins, ends, **kw):
    p, s, body = check(torch, f, kind, begins, ends, **kw)
    assert s.status == 0 and s.bad_member == len(f.rows)
    check_bytes(f, p, body)
    return p, s, body


# ---- 1. member counts ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049])
def test_member_counts(pkg, torch, dev, n):
    blob, data = tiny_file(pkg, n, seed=n, kinds=KINDS)
    f = File(torch, dev, blob, data)
    total = len(data)
    begins, ends = [0, 0, total], [total, 0, total]                       # the whole file, two empty queries
    for r in f.rows:
        for db, de in ((0, 0), (-1, -1), (1, 1), (-1, 1), (1, -1)):
            b, e = r[3] + db, r[3] + r[2] + de
            if b >= 0 and e >= 0:
                begins.append(b)
                ends.append(e)                                            # (begin > end where a member of one byte shrinks: refused)
    p, s, _ = read(torch, f, rm.BYTES, begins, ends)
    assert s.nselected == n - 1 and s.sel_bytes == total
    # one member's range alone selects that member alone: the first, one in the middle, the last
    for m in sorted(set([0, (n - 1) // 2, max(n - 2, 0)])):
        if f.rows[m][2]:
            p, s, _ = read(torch, f, rm.BYTES, [f.rows[m][3]], [f.rows[m][3] + f.rows[m][2]])
            assert p["selected"] == [m] and s.nselected == 1


# ---- 2. query counts ----------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def file300(pkg, torch, dev):
    blob, data = tiny_file(pkg, 300, seed=300, kinds=KINDS)
    return File(torch, dev, blob, data)


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_query_counts(torch, file300, nq):
    rng = np.random.default_rng(nq)
    total = len(file300.data)
    begins = [int(x) for x in rng.integers(0, total, nq)]
    ends = [b + int(x) for b, x in zip(begins, rng.integers(0, 300, nq))]
    p, s, _ = read(torch, file300, rm.BYTES, begins, ends)
    if nq == 0:
        assert (s.out_bytes, s.nselected, s.sel_bytes, s.nrefused, s.status) == (0, 0, 0, 0, 0)


def test_no_members_gives_a_zero_summary(torch, dev):
    d = dev.DeviceInflate(4)
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    dst_off, q_len, q_status, s = d.ranges_call(empty, u64(torch, [0, 5]), u64(torch, [9, 7]), rm.BYTES, 0, None, 0)
    assert (s.out_bytes, s.nselected, s.sel_bytes, s.nrefused, s.bad_member, s.status) == (0, 0, 0, 0, 0, 0)
    out, _, _, _, s = dev.read_ranges(empty, [], [])
    assert out.numel() == 0 and s.status == 0


# ---- 3. selection is exact ----------------------------------------------------------------------------------------


def test_selection_with_empty_members(pkg, torch, dev):
    chunks = [bytes(hdtest.synth().text_like(40 + 37 * k, seed=k)) for k in range(20)]
    for k in (0, 4, 5, 11, 19):
        chunks[k] = b""
    blob = b"".join(coded(KINDS[k % 5], c) for k, c in enumerate(chunks)) + pkg.BGZF_EOF * 3
    f = File(torch, dev, blob, b"".join(chunks))
    rows, total = f.rows, len(f.data)
    r3, r6 = rows[3], rows[6]
    begins = [r3[3], r3[3] + r3[2] - 1, r3[3] + r3[2] - 1, r6[3], total, total - 1, total - 5, 0, 0]
    ends = [r3[3] + r3[2], r3[3] + r3[2], r3[3] + r3[2] + 1, r6[3] + 1, total, total + 99, 1 << 40, 1, 0]
    for q in range(len(begins)):                                          # each alone: what it selects is its own
        p, s, _ = read(torch, f, rm.BYTES, begins[q:q + 1], ends[q:q + 1])
    assert rm.plan(rows, rm.BYTES, begins[0:1], ends[0:1])["selected"] == [3]           # ends on member 3's last byte
    assert rm.plan(rows, rm.BYTES, begins[2:3], ends[2:3])["selected"] == [3, 6]        # across the empty 4 and 5
    assert rm.plan(rows, rm.BYTES, begins[4:5], ends[4:5])["selected"] == []            # begin == total
    p, s, _ = read(torch, f, rm.BYTES, begins, ends)
    assert s.nrefused == 0


def test_duplicate_nested_overlapping_unsorted(torch, file300):
    begins = [500, 100, 100, 150, 90, 2000, 0, 100, 3000, 10]
    ends = [900, 400, 400, 200, 120, 2500, 50, 400, 2999, 4000]
    p, s, _ = read(torch, file300, rm.BYTES, begins, ends)
    assert p["q_status"] == [0] * 8 + [1, 0] and s.nrefused == 1


@pytest.fixture(scope="module")
def file2050(pkg, torch, dev):
    blob, data = tiny_file(pkg, 2050, seed=9, kinds=KINDS)                # 2049 members with bytes + the EOF member
    return File(torch, dev, blob, data)


def test_2049_one_byte_queries_in_2049_members(torch, file2050):
    rows = file2050.rows[:2049]
    order = np.random.default_rng(5).permutation(2049)
    begins = [rows[m][3] + rows[m][2] // 2 for m in order]
    p, s, _ = read(torch, file2050, rm.BYTES, begins, [b + 1 for b in begins])
    assert s.nselected == 2049 and s.out_bytes == 2049 and s.sel_bytes == len(file2050.data)


def test_2049_queries_in_one_member(torch, file2050):
    r = max(file2050.rows[1000:1100], key=lambda row: row[2])
    assert r[2] >= 30
    begins = [r[3] + q % r[2] for q in range(2049)]
    ends = [min(b + 1 + q % 3, r[3] + r[2]) for q, b in enumerate(begins)]
    p, s, _ = read(torch, file2050, rm.BYTES, begins, ends)
    assert s.nselected == 1 and s.sel_bytes == r[2]


def test_one_query_over_all_2049_members(torch, file2050):
    p, s, _ = read(torch, file2050, rm.BYTES, [0], [len(file2050.data)])
    assert s.nselected == 2049 and s.out_bytes == s.sel_bytes == len(file2050.data)


# ---- 4. gather edges ----------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def file3(pkg, torch, dev):
    data = bytes(hdtest.synth().fastq_like(3 * 0xff00, seed=41))
    blob = b"".join(coded("BC", data[o:o + 0xff00], 1) for o in range(0, len(data), 0xff00)) + pkg.BGZF_EOF
    return File(torch, dev, blob, data)


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_every_begin_alignment_and_short_lengths(torch, file3, shift):
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 47, 4095, 4096, 4097]
    begins, ends = [], []
    for a in range(16):
        for k, ln in enumerate(lengths):
            b = 0xff00 - 2000 + 16 * (7 * k + a) + a                      # begin mod 16 == a; the long ones cross into member 1
            begins.append(b)
            ends.append(b + ln)
    assert sorted(set(b % 16 for b in begins)) == list(range(16))
    read(torch, file3, rm.BYTES, begins, ends, shift=shift)


def test_dst_every_misalignment(torch, file3):
    begins = [3, 70000, 0xff00 - 1, 131000, 5]
    ends = [20, 70040, 0xff00 + 17, 135097, 5]
    for shift in range(1, 16):
        read(torch, file3, rm.BYTES, begins, ends, shift=shift)


@pytest.fixture(scope="module")
def file1m(pkg, torch, dev):
    data = bytes(hdtest.synth().fastq_like(17 * 0xff00 - 321, seed=42))
    blob = b"".join(coded("BC", data[o:o + 0xff00], 1) for o in range(0, len(data), 0xff00)) + pkg.BGZF_EOF
    return File(torch, dev, blob, data)


def test_lengths_around_a_piece(pkg, torch, file1m):
    piece = pkg.RANGE_PIECE
    assert len(file1m.data) > 2 * piece + 5 + 70000
    lengths = [piece - 1, piece, piece + 1, 2 * piece + 5]
    begins = [1234 + 4099 * k for k in range(4)]
    p, s, _ = read(torch, file1m, rm.BYTES, begins, [b + ln for b, ln in zip(begins, lengths)], shift=3)
    assert p["q_len"] == lengths


# ---- 5. virtual offsets -------------------------------------------------------------------------------------------


def test_virtual_offsets_of_a_mixed_file(pkg, torch, dev):
    chunks = [bytes(hdtest.synth().text_like(60 + 211 * k, seed=50 + k)) for k in range(25)]
    chunks[8] = chunks[9] = b""
    blob = b"".join(coded(KINDS[k % 5], c, fname=b"f%d" % k if k % 2 else b"", fcomment=b"c" if k % 3 == 0 else b"",
                          fhcrc=k % 4 == 0) for k, c in enumerate(chunks)) + pkg.BGZF_EOF
    f = File(torch, dev, blob, b"".join(chunks))
    rows, total = f.rows, len(f.data)
    starts, end = rm.member_starts(rows)
    assert end == len(blob)
    V = pkg.voffset
    begins, ends = [], []
    for m, r in enumerate(rows):
        s, size = starts[m], r[2]
        nxt = V(starts[m + 1], 0) if m + 1 < len(rows) else V(end, 0)
        for b, e in ((V(s, 0), V(s, size)),                               # the whole member
                     (V(s, 0), V(s, size + 1)),                           # uoffset past ISIZE: refused
                     (V(s, size), nxt),                                   # uoffset == ISIZE is the next member's first byte
                     (V(s + 1, 0), nxt),                                  # coffset inside the header: refused
                     (V(s, size // 3), nxt),
                     (V(r[0], 0), nxt),                                   # coffset of the payload: refused
                     (V(s, 0), V(end, 0))):                               # to the end of the file
            begins.append(b)
            ends.append(e)
    begins += [V(end, 0), V(0, 0), V(starts[3], 5), V(0, 0)]
    ends += [V(end, 0), V(end, 1), V(starts[2], 5), V(end, 0)]            # the total; refused; U(begin) > U(end); everything
    p, s, body = read(torch, f, rm.VOFFSET, begins, ends)
    assert p["q_status"][:7] == [0, 1, 0, 1, 0, 1, 0] and p["q_status"][-4:] == [0, 1, 1, 0] and p["q_len"][-1] == total
    # the accepted ones, translated to byte ranges, give the same bytes at the same places
    ok = [q for q in range(len(begins)) if p["q_status"][q] == 0]
    p2, s2, body2 = read(torch, f, rm.BYTES, [p["spans"][q][0] for q in ok], [p["spans"][q][1] for q in ok])
    assert body2 == body and (s2.nselected, s2.sel_bytes) == (s.nselected, s.sel_bytes)


# ---- 6. room ------------------------------------------------------------------------------------------------------


def test_room(torch, file300):
    begins = [10, 700, 5000, 3, 9]
    ends = [300, 1900, 5001, 2, 9]
    p, s, _ = check(torch, file300, rm.BYTES, begins, ends)
    assert s.status == 0 and p["out_bytes"] == 290 + 1200 + 1
    _, s, _ = check(torch, file300, rm.BYTES, begins, ends, cap=p["out_bytes"] - 1)
    assert s.status == 3
    _, s, _ = check(torch, file300, rm.BYTES, begins, ends, cap=0, null_dst=True)           # the sizing call
    assert s.status == 3 and s.out_bytes == p["out_bytes"]
    _, s, _ = check(torch, file300, rm.BYTES, begins, ends, cap=p["out_bytes"] + 100)
    assert s.status == 0
    _, s, _ = check(torch, file300, rm.BYTES, [5, 9], [4, 9], cap=0, null_dst=True)         # nothing to deliver: no room needed
    assert s.status == 0 and s.out_bytes == 0


# ---- 7. bad trailer -----------------------------------------------------------------------------------------------


def test_bad_trailer(pkg, torch, dev):
    chunks = [bytes(hdtest.synth().text_like(900 + 50 * k, seed=70 + k)) for k in range(10)]
    good = b"".join(coded("BC", c) for c in chunks) + pkg.BGZF_EOF
    data = b"".join(chunks)
    rows = mm.walk(good)[0]

    def flipped(*members):
        blob = bytearray(good)
        for k in members:
            blob[rows[k][0] + rows[k][1] - 8] ^= 1
        return File(torch, dev, bytes(blob), data)
    k = 6
    f = flipped(k)
    rk = f.rows[k]
    avoid_b = [0, f.rows[2][3] + 5, rk[3] + rk[2], f.rows[9][3]]
    avoid_e = [rk[3], f.rows[4][3], rk[3] + rk[2] + 10, f.rows[9][3] + 100]
    p, s, _ = read(torch, f, rm.BYTES, avoid_b, avoid_e)                   # only selected members are decoded
    assert k not in p["selected"] and k - 1 in p["selected"] and k + 1 in p["selected"]
    begins = avoid_b + [rk[3] - 1, rk[3] + 10]
    ends = avoid_e + [rk[3] + 1, rk[3] + 20]
    p, s, body = check(torch, f, rm.BYTES, begins, ends)
    assert (s.status, s.bad_member) == (2, k)
    check_bytes(f, p, body, skip=(4, 5))                                   # the other queries' bytes are right
    with pytest.raises(pkg.HipDeflateError, match="member %d:" % k):
        f.d.read_ranges(f.blob, begins, ends)
    f = flipped(8, 3)
    p, s, _ = check(torch, f, rm.BYTES, [0], [len(data)])
    assert (s.status, s.bad_member) == (2, 3)
    p, s, _ = check(torch, f, rm.BYTES, [f.rows[5][3]], [len(data)])
    assert (s.status, s.bad_member) == (2, 8)


# ---- 8. past 2^32 -------------------------------------------------------------------------------------------------


def test_positions_past_four_gib(pkg, torch, dev):
    a, b = bytes(hdtest.synth().text_like(3000, seed=81)), bytes(hdtest.synth().text_like(2000, seed=82))
    ma, mb = coded("BC", a), coded("MZ", b)
    filler = bytes(64)                                                     # where the two huge rows point: never read
    blob = ma + filler + mb
    big = 0xffffffff
    off_b = len(a) + 2 * big + big
    assert off_b > 1 << 33
    rows = [(18, len(ma) - 18, len(a), 0, zlib.crc32(a)),
            (len(ma) + 8, 16, big, len(a), 0), (len(ma) + 32, 16, big, len(a) + big, 0),
            (len(ma) + 56, 8, big, len(a) + 2 * big, 0),
            (len(ma) + 64 + 20, len(mb) - 20, len(b), off_b, zlib.crc32(b))]
    f = File(torch, dev, blob, None, rows=rows)
    total = off_b + len(b)
    begins = [5, off_b + 7, 100, off_b, len(a) - 1, total - 1, 0]
    ends = [2900, off_b + 1500, 100 + (1 << 32), total + 5, len(a) - 1 + (1 << 32), total, total]
    p, s, body = check(torch, f, rm.BYTES, begins, ends)
    assert p["q_status"] == [0, 0, 2, 0, 2, 0, 2] and p["selected"] == [0, 4]
    assert (s.status, s.nselected, s.sel_bytes, s.nrefused) == (0, 2, len(a) + len(b), 3)
    want = [a[5:2900], b[7:1500], b"", b, b"", b[-1:], b""]
    for q, w in enumerate(want):
        assert body[p["dst_off"][q]:p["dst_off"][q] + p["q_len"][q]] == w, q


# ---- 9. the library's own files -----------------------------------------------------------------------------------


@pytest.mark.parametrize("level", [1, 6])
def test_own_files_random_ranges_and_virtual_offsets(pkg, torch, dev, level):
    n = 2 << 20
    data = hdtest.synth().fastq_like(n, seed=90 + level)
    src = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    in_off, in_len = dev.block_table(n, pkg.BGZF_BLOCK)
    nb = in_off.numel()
    enc = dev.DeviceDeflate(nb)
    enc.run(src, in_off, in_len, level=level)
    enc.scan()
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    comp = int(enc.total[0])
    blob = torch.empty(comp + len(pkg.BGZF_EOF), dtype=torch.uint8, device="cuda")
    enc.compact(blob)
    blob[comp:] = torch.frombuffer(bytearray(pkg.BGZF_EOF), dtype=torch.uint8).cuda()
    member_at = enc.dst_off.cpu().tolist()                                # where the gather put member i
    data = bytes(data)
    rng = np.random.default_rng(level)
    begins = [int(x) for x in rng.integers(0, n, 500)]
    ends = [min(n, b + int(x)) for b, x in zip(begins, rng.integers(0, 200000, 500))]
    out, dst_off, q_len, q_status, s = dev.read_ranges(blob, begins, ends)
    assert s.status == 0 and s.nrefused == 0 and s.out_bytes == sum(e - b for b, e in zip(begins, ends)) == out.numel()
    got, offs = bytes(out.cpu().numpy()), dst_off.cpu().tolist()
    for q, (b, e) in enumerate(zip(begins, ends)):
        assert got[offs[q]:offs[q] + e - b] == data[b:e], q
    touched = set()
    for b, e in zip(begins, ends):
        if b < e:
            touched.update(range(b // pkg.BGZF_BLOCK, (e - 1) // pkg.BGZF_BLOCK + 1))
    assert s.nselected == len(touched)
    # the same ranges as virtual offsets: member i starts where the gather put it
    vb = [pkg.voffset(member_at[b // pkg.BGZF_BLOCK], b % pkg.BGZF_BLOCK) for b in begins]
    ve = [pkg.voffset(member_at[e // pkg.BGZF_BLOCK], e % pkg.BGZF_BLOCK) if e < n else pkg.voffset(comp, 0) for e in ends]
    out2, dst_off2, q_len2, q_status2, s2 = dev.read_ranges(blob, vb, ve, pkg.RANGE_VOFFSET)
    assert torch.equal(out2, out) and torch.equal(dst_off2, dst_off) and torch.equal(q_len2, q_len)
    assert int(q_status2.abs().sum()) == 0 and (s2.nselected, s2.sel_bytes) == (s.nselected, s.sel_bytes)


# ---- 10. scratch reuse and stream order ---------------------------------------------------------------------------


def test_scratch_reuse_and_a_side_stream(torch, file1m):
    total = len(file1m.data)
    rng = np.random.default_rng(10)
    big_b = [int(x) for x in rng.integers(0, total - 70000, 300)]
    big_e = [b + int(x) for b, x in zip(big_b, rng.integers(1, 70000, 300))]
    small_b, small_e = [17, 70000], [29, 70001]
    plans = {"big": rm.plan(file1m.rows, rm.BYTES, big_b, big_e), "small": rm.plan(file1m.rows, rm.BYTES, small_b, small_e)}

    def rounds():
        out = []
        for name, b, e in (("big", big_b, big_e), ("small", small_b, small_e), ("big", big_b, big_e)):
            p, s, body = read(torch, file1m, rm.BYTES, b, e, plan=plans[name])
            out.append((body, s.nselected, s.sel_bytes))
        return out
    first = rounds()
    assert first[0] == first[2]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = rounds()
    side.synchronize()
    assert second == first
