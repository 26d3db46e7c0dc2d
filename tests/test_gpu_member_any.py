"""The member index that sizes by decoding -- hipdeflate_index_members_any_dev, DeviceInflate.index_any,
inflate_gzip_members, inflate_gzip_file, hip_inflate_members -- against the plain Python walk of tests/member_any_model.py.
Bit-exact: every field of the summary, every table entry, and a sentinel in every entry the call must not touch.  The files
are those of tests/member_any_cases.py, whose classification tests/test_member_any_model.py pins without a GPU.  No case
provokes a fault: each corrupt blob is a case the contract of include/hipdeflate.h defines, and each runs once.

Cuts are made by passing a smaller nbytes over the WHOLE blob in device memory: a read behind nbytes would find the rest of
the member there and answer "ok".

Where the cases land (hd_index.hpp, hd_inflate_size.hpp):
  * member counts 63 / 64 / 65 and 255 / 256 / 257: a wavefront and a workgroup of the one-lane-per-candidate kernels and of
    the subset scan; 5,000 members: several tiles of that scan, 5,000 wavefronts of k_inflate_member.
  * FNAME 63 / 64 / 65 / 5,000: the 64-byte steps of the name scan in k_member_open.
  * the eight ending bits: the byte the trailer is read from (used = ceil(bits / 8)) for static, dynamic and stored blocks.
  * the straddles: MatchAny across a lane's 16 bytes, a wavefront's 1 KiB and a workgroup's 256 KiB.
  * decoys: candidates that are sized but that nothing links to, or whose end joins the true chain."""
import ctypes
import gzip
import importlib
import os

import numpy as np
import pytest

import hdtest
import member_any_cases as mc
import member_any_model as am

pytestmark = pytest.mark.gpu

S64 = 0x5a5a5a5a5a5a5a5a
S32 = 0x5a5a5a5a
GUARD = 8
FIELDS = ("nmembers", "out_bytes", "end_offset", "ncandidates", "nsized", "status")


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


def to_dev(torch, blob):
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]


def sentinel_tables(dev, cap):
    d = dev.DeviceInflate(cap + GUARD)
    d.max_members = cap
    for t in (d.in_off, d.out_off):
        t.fill_(S64)
    for t in (d.in_len, d.out_size, d.crc_want):
        t.fill_(S32)
    return d


def check(dev, torch, case, cap=None, t=None):
    """index the case into a table of `cap` entries (default: the members the model finds + 3) and hold the summary, the
    rows and the sentinels to the model -> (summary, DeviceInflate, device blob)"""
    rows, want = case.model(cap)
    cap = want["nmembers"] + 3 if cap is None else cap
    for k, v in case.want.items():
        assert v is None or cap < want["nmembers"] or want[k] == v, (k, want[k], v)
    d = sentinel_tables(dev, cap)
    t = to_dev(torch, case.blob) if t is None else t
    s = d.index_any(t[:case.nbytes], case.first_offset, case.max_member_in)
    got = {f: getattr(s, f) for f in FIELDS}
    print(got)
    assert got == want, (got, want)
    k = len(rows)
    want_cols = np.array(rows, dtype=np.uint64).reshape(k, 5)
    cols = [x.cpu().numpy() for x in (d.in_off, d.in_len, d.out_size, d.out_off, d.crc_want)]
    for col, (g, wide) in enumerate(zip(cols, (True, False, False, True, False))):
        g = g.view(np.uint64 if wide else np.uint32)
        assert np.array_equal(g[:k].astype(np.uint64), want_cols[:, col]), ("column", col)
        assert np.all(g[k:] == (S64 if wide else S32)), ("sentinel of column", col)
    return s, d, t


def decode(dev, torch, s, d, t):
    out = torch.full((s.out_bytes + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    d.max_members = s.nmembers
    d.run(t, out[:s.out_bytes], s)
    got = bytes(out.cpu().numpy())
    assert got[s.out_bytes:] == b"\x5a" * 16
    return got[:s.out_bytes]


# ---- 1. member counts ----

@pytest.mark.parametrize("n", mc.COUNTS)
def test_member_counts(pkg, torch, dev, n):
    c = mc.counts(n)
    s, d, t = check(dev, torch, c)
    assert s.nmembers == n == s.nsized and s.status == 0
    check(dev, torch, c, cap=n, t=t)                                   # a table of exactly n entries is enough
    if n in (65, 5000):
        assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


def test_three_hundred_empty_members(pkg, torch, dev):
    s, d, t = check(dev, torch, mc.empty_members())
    assert (s.nmembers, s.out_bytes, s.end_offset) == (300, 0, 6000)


# ---- 2. headers ----

@pytest.mark.parametrize("name", list(mc.HEADERS))
def test_headers(pkg, torch, dev, name):
    c = mc.header(name)
    s, d, t = check(dev, torch, c)
    assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


# ---- 3. ending bits ----

@pytest.mark.parametrize("kind", ["stored", "static", "dynamic"])
def test_final_block_ends_on_every_bit(pkg, torch, dev, kind):
    c = mc.ending_bits(kind)
    s, d, t = check(dev, torch, c)
    assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


# ---- 4. alignment ----

def test_member_start_at_every_offset_mod_16(pkg, torch, dev):
    s, _, _ = check(dev, torch, mc.every_alignment())
    assert s.nmembers == 33


@pytest.mark.parametrize("boundary", mc.BOUNDARIES)
def test_magic_across_granule_word_and_tile(pkg, torch, dev, boundary):
    for k in mc.STRADDLES:
        s, _, _ = check(dev, torch, mc.straddle(boundary, k))
        assert s.nmembers == 3 and s.status == 0


# ---- 5. decoys ----

@pytest.mark.parametrize("depth", [1, 2])
def test_a_gz_file_inside_a_stored_payload(pkg, torch, dev, depth):
    c = mc.decoy(depth)
    s, d, t = check(dev, torch, c)
    assert s.nmembers == 3 and s.ncandidates == s.nsized == 3 + 3 * depth
    assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


def test_a_decoy_whose_end_is_a_real_members_start(pkg, torch, dev):
    c = mc.decoy_joins_chain()
    s, d, t = check(dev, torch, c)
    assert (s.nmembers, s.ncandidates) == (3, 4)
    assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


def test_stored_payload_of_nothing_but_magics(pkg, torch, dev):
    c = mc.decoy_magics()
    s, d, t = check(dev, torch, c)
    assert (s.nmembers, s.ncandidates, s.nsized) == (3, 4099, 4099)
    assert decode(dev, torch, s, d, t) == gzip.decompress(c.blob)


# ---- 6. mixed kinds ----

def test_mixed_kinds_interleaved(pkg, torch, dev):
    c = mc.mixed()
    s, d, t = check(dev, torch, c)
    assert s.nmembers == 40 and s.nsized == 15
    assert decode(dev, torch, s, d, t) == mc.gunzip_all(c.blob)[0]


def test_pure_bgzf_sizes_nothing_and_equals_the_old_call(pkg, torch, dev):
    c = mc.pure_bgzf()
    s, d, t = check(dev, torch, c)
    assert s.nmembers == 2048 and s.nsized == 0
    old = sentinel_tables(dev, s.nmembers + 3)
    so = old.index(t)
    assert (so.nmembers, so.out_bytes, so.end_offset, so.status) == (s.nmembers, s.out_bytes, s.end_offset, 0)
    for a, b in zip((d.in_off, d.in_len, d.out_size, d.out_off, d.crc_want), (old.in_off, old.in_len, old.out_size, old.out_off, old.crc_want)):
        assert torch.equal(a, b)


# ---- 7. cuts and corruption ----

def test_cut_at_every_byte_of_the_last_header_and_trailer(pkg, torch, dev):
    cuts = mc.cuts()
    t = to_dev(torch, cuts[0][1].blob)
    for nbytes, c in cuts:
        s, _, _ = check(dev, torch, c, t=t)
        assert (s.status, s.nmembers) == (2, 2), nbytes


@pytest.mark.parametrize("kind", mc.CORRUPT)
def test_corruptions(pkg, torch, dev, kind):
    c = mc.corrupt(kind)
    s, d, t = check(dev, torch, c)
    assert s.status == c.want["status"]
    if kind == "crc":                                                  # the index does not examine the CRC: the verify names the member
        out = torch.empty(s.out_bytes, dtype=torch.uint8, device="cuda")
        dev.device_inflate(t, d.in_off[:3], d.in_len, out, d.out_off, d.out_size, d.out_len, d.crc, d.status)
        assert d.verify(3) == 1
        with pytest.raises(pkg.HipDeflateError):
            dev.inflate_gzip_members(t)


# ---- 8. max_member_in ----

@pytest.mark.parametrize("kind", mc.BOUNDED)
def test_max_member_in(pkg, torch, dev, kind):
    c = mc.bounded(kind)
    s, _, _ = check(dev, torch, c)
    assert s.status == c.want["status"]


def test_max_member_in_beyond_the_most_is_refused(pkg, torch, dev):
    t = to_dev(torch, mc.counts(2).blob)
    s = pkg.MemberAnySummary()
    args = (t.data_ptr(), t.numel(), 0, 0)
    assert pkg.lib().hipdeflate_index_members_any_dev(*args, am.MAX_IN, None, None, None, None, None, ctypes.byref(s), None) == pkg.HD_E_ARG
    assert pkg.lib().hipdeflate_index_members_any_dev(*args, am.MAX_IN - 1, None, None, None, None, None, ctypes.byref(s), None) == 0
    assert (s.nmembers, s.status) == (2, 3)


# ---- 9. first_offset ----

def test_first_offset(pkg, torch, dev):
    cases = mc.resumes()
    t = to_dev(torch, cases[0][1].blob)
    for k, c in cases:
        s, _, _ = check(dev, torch, c, t=t)
        assert s.status == c.want["status"], k
    s = pkg.MemberAnySummary()
    rc = pkg.lib().hipdeflate_index_members_any_dev(t.data_ptr(), t.numel(), t.numel() + 1, 0, 0, None, None, None, None, None,
                                                    ctypes.byref(s), None)
    assert rc == pkg.HD_E_ARG


# ---- 10. table too small ----

def test_table_too_small_sizing_call_and_no_bytes(pkg, torch, dev):
    c = mc.counts(65)
    s, _, t = check(dev, torch, c, cap=64)
    assert (s.status, s.nmembers, s.end_offset) == (3, 65, len(c.blob))
    s = dev.DeviceInflate(0).index_any(t)                              # NULL tables of no entries
    _, want = c.model(cap=0)
    assert {f: getattr(s, f) for f in FIELDS} == want and s.status == 3
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    s = sentinel_tables(dev, 4).index_any(empty)
    assert {f: getattr(s, f) for f in FIELDS} == dict.fromkeys(FIELDS, 0)


# ---- 11. end to end ----

@pytest.fixture(scope="module")
def thousand():
    """1,000 members of 1..70,000 bytes, at levels 0, 1 and 6"""
    parts, data = [], []
    for i in range(1000):
        n = 1 + (i * i * 7919 + 13 * i) % 70000
        chunk = mc.text(n, seed=i)
        parts.append(am.plain_member(chunk, level=(0, 1, 6)[i % 3]))
        data.append(chunk)
    return b"".join(parts), b"".join(data)


def test_inflate_gzip_members_and_ranges(pkg, torch, dev, thousand):
    blob, data = thousand
    assert gzip.decompress(blob) == data
    t = to_dev(torch, blob)
    out = dev.inflate_gzip_members(t)
    assert bytes(out.cpu().numpy()) == data
    d = dev.DeviceInflate(1000)
    s = d.index_any(t)
    assert (s.nmembers, s.out_bytes, s.status, s.ncandidates) == (1000, len(data), 0, len(am.candidates(blob)))
    begins = [0, 1, len(data) // 3, len(data) - 70001, len(data) - 1]
    ends = [1, 70001, len(data) // 3 + 200000, len(data), len(data)]
    got, dst_off, q_len, q_status, _ = d.read_ranges(t, begins, ends)
    got, dst_off, q_len = bytes(got.cpu().numpy()), dst_off.cpu().numpy(), q_len.cpu().numpy()
    assert not q_status.cpu().numpy().any()
    for q, (b, e) in enumerate(zip(begins, ends)):
        assert got[int(dst_off[q]):int(dst_off[q]) + int(q_len[q])] == data[b:e], q
    assert pkg.lib().hipdeflate_stall_count() == 0


def test_inflate_gzip_file_with_members_large_and_small(pkg, torch, dev):
    big = mc.text(1 << 20, seed=0) * 3 + mc.text(12345, seed=3)        # 3 MiB and a bit in one member
    parts = [mc.small(0, seed=120), mc.small(1, seed=120), am.plain_member(big), mc.small(3, seed=120), am.plain_member(mc.text(300000, seed=5))]
    blob, data = b"".join(parts), gzip.decompress(b"".join(parts))
    t = to_dev(torch, blob)
    assert bytes(dev.inflate_gzip_file(t).cpu().numpy()) == data      # everything fits the library's bound: one index
    small_only = to_dev(torch, b"".join(parts[:2]))
    assert bytes(dev.inflate_gzip_file(small_only, max_member_in=1 << 20).cpu().numpy()) == gzip.decompress(b"".join(parts[:2]))
    assert len(parts[2]) > 1 << 18 and len(parts[4]) < 1 << 18
    assert bytes(dev.inflate_gzip_file(t, max_member_in=1 << 18).cpu().numpy()) == data    # the long member goes through the block index
    with pytest.raises(pkg.HipDeflateError):
        dev.inflate_gzip_members(t, max_member_in=1 << 18)
    assert pkg.lib().hipdeflate_stall_count() == 0


def test_hip_inflate_members(pkg, thousand):
    blob, data = thousand
    r, out, need, used = pkg.hip_inflate_members(blob, len(data))
    assert (r, need, used) == (0, len(data), len(blob)) and out == data
    r, out, need, used = pkg.hip_inflate_members(blob, len(data) - 1)
    assert (r, need, used) == (3, len(data), len(blob))
    c = mc.corrupt("garbage")
    r, _, _, used = pkg.hip_inflate_members(c.blob, 1 << 20)
    assert (r, used) == (1, c.want["end_offset"])
    assert pkg.hip_inflate_members(mc.corrupt("crc").blob, 1 << 20)[0] == 1
    r, out, need, used = pkg.hip_inflate_members(b"", 16)
    assert (r, out, need, used) == (0, b"", 0, 0)
    assert pkg.lib().hipdeflate_stall_count() == 0


# ---- 12. far offsets ----

def test_members_past_four_gib(pkg, torch, dev):
    """a 64 MiB tile of 64 stored members of about 1 MiB, 71 times on the device: 4.4 GiB.  The first and last rows and the
    rows either side of 2^32 against the tiling arithmetic; out_off passes 2^32 with in_off."""
    import far_offsets as fo
    tile_bytes, reps = 64 << 20, 71
    parts = [mc.stored_of_length(1 << 20, seed=200 + i) for i in range(63)]
    parts.append(mc.stored_of_length(tile_bytes - 63 * (1 << 20), seed=263))
    tile = b"".join(parts)
    assert len(tile) == tile_bytes and am.candidates(tile) == mc.starts(parts)[:-1]
    rows, status, end = am.walk(tile)
    assert status == 0 and len(rows) == 64
    tile_out = sum(r[2] for r in rows)
    tile_dev = torch.from_numpy(np.frombuffer(tile, dtype=np.uint8).copy()).cuda()
    blob = torch.empty(reps * tile_bytes + 16, dtype=torch.uint8, device="cuda")[:reps * tile_bytes]
    blob.view(reps, tile_bytes)[:] = tile_dev[None, :]
    n = 64 * reps
    d = sentinel_tables(dev, n)
    s = d.index_any(blob)
    assert {f: getattr(s, f) for f in FIELDS} == {"nmembers": n, "out_bytes": reps * tile_out, "end_offset": reps * tile_bytes,
                                                  "ncandidates": n, "nsized": n, "status": 0}
    assert s.end_offset > fo.P32 and s.out_bytes > fo.P32
    cross = fo.P32 // tile_bytes * 64                                 # the first row whose member starts at or past 2^32
    cols = [x.cpu().numpy().view(np.uint64 if wide else np.uint32) for x, wide in
            ((d.in_off, True), (d.in_len, False), (d.out_size, False), (d.out_off, True), (d.crc_want, False))]
    for i in (0, 1, cross - 1, cross, cross + 1, n - 1):
        r, k = rows[i % 64], i // 64
        want = (k * tile_bytes + r[0], r[1], r[2], k * tile_out + r[3], r[4])
        assert tuple(int(c[i]) for c in cols) == want, i
    assert int(cols[0][cross]) >= fo.P32 > int(cols[0][cross - 1])
    for c, wide in zip(cols, (True, False, False, True, False)):
        assert np.all(c[n:] == (S64 if wide else S32))
    # every row, by the same arithmetic, on the device
    k = torch.arange(n, device="cuda") // 64
    base = torch.from_numpy(np.array([r[0] for r in rows], dtype=np.int64)).cuda().repeat(reps)
    assert torch.equal(d.in_off[:n], k * tile_bytes + base)
