"""The device gather under every pipe and batch call -- hipdeflate_scan_sizes_dev, hipdeflate_compact_dev,
hipdeflate_compact_span_dev -- and the Adler-32 patch kernel of HD_FRAME_ZLIB, each against a plain reference:
numpy's uint64 cumsum, a byte-by-byte placement into a pre-filled buffer, zlib.adler32.  Bit-exact, no tolerances.

Where the cases land (hd_compact.hpp):
  * n around 8 / 64 / 2,048 / 524,288: a thread's eight elements, a wavefront, a tile (SCAN_TILE), and the 256 tiles
    up to which k_scan_tiles gives each thread one tile; 1,200,000 is 586 tiles, three per thread, the last thread's
    share ragged.
  * 0xffffffff everywhere: a thread's sum is 2^35 - 8, a wavefront's passes 2^32 in its first lane pair -- the split
    of wave_incl_scan64; a tile's sum passes 2^43.
  * base 2^32 - 1 and 2^40 + 5: the carry out of the low dword on the first add, and a base with both halves set --
    what a higher rank of a sharded stream passes.
  * members of 0..3 bytes at each destination alignment: shorter than compact_one's head."""
import importlib
import os
import zlib

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

SCAN_N = [1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4096, 524287, 524288, 524289, 1200000]
SCAN_BASES = [0, 1, 2 ** 32 - 1, 2 ** 40 + 5]
SCAN_VALUES = ["zero", "one", "below_65536", "whole_u32", "all_ffffffff", "tile_first", "tile_last"]
TILE = 2048                                    # hd_compact.hpp SCAN_TILE
SENTINEL = -0x0123456789abcdef                 # what dst_off / total hold before a scan


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


def scan_values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, dtype=np.uint32)
    if kind == "one":
        return np.ones(n, dtype=np.uint32)
    if kind == "below_65536":
        return rng.integers(0, 65536, n, dtype=np.uint32)
    if kind == "whole_u32":
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "all_ffffffff":
        return np.full(n, 0xffffffff, dtype=np.uint32)
    v = np.zeros(n, dtype=np.uint32)
    if kind == "tile_first":
        v[0::TILE] = 0xffffffff
    else:
        v[TILE - 1::TILE] = 0xffffffff
        v[n - 1] = 0xffffffff                  # (the ragged last tile's last element too)
    return v


def scan_reference(vals, base):
    """-> (exclusive offsets + base, total without base), numpy uint64; asserts that nothing wraps 2^64"""
    n = len(vals)
    assert n * (int(vals.max()) if n else 0) + base < 2 ** 53, "the reference itself would not be exact"
    incl = np.cumsum(vals, dtype=np.uint64)
    excl = np.concatenate([np.zeros(1, dtype=np.uint64), incl[:-1]]) if n else np.zeros(0, dtype=np.uint64)
    return excl + np.uint64(base), int(incl[-1]) if n else 0


def dev_u32(torch, vals):
    return torch.from_numpy(np.ascontiguousarray(vals).view(np.int32)).cuda()


def run_scan(pkg, torch, d_len, n, base, want_total=True, stream=None):
    """-> (dst_off tensor of n + 8 int64 pre-filled with SENTINEL, total tensor or None); enqueued, not synchronised"""
    d_off = torch.full((n + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    d_total = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda") if want_total else None
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())           # the fills above
    rc = pkg.lib().hipdeflate_scan_sizes_dev(d_len.data_ptr() if d_len is not None else None, n, base, d_off.data_ptr(),
                                             d_total.data_ptr() if want_total else None, st.cuda_stream)
    assert rc == 0
    return d_off, d_total


def check_scan(d_off, d_total, vals, base, what):
    n = len(vals)
    want_off, want_total = scan_reference(vals, base)
    got = d_off.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint64), want_off), \
        (what, "first wrong element", int(np.nonzero(got[:n].view(np.uint64) != want_off)[0][0]))
    assert np.all(got[n:] == SENTINEL), (what, "written behind element n")
    if d_total is not None:
        assert int(d_total.cpu().numpy().view(np.uint64)[0]) == want_total, (what, "total excludes base")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_sizes_equal_numpy_cumsum(pkg, torch, n):
    """dst_off = base + exclusive uint64 prefix sum, total = the sum without base, for every value set and base"""
    for k, kind in enumerate(SCAN_VALUES):
        vals = scan_values(kind, n, 1000 + k)
        d_len = dev_u32(torch, vals)
        for base in SCAN_BASES:
            d_off, d_total = run_scan(pkg, torch, d_len, n, base)
            torch.cuda.synchronize()
            check_scan(d_off, d_total, vals, base, (kind, n, base))
    # total = NULL is accepted
    vals = scan_values("whole_u32", n, 5)
    d_off, _ = run_scan(pkg, torch, dev_u32(torch, vals), n, 2 ** 40 + 5, want_total=False)
    torch.cuda.synchronize()
    check_scan(d_off, None, vals, 2 ** 40 + 5, ("no total", n))


@pytest.mark.timeout(300)
def test_scan_of_nothing_zeroes_total(pkg, torch):
    for base in SCAN_BASES:
        d_off, d_total = run_scan(pkg, torch, None, 0, base)
        torch.cuda.synchronize()
        assert int(d_total.item()) == 0 and np.all(d_off.cpu().numpy() == SENTINEL)
    d_off, _ = run_scan(pkg, torch, None, 0, 7, want_total=False)
    torch.cuda.synchronize()
    assert np.all(d_off.cpu().numpy() == SENTINEL)


@pytest.mark.timeout(300)
def test_two_scans_on_two_streams_share_the_tile_buffer(pkg, torch):
    """1,200,000 sizes on one stream and 9 on another, issued back to back: the second must not touch the tile
    buffer before the first has finished with it"""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd, (kind_a, kind_b) in enumerate([("all_ffffffff", "whole_u32"), ("whole_u32", "all_ffffffff"),
                                             ("tile_last", "one"), ("below_65536", "tile_first")]):
        a, b = scan_values(kind_a, 1200000, 40 + rnd), scan_values(kind_b, 9, 50 + rnd)
        d_a, d_b = dev_u32(torch, a), dev_u32(torch, b)
        torch.cuda.synchronize()
        off_a, tot_a = run_scan(pkg, torch, d_a, len(a), 2 ** 40 + 5, stream=s1)
        off_b, tot_b = run_scan(pkg, torch, d_b, len(b), 2 ** 32 - 1, stream=s2)
        off_a2, tot_a2 = run_scan(pkg, torch, d_a, len(a), 1, stream=s2)         # and a large one behind the small
        off_b2, tot_b2 = run_scan(pkg, torch, d_b, len(b), 0, stream=s1)
        torch.cuda.synchronize()
        check_scan(off_a, tot_a, a, 2 ** 40 + 5, ("large, first stream", rnd))
        check_scan(off_b, tot_b, b, 2 ** 32 - 1, ("small, second stream", rnd))
        check_scan(off_a2, tot_a2, a, 1, ("large, second stream", rnd))
        check_scan(off_b2, tot_b2, b, 0, ("small, first stream", rnd))


# ---- compact --------------------------------------------------------------------------------------------------------

COMPACT_LENGTHS = list(range(0, 71)) + list(range(4093, 4101))
COMPACT_STRIDES = [16, 80, 4112, 65536]
# the (stride, length) pairs that run: every length that fits the stride
COMPACT_PAIRS = [(s, L) for s in COMPACT_STRIDES for L in COMPACT_LENGTHS if L <= s]
SPAN_BASES = [0, 16, 2 ** 33 + 3]


def compact_layout(lengths):
    """Hand-made destination offsets: every length at each destination alignment 0..3, gaps of 0..7 bytes between
    members.  -> [(length, offset)], bytes of the destination"""
    out, pos = [], 0
    for j, (L, a) in enumerate((L, a) for L in lengths for a in range(4)):
        gap = (a - pos) & 3
        if (j // 4 + j) & 1:
            gap += 4
        out.append((L, pos + gap))
        pos += gap + L
    return out, pos + 64


@pytest.mark.timeout(300)
def test_compact_pairs_are_the_stated_ones():
    assert len(COMPACT_PAIRS) == 17 + 71 + 79 + 79
    assert [L for s, L in COMPACT_PAIRS if s == 16] == list(range(17))
    for s in COMPACT_STRIDES:
        lay, size = compact_layout([L for st, L in COMPACT_PAIRS if st == s])
        ends = [0] + [o + L for L, o in lay]
        gaps = [o - e for (L, o), e in zip(lay, ends)]
        assert set(gaps) == set(range(8)), (s, sorted(set(gaps)))
        for L in set(L for L, _ in lay):
            assert sorted(o & 3 for l2, o in lay if l2 == L) == [0, 1, 2, 3]
        assert size == ends[-1] + 64


@pytest.mark.timeout(300)
@pytest.mark.parametrize("span_base", SPAN_BASES)
@pytest.mark.parametrize("stride", COMPACT_STRIDES)
def test_compact_places_every_member_and_nothing_else(pkg, torch, stride, span_base):
    lengths = [L for s, L in COMPACT_PAIRS if s == stride]
    lay, size = compact_layout(lengths)
    n = len(lay)
    rng = np.random.default_rng(stride)
    slots = rng.integers(0, 256, n * stride, dtype=np.uint8)
    want = np.full(size, 0xa5, dtype=np.uint8)
    for i, (L, o) in enumerate(lay):
        want[o:o + L] = slots[i * stride: i * stride + L]
    d_slots = torch.from_numpy(slots).cuda()
    d_len = dev_u32(torch, np.array([L for L, _ in lay], dtype=np.uint32))
    d_off = torch.from_numpy(np.array([o + span_base for _, o in lay], dtype=np.uint64).view(np.int64)).cuda()
    d_dst = torch.full((size,), 0xa5, dtype=torch.uint8, device="cuda")
    assert d_dst.data_ptr() % 4 == 0 and d_slots.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    L_ = pkg.lib()
    if span_base == 0:
        rc = L_.hipdeflate_compact_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                       d_dst.data_ptr(), st)
    else:
        rc = L_.hipdeflate_compact_span_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                            d_dst.data_ptr(), span_base, st)
    assert rc == 0
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        inside = [(i, L, o) for i, (L, o) in enumerate(lay) if o <= k < o + L]
        raise AssertionError("stride %d span_base %d: byte %d is %#x, not %#x (%s)" % (
            stride, span_base, k, got[k], want[k], "member %d, length %d at %d" % inside[0] if inside else "a gap byte"))


@pytest.mark.timeout(300)
def test_compact_refuses_what_it_cannot_address(pkg, torch):
    """stride & 3 or a misaligned slots pointer: HD_E_ARG, and nothing is written"""
    d_slots = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_len = dev_u32(torch, np.array([8, 8], dtype=np.uint32))
    d_off = torch.from_numpy(np.array([0, 8], dtype=np.int64)).cuda()
    d_dst = torch.full((64,), 0xa5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L_ = pkg.lib()
    for stride, delta in ((18, 0), (17, 0), (6, 0), (16, 1), (16, 2), (16, 3)):
        assert L_.hipdeflate_compact_dev(d_slots.data_ptr() + delta, stride, d_len.data_ptr(), d_off.data_ptr(), 2,
                                         d_dst.data_ptr(), st) == pkg.HD_E_ARG, (stride, delta)
        assert L_.hipdeflate_compact_span_dev(d_slots.data_ptr() + delta, stride, d_len.data_ptr(), d_off.data_ptr(), 2,
                                              d_dst.data_ptr(), 0, st) == pkg.HD_E_ARG, (stride, delta)
    torch.cuda.synchronize()
    assert bool((d_dst == 0xa5).all())
    assert L_.hipdeflate_compact_dev(d_slots.data_ptr(), 16, d_len.data_ptr(), d_off.data_ptr(), 2, d_dst.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((d_dst[:16] == 0).all()) and bool((d_dst[16:] == 0xa5).all())


# ---- Adler-32 patch kernel --------------------------------------------------------------------------------------------

ADLER_LENGTHS = [1, 15, 16, 17, 5552, 5553, 65520, 65521, 65522, 1 << 20, 8 << 20]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level", [0, 1])
def test_zlib_members_carry_the_adler32_of_their_block(pkg, torch, level):
    """HD_FRAME_ZLIB members of all-0xff blocks (the input that overflows a sum reduced too late) and of random
    bytes, around 16 bytes (a lane's share), NMAX = 5552, the modulus 65521 and far beyond, the source at offsets
    0 and 3 (mod 16): the trailer k_adler32_patch writes == zlib.adler32"""
    rng = np.random.default_rng(99)
    blocks, offs, pos = [], [], 0
    for n in ADLER_LENGTHS:
        for content in ("ff", "random"):
            for shift in (0, 3):
                blocks.append(np.full(n, 0xff, dtype=np.uint8) if content == "ff" else rng.integers(0, 256, n, dtype=np.uint8))
                offs.append(pos + shift)
                pos += (n + shift + 15) // 16 * 16 + 16
    host = np.zeros(pos + 16, dtype=np.uint8)
    for b, o in zip(blocks, offs):
        host[o:o + len(b)] = b
    nb = len(blocks)
    slot = int(pkg.lib().hipdeflate_bound(max(ADLER_LENGTHS), level))
    assert slot % 16 == 0
    d_in = torch.from_numpy(host).cuda()
    d_off = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
    d_len = dev_u32(torch, np.array([len(b) for b in blocks], dtype=np.uint32))
    d_slots = torch.zeros(nb * slot, dtype=torch.uint8, device="cuda")
    d_olen = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_st = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_slots.data_ptr() % 16 == 0
    rc = pkg.lib().hipdeflate_batch_deflate_dev(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), nb, level,
                                                pkg.FRAME_ZLIB, d_slots.data_ptr(), slot, slot, d_olen.data_ptr(), None,
                                                d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    olen = d_olen.cpu().numpy().view(np.uint32)
    for i, b in enumerate(blocks):
        m = bytes(d_slots[i * slot: i * slot + int(olen[i])].cpu().numpy())
        what = (level, len(b), "ff" if b[0] == 0xff and b[-1] == 0xff and len(b) > 1 else "?", offs[i] & 15)
        assert m[:2] == b"\x78\xda", what
        assert int.from_bytes(m[-4:], "big") == zlib.adler32(b.tobytes()), what
        assert zlib.decompress(m) == b.tobytes(), what
