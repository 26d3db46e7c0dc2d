"""The gather kernel (k_compact, hd_compact.hpp) where a copy of 16 bytes per lane and a persistent grid can go wrong,
bit-exact against a byte-by-byte numpy placement into a destination pre-filled with 0xa5 (the scheme of
tests/test_gpu_gather.py, which stops at destination alignment mod 4, 16-aligned slots and ~320 members).

Where the cases land:
  * every destination alignment 0..15 for every length: the head in front of the first whole 16-byte line is 0..15 bytes;
  * the slot array at +0, +4, +8, +12 from a 16-aligned tensor and strides 20, 84, 4116, 65536 (multiples of 4 that are
    and are not multiples of 16): the source of a destination line lies at every byte alignment;
  * lengths 0..49 (shorter than head + one line + tail), 1008..1040 (round one wavefront access of 64 x 16 bytes),
    COMPACT_GROUP - 17 .. + 17 (round one trip of the unrolled body loop), 65536, and length == stride (the last member
    ends where the slot array ends: nothing to read beyond);
  * neighbours 0..15 bytes apart, so that two members' wavefronts share 16-byte lines: every gap byte stays 0xa5;
  * n = 1, 63, 64, 65 and 24,577 = 3 x 256 CUs x 32 wavefront slots + 1: any persistent grid walks at least three
    rounds, the last one ragged;
  * the same through hipdeflate_compact_span_dev with span_base 2^33 + 3."""
import importlib
import os

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

GROUP = 4096                                   # hd_compact.hpp COMPACT_GROUP (tests/test_compact_isa.py holds it to the header)
STRIDES = [20, 84, 4116, 65536]
SLOT_DELTAS = [0, 4, 8, 12]
LENGTHS = (list(range(0, 50)) + list(range(1008, 1041)) + list(range(GROUP - 17, GROUP + 18)) + [65536])
SPAN_BASE = 2 ** 33 + 3
LEAD, TRAIL = 32, 64                           # 0xa5 bytes in front of the first member and behind the last
GRID_N = [1, 63, 64, 65, 3 * 256 * 32 + 1]


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
def pool():
    """random bytes every case cuts its slot array from (made once)"""
    n = max(len([L for L in LENGTHS if L <= s] + [s]) * 16 * s for s in STRIDES)
    return np.frombuffer(np.random.default_rng(20260101).bytes(n), dtype=np.uint8).copy()


def lengths_for(stride):
    return sorted(set([L for L in LENGTHS if L <= stride] + [stride]))


def layout_every_alignment(lengths):
    """every length at every destination alignment 0..15; the gap in front of a member is what its alignment asks,
    0..15 bytes -> [(length, offset)], bytes of the destination.  The LAST member has the greatest length (== stride)."""
    out, pos = [], LEAD
    for L in lengths:
        for a in range(16):
            o = pos + ((a - pos) & 15)
            out.append((L, o))
            pos = o + L
    return out, pos + TRAIL


def layout_random_gaps(lens, seed):
    gaps = np.random.default_rng(seed).integers(0, 16, len(lens))
    out, pos = [], LEAD
    for L, g in zip(lens, gaps):
        out.append((int(L), pos + int(g)))
        pos += int(g) + int(L)
    return out, pos + TRAIL


def run_and_check(pkg, torch, slots, stride, delta, lay, size, span_base, what):
    n = len(lay)
    assert len(slots) == n * stride
    want = np.full(size, 0xa5, dtype=np.uint8)
    for i, (L, o) in enumerate(lay):
        want[o:o + L] = slots[i * stride: i * stride + L]
    d_all = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    assert d_all.data_ptr() % 16 == 0
    d_slots = d_all[delta:delta + n * stride]
    d_slots.copy_(torch.from_numpy(slots))
    d_len = torch.from_numpy(np.array([L for L, _ in lay], dtype=np.uint32).view(np.int32)).cuda()
    d_off = torch.from_numpy(np.array([o + span_base for _, o in lay], dtype=np.uint64).view(np.int64)).cuda()
    d_dst = torch.full((size,), 0xa5, dtype=torch.uint8, device="cuda")
    assert d_dst.data_ptr() % 16 == 0 and d_slots.data_ptr() % 16 == delta
    st = torch.cuda.current_stream().cuda_stream
    if span_base == 0:
        rc = pkg.lib().hipdeflate_compact_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                              d_dst.data_ptr(), st)
    else:
        rc = pkg.lib().hipdeflate_compact_span_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                                   d_dst.data_ptr(), span_base, st)
    assert rc == 0, what
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        inside = [(i, L, o) for i, (L, o) in enumerate(lay) if o <= k < o + L]
        raise AssertionError("%s: byte %d is %#x, not %#x (%s)" % (
            what, k, got[k], want[k], "member %d, length %d at %d" % inside[0] if inside else "a gap byte"))


def test_layout_is_the_stated_one():
    for s in STRIDES:
        lens = lengths_for(s)
        lay, size = layout_every_alignment(lens)
        assert lens[-1] == s and lay[-1][0] == s
        ends = [LEAD] + [o + L for L, o in lay]
        assert set(o - e for (L, o), e in zip(lay, ends)) <= set(range(16))
        for L in lens:
            assert sorted(o & 15 for l2, o in lay if l2 == L) == list(range(16))
        assert size == ends[-1] + TRAIL
    assert lengths_for(20) == list(range(21))
    assert set(range(GROUP - 17, GROUP + 18)) <= set(lengths_for(4116)) and 4116 in lengths_for(4116)
    assert {1008, 1024, 1040, 65536} <= set(lengths_for(65536))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("delta", SLOT_DELTAS)
@pytest.mark.parametrize("stride", STRIDES)
def test_every_alignment_length_stride_and_slot_base(pkg, torch, pool, stride, delta):
    lay, size = layout_every_alignment(lengths_for(stride))
    run_and_check(pkg, torch, pool[:len(lay) * stride], stride, delta, lay, size, 0, ("stride", stride, "slots +", delta))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("stride,delta", [(84, 12), (4116, 4), (65536, 8)])
def test_every_alignment_through_the_span_call(pkg, torch, pool, stride, delta):
    lay, size = layout_every_alignment(lengths_for(stride))
    run_and_check(pkg, torch, pool[:len(lay) * stride], stride, delta, lay, size, SPAN_BASE,
                  ("span", stride, "slots +", delta))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("span_base", [0, SPAN_BASE])
def test_neighbours_share_sixteen_byte_lines(pkg, torch, pool, span_base):
    """4,096 members of 0..40 bytes, 0..15 bytes apart: most 16-byte lines of the destination hold the ends of two or
    three members and a gap, and every gap byte is still 0xa5"""
    lens = np.random.default_rng(7).integers(0, 41, 4096)
    lay, size = layout_random_gaps(lens, 8)
    lines = {}
    for L, o in lay:
        for b in range(o >> 4, ((o + L - 1) >> 4) + 1 if L else o >> 4):
            lines[b] = lines.get(b, 0) + 1
    assert sum(1 for v in lines.values() if v >= 2) > 1000
    run_and_check(pkg, torch, pool[:4096 * 84], 84, 4, lay, size, span_base, ("shared lines", span_base))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("span_base", [0, SPAN_BASE])
@pytest.mark.parametrize("n", GRID_N)
def test_grid_edges(pkg, torch, pool, n, span_base):
    """members of 0..100 bytes in slots of 100: one member, a wavefront's worth and one more, and more members than
    three rounds of any persistent grid"""
    lens = np.random.default_rng(n).integers(0, 101, n)
    lay, size = layout_random_gaps(lens, n + 1)
    run_and_check(pkg, torch, pool[:n * 100], 100, 0, lay, size, span_base, ("n", n, span_base))
