"""The gather on the small grid (hd_compact.hpp COMPACT_BESIDE_WAVES_PER_2CU) and the rule that picks it
(hd_api.hip compact_beside): a gather launched while an encode of the library's own is still queued or
running in another stream, into other slots, gets fewer wavefronts -- the same kernel, the same bytes.

  1. the small grid copies right: 3 x grid + 5 members, so that every wavefront takes three or four of them (wavefront w
     takes members w, w + grid, ...), every length round the kernel's edges at destination offsets of every alignment
     mod 16, both entry points, against a byte-by-byte numpy placement into a destination pre-filled with 0xa5;
  2. the decision, case by case, read back through hipdeflate_test_compact_grid();
  3. bench.py's pipeline (tools/gather_beside.py, leg 2) in small: `auto` and `full` write the same bytes, and under
     `auto` every gather but the drained one runs on the small grid.

Cases 2 and 3 ask the library what it saw on the host at the launch of the gather; the encode they launch in front of it
(1 GiB: about 3 ms; 0.25 GiB: about 0.7 ms behind another one) outlasts the few host calls in between by far (some 40
microseconds), once every kernel and every stream involved has been used before: the first launch into a new stream
costs the host several milliseconds, more than the encode takes."""
import importlib
import os
import sys

import numpy as np
import pytest

import hdtest

pytestmark = pytest.mark.gpu

BLOCK = 0xff00
SPAN_BASE = 2 ** 33 + 3
GUARD = 64                                     # 0xa5 bytes in front of the first member and behind the last
STRIDES = [4112, 65536]
LENGTHS = [0, 1, 15, 16, 17] + list(range(4096 - 17, 4096 + 18)) + [65536]     # (4079..4081 are the first of the range)
ENCODE_WAVES_PER_CU = 21                       # level-1 wavefronts a CU holds (hd_api.hip ENCODE_L1_WAVES_PER_CU)
FULL_WAVES_PER_CU = 3                          # hd_compact.hpp COMPACT_WAVES_PER_CU


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
def dev(pkg):
    return importlib.import_module("7bgzf_amd.device")


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def hook(pkg):
    return int(pkg.lib().hipdeflate_test_compact_grid())


@pytest.fixture(scope="module")
def small_grid(pkg, torch, cus):
    """the small grid of this build on this device, as a forced launch of more members than the full grid reports it"""
    n = cus * FULL_WAVES_PER_CU + 1
    d_slots = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_dst = torch.zeros(16, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    old = os.environ.get("HIPDEFLATE_GATHER_GRID")
    grids = {}
    try:
        for mode in ("beside", "full"):
            os.environ["HIPDEFLATE_GATHER_GRID"] = mode
            assert pkg.lib().hipdeflate_compact_dev(d_slots.data_ptr(), 16, d_len.data_ptr(), d_off.data_ptr(), n,
                                                    d_dst.data_ptr(), st) == 0
            grids[mode] = hook(pkg)
    finally:
        if old is None:
            del os.environ["HIPDEFLATE_GATHER_GRID"]
        else:
            os.environ["HIPDEFLATE_GATHER_GRID"] = old
    torch.cuda.synchronize()
    assert grids["full"] == cus * FULL_WAVES_PER_CU
    assert 1 <= grids["beside"] < grids["full"]
    return grids["beside"]


# ---- 1. the small grid copies right -------------------------------------------------------------------------------

def lengths_for(stride):
    return [L for L in LENGTHS if L < stride] + [stride]


def layout(n, stride):
    """member i: the i-th length of the cycle, at a destination offset whose alignment mod 16 moves on by one from
    member to member and by one more with every turn of the cycle -> [(length, offset)], bytes of the destination"""
    lens = lengths_for(stride)
    out, pos = [], GUARD
    for i in range(n):
        a = (i + i // len(lens)) & 15
        o = pos + ((a - pos) & 15)
        L = lens[i % len(lens)]
        out.append((L, o))
        pos = o + L
    return out, pos + GUARD


def test_layout_is_the_stated_one():
    for stride in STRIDES:
        lens = lengths_for(stride)
        assert stride in lens and max(lens) == stride and {0, 1, 15, 16, 17, 4079, 4080, 4081} <= set(lens)
        assert len(set(lens)) == len(lens)
        assert set(range(4096 - 17, min(4096 + 18, stride))) <= set(lens)
        lay, size = layout(3 * 128 + 5, stride)
        assert set(o & 15 for _, o in lay) == set(range(16))
        assert set(L for L, _ in lay) == set(lens)
        assert lay[0][1] >= GUARD and size == lay[-1][0] + lay[-1][1] + GUARD
        ends = [GUARD] + [o + L for L, o in lay]
        assert all(0 <= o - e < 16 for (L, o), e in zip(lay, ends))
    assert 65536 in lengths_for(65536) and 4096 + 17 in lengths_for(65536)


@pytest.mark.parametrize("span_base", [0, SPAN_BASE])
@pytest.mark.parametrize("stride", STRIDES)
def test_small_grid_copies_right(pkg, torch, small_grid, monkeypatch, stride, span_base):
    monkeypatch.setenv("HIPDEFLATE_GATHER_GRID", "beside")
    n = 3 * small_grid + 5
    lay, size = layout(n, stride)
    slots = np.frombuffer(np.random.default_rng(stride).bytes(n * stride), dtype=np.uint8)
    want = np.full(size, 0xa5, dtype=np.uint8)
    for i, (L, o) in enumerate(lay):
        want[o:o + L] = slots[i * stride: i * stride + L]
    d_slots = torch.from_numpy(slots.copy()).cuda()
    d_len = torch.from_numpy(np.array([L for L, _ in lay], dtype=np.uint32).view(np.int32)).cuda()
    d_off = torch.from_numpy(np.array([o + span_base for _, o in lay], dtype=np.uint64).view(np.int64)).cuda()
    d_dst = torch.full((size,), 0xa5, dtype=torch.uint8, device="cuda")
    assert d_dst.data_ptr() % 16 == 0 and d_slots.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    if span_base == 0:
        rc = pkg.lib().hipdeflate_compact_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                              d_dst.data_ptr(), st)
    else:
        rc = pkg.lib().hipdeflate_compact_span_dev(d_slots.data_ptr(), stride, d_len.data_ptr(), d_off.data_ptr(), n,
                                                   d_dst.data_ptr(), span_base, st)
    assert rc == 0
    assert hook(pkg) == small_grid
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got[:GUARD], want[:GUARD]) and np.array_equal(got[-GUARD:], want[-GUARD:]), "guard bytes"
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        inside = [(i, L, o) for i, (L, o) in enumerate(lay) if o <= k < o + L]
        raise AssertionError("stride %d, span_base %d: byte %d is %#x, not %#x (%s)" % (
            stride, span_base, k, got[k], want[k], "member %d, length %d at %d" % inside[0] if inside else "a gap byte"))


# ---- 2. the decision ----------------------------------------------------------------------------------------------

def packed_reference(torch, enc):
    """what the gather of enc's members must write, made with torch indexing from the slots (enc scanned, base 0)"""
    total = int(enc.total.item())
    pos = torch.arange(total, dtype=torch.int64, device="cuda")
    member = torch.searchsorted(enc.dst_off, pos, right=True) - 1
    return enc.slots[member * enc.slot + (pos - enc.dst_off[member])]


class Decision:
    """1 GiB of FASTQ-like blocks, two sets of slots: A is what the encode of a case fills on stream a, B holds the same
    members from an encode long finished ("other slots")"""
    NB = 16384

    def __init__(self, pkg, torch, dev):
        self.pkg, self.torch, self.dev = pkg, torch, dev
        tile = hdtest.synth().fastq_like(16 << 20, seed=77, first_record=100_000_000)
        reps = -(-self.NB * BLOCK // len(tile))
        self.data = torch.from_numpy(tile).cuda().repeat(reps)[:self.NB * BLOCK].contiguous()
        self.off, self.ln = dev.block_table(self.NB * BLOCK, BLOCK)
        self.A, self.B = dev.DeviceDeflate(self.NB), dev.DeviceDeflate(self.NB)
        self.a, self.b = torch.cuda.Stream(), torch.cuda.Stream()
        for level in (0, 1):                                   # level 1 last: both sets hold its members afterwards
            for enc in (self.A, self.B):
                enc.run(self.data, self.off, self.ln, level=level)
                enc.scan()
            torch.cuda.synchronize()
            assert int(self.A.status.abs().sum()) == 0 and int(self.B.status.abs().sum()) == 0
        self.ref = packed_reference(torch, self.A)             # made once: every case packs these bytes
        assert torch.equal(self.ref, packed_reference(torch, self.B))
        self.pack = torch.empty(self.ref.numel() + 2 * GUARD, dtype=torch.uint8, device="cuda")
        # every kernel and both streams of a case have run once: nothing is loaded or created between a case's encode and
        # its gather
        self.encode(nb=256)
        with torch.cuda.stream(self.b):
            self.B.compact(self.pack[GUARD:])
        torch.cuda.synchronize()

    def encode(self, level=1, nb=None):
        """on stream a, into A"""
        nb = self.NB if nb is None else nb
        self.pack.fill_(0xa5)
        self.torch.cuda.synchronize()
        with self.torch.cuda.stream(self.a):
            rc = self.pkg.lib().hipdeflate_batch_deflate_dev(
                self.data.data_ptr(), self.off.data_ptr(), self.ln.data_ptr(), nb, level, self.pkg.FRAME_BGZF,
                self.A.slots.data_ptr(), self.A.slot, self.A.slot, self.A.out_len.data_ptr(), self.A.crc.data_ptr(),
                self.A.status.data_ptr(), self.a.cuda_stream)
        assert rc == 0

    def gather(self, enc, stream):
        """enc's members on `stream` -> the grid the library chose; the packed bytes and the guards are checked"""
        torch = self.torch
        with torch.cuda.stream(stream):
            enc.compact(self.pack[GUARD:])
        grid = hook(self.pkg)
        torch.cuda.synchronize()
        ref = self.ref
        assert torch.equal(self.pack[GUARD:GUARD + ref.numel()], ref)
        assert bool((self.pack[:GUARD] == 0xa5).all()) and bool((self.pack[GUARD + ref.numel():] == 0xa5).all())
        return grid


@pytest.fixture(scope="module")
def decision(pkg, torch, dev, small_grid):
    return Decision(pkg, torch, dev)


def test_decision_other_slots_in_another_stream_get_the_small_grid(decision, small_grid, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    assert decision.NB >= cus * ENCODE_WAVES_PER_CU
    decision.encode()
    assert decision.gather(decision.B, decision.b) == small_grid


def test_decision_same_stream_is_full(decision, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    decision.encode()
    assert decision.gather(decision.B, decision.a) == cus * FULL_WAVES_PER_CU


def test_decision_own_slots_behind_an_event_is_full(decision, torch, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    decision.encode()
    done = torch.cuda.Event()
    done.record(decision.a)
    decision.b.wait_event(done)
    with torch.cuda.stream(decision.b):
        decision.A.scan()
    assert decision.gather(decision.A, decision.b) == cus * FULL_WAVES_PER_CU


def test_decision_after_a_device_synchronise_is_full(decision, torch, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    decision.encode()
    torch.cuda.synchronize()
    assert decision.gather(decision.B, decision.b) == cus * FULL_WAVES_PER_CU


def test_decision_level_0_is_full(decision, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    decision.encode(level=0)
    assert decision.gather(decision.B, decision.b) == cus * FULL_WAVES_PER_CU


def test_decision_256_blocks_is_full(decision, cus, monkeypatch):
    monkeypatch.delenv("HIPDEFLATE_GATHER_GRID", raising=False)
    decision.encode(nb=256)
    assert decision.gather(decision.B, decision.b) == cus * FULL_WAVES_PER_CU


def test_decision_switched_off_is_full(decision, cus, monkeypatch):
    monkeypatch.setenv("HIPDEFLATE_GATHER_GRID", "full")
    decision.encode()
    assert decision.gather(decision.B, decision.b) == cus * FULL_WAVES_PER_CU


# ---- 3. bench.py's pipeline in small ------------------------------------------------------------------------------

def test_pipeline_auto_and_full_write_the_same_stream(pkg, torch, dev, small_grid, cus, monkeypatch):
    """two buffer sets, four steps, 0.25 GiB a pass.  In blocks of 32 KiB: 8,192 of them, where blocks of 0xff00 bytes
    would be 4,113, fewer than the 21 wavefronts x 256 CUs the rule wants of an encode before it counts as running
    beside anything."""
    tools = os.path.join(hdtest.ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    gb = importlib.import_module("gather_beside")
    block, nb = 32768, 8192
    assert nb >= cus * ENCODE_WAVES_PER_CU
    tile = hdtest.synth().fastq_like(16 << 20, seed=78, first_record=100_000_000)
    data = torch.from_numpy(tile).cuda().repeat(16).contiguous()
    assert data.numel() == nb * block
    off, ln = dev.block_table(nb * block, block)
    encs = [dev.DeviceDeflate(nb), dev.DeviceDeflate(nb)]
    packs = [torch.zeros(nb * block, dtype=torch.uint8, device="cuda") for _ in range(2)]
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    full = cus * FULL_WAVES_PER_CU

    def run(mode):
        monkeypatch.setenv("HIPDEFLATE_GATHER_GRID", mode)
        for p in packs:
            p.zero_()
        torch.cuda.synchronize()
        grids = []
        step, drain = gb.pipeline(torch, main, side, encs, packs, lambda i: encs[i].run(data, off, ln, level=1),
                                  after_gather=lambda i: grids.append(hook(pkg)))
        for _ in range(4):
            step([], [])
        drain([])
        torch.cuda.synchronize()
        assert all(int(e.status.abs().sum()) == 0 for e in encs)
        return grids, [(e.dst_off.clone(), int(e.total.item()), p.clone()) for e, p in zip(encs, packs)]

    run("full")                                                # (every kernel has run once)
    g_full, r_full = run("full")
    g_auto, r_auto = run("auto")
    assert g_full == [full] * 4
    assert g_auto == [small_grid] * 3 + [full]                 # steps 2..4, then the drained one
    for (o1, t1, p1), (o2, t2, p2) in zip(r_full, r_auto):
        assert t1 == t2 > 0 and torch.equal(o1, o2) and torch.equal(p1, p2)
    # ... and the stream is the members in order
    assert torch.equal(r_auto[1][2][:r_auto[1][1]], packed_reference(torch, encs[1]))
