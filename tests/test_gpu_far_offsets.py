"""Every device path of include/hipdeflate.h with data really AT offsets of 2^32 and more: inputs, outputs, slots, scratch
records, table entries.  The technique (tests/far_offsets.py, pinned by tests/test_far_offsets.py): big buffers are never
filled -- small blocks sit at the edge offsets (ending at 2^32, straddling it, starting at it, 2^32 + 1, 2^32 + 2^31 + 7,
the buffer's end), the tables point at them in shuffled order with low-offset controls among them; sentinels guard both
ends of every far output and its alias at X - 2^32; containers and streams past 4 GiB are a tile repeated on the device
and compared repeat by repeat.  Bit-exact, no tolerances.  No case provokes a fault: every offset lies inside its
buffer, every refused input is a case the header defines.

Which test holds which 64-bit quantity to a value >= 2^32 whose bytes are at that address:
  in_off of the encode        test_encode_far_input_and_far_output (blocks at every edge of a 6.06 GiB input)
  i * out_stride              the same (stride 256 MiB + 16: rows 16..23), test_rows_times_stride (rows 4096..4199 of 1 MiB)
  scratch record offset       test_scratch_records_past_4gib (levels 2 and 6; the arithmetic is in its docstring)
  dst_off, span_base          test_scan_and_gather_at_far_addresses (slots and destination past 2^32, base 2^40 + 5)
  in_off / out_off of the     test_inflate_far_input_and_far_output
  inflate
  a member's header address,  test_members_far_input_and_far_output (tests/far_framed.py: raw, zlib and gzip members at every
  the payload table (p_off),  edge of a 6.06 GiB input -- a name scanned across 2^32, header and payload 64 KiB apart at 2^32, a
  the trailer's address       gzip trailer cut 4 | 4 and a zlib trailer cut 2 | 2 by 2^32, refused members on far rows)
  p_off + used, in_used,
  out_off of the framed       the same (outputs at ANOTHER edge of a 6.06 GiB output, one of 300,000 bytes read back from HBM at
  decode, the Adler pass      a far out_off; zlib members: k_chunk_adler over out + out_off); in_off + in_used as a 64-bit tensor
  the host forms' host        test_host_forms_with_far_host_offsets
  offsets
  index pos / in_off /        test_index_and_run_on_a_container_past_4gib, test_ranged_reads_past_4gib (also a virtual
  end_offset / out_bytes,     offset's coffset and a range's dst_off)
  chunk_off, the stream's     test_one_stream_past_4gib
  in_bytes / out_bytes, ISIZE
  the 32-bit counters of one  test_inflate_input_of_max_in, test_inflate_output_past_2_31 (and its 128 MiB form, which the
  inflate (bit position, out) oracle can still follow: test_inflate_output_of_128_mib)
  the size pass's bit         test_size_pass_input_of_max_in (stored-block seeks up to bit 2^31, ISIZE read at src + used + 4),
  position, `used` near 2^28  test_framed_decode_input_of_max_in (in_used and the trailer's address at 2^28 - 1)
  inflate_members' prefix     test_inflate_members_prefix_sum_past_4gib (out_off up to 2^32 + 64 MiB + 70,100 from the scan,
  sum                         a member that straddles 2^32, a refused member with and without room)

Every test asserts the free device memory it needs before it allocates (it fails, never skips) and frees its buffers."""
import ctypes
import gc
import importlib
import os
import zlib

import numpy as np
import pytest

import encode_room as er
import far_framed as ff
import far_offsets as fo
import framed_model as fm
import hdtest
import member_index_model as mm
import range_read_model as rm
import stream_model as sm

pytestmark = pytest.mark.gpu

P32 = fo.P32
BIG = P32 + (1 << 31) + (64 << 20)                   # the sparse buffers: edge offsets up to 2^32 + 2^31 + 64 MiB
SENT = fo.SENT
GIB = 1 << 30
SEG_LIMIT = er.SEG_LIMIT


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


def need_room(torch, nbytes):
    """assert that the device has nbytes free: a full device FAILS the test, a skip would hide the gap"""
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert nbytes <= 16 * GIB + (1 << 29), "a test of this file stays under about 16 GiB"
    assert free >= nbytes + GIB, "needs %.1f GiB of device memory, %.1f are free" % (nbytes / GIB, free / GIB)


@pytest.fixture
def room(torch):
    """room(nbytes) = need_room; everything is handed back to the device behind the test"""
    yield lambda nbytes: need_room(torch, nbytes)
    gc.collect()
    torch.cuda.empty_cache()


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def put(torch, mem, offset, data):
    if len(data):
        mem[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def u64(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64).copy()).cuda()


def u32(torch, values):
    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32).copy()).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64).tolist()


def empty(torch, n):
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


_corpus = {}


def corpus():
    """the block kinds, made once: text, FASTQ-like, noise, zeros"""
    if not _corpus:
        s = hdtest.synth()
        _corpus.update(text=bytes(s.text_like(400000, seed=41)), fastq=bytes(s.fastq_like(400000, seed=42)),
                       noise=bytes(s.random_bytes(70000, seed=43)), zeros=bytes(70000))
    return _corpus


_models = {}


def model(data, level):
    k = (hdtest.sha(data), level)
    if k not in _models:
        _models[k] = er.Block(data, level, False)
    return _models[k]


# ---- A. batch encode: far input, far output ---------------------------------------------------------------------------

A_STRIDE = (256 << 20) + 16
A_ROWS = 24
A_CAP = 1 << 20
ZONE_AT = P32 - 163841                               # the HD_SEG_LIMIT + 1 block: straddles 2^32, starts unaligned


def encode_layout():
    """-> (writes: [(offset, bytes)] of the input buffer, rows: [(in_off, in_len)] in OUTPUT order).  The four blocks
    that touch 2^32 are windows of one zone of HD_SEG_LIMIT + 1 bytes around it (text below 2^32, FASTQ-like above), which
    is a block of its own too: its segments read across 2^32.  Rows 0..7 give members of at most 256 bytes: rows 16..23
    lie 2^32 + 256 behind them, so their aliases stay clear of every member."""
    c = corpus()
    zone = c["text"][:P32 - ZONE_AT] + c["fastq"][:SEG_LIMIT + 1 - (P32 - ZONE_AT)]
    assert len(zone) == SEG_LIMIT + 1
    high = fo.place(BIG, [("high", 0xff00), ("high", 0xff00), ("high", 20000), ("high", 5), ("end", 0xff00), ("end", 150),
                          ("low", 0xff00), ("low", 0xff00), ("low", 5), ("low", 200), ("low", 1000), ("low", 100)])
    datas = [c["noise"][:0xff00], c["zeros"][:0xff00], c["text"][1000:21000], b"far!\n", c["fastq"][7:7 + 0xff00],
             c["noise"][300:450], c["text"][:0xff00], c["noise"][3:3 + 0xff00], b"tiny\0", c["noise"][:200], c["zeros"][:1000],
             c["text"][:100]]
    writes = [(ZONE_AT, zone)] + [(r.offset, d) for r, d in zip(high, datas)]
    h_noise, h_zeros, h_text, h_five, e_fastq, e_noise, l_text, l_noise, l_five, l_n200, l_z1000, l_t100 = \
        [(r.offset, r.length) for r in high]
    ends_at = (P32 - 0xff00, 0xff00)
    straddle = (P32 - fo.STRADDLE, 30000)
    starts_at = (P32, 0xff00)
    plus1 = (P32 + 1, 5)
    whole = (ZONE_AT, SEG_LIMIT + 1)
    rows = [l_five, plus1, l_n200, h_five, l_z1000, l_t100, e_noise, l_z1000,
            l_text, ends_at, h_noise, whole, l_noise, starts_at, e_fastq, h_zeros,
            straddle, l_text, h_text, whole, starts_at, ends_at, e_fastq, h_noise]
    assert len(rows) == A_ROWS
    return writes, rows


def read_back(writes, off, n):
    for at, d in writes:
        if at <= off and off + n <= at + len(d):
            return d[off - at:off - at + n]
    raise AssertionError("no block at %d" % off)


A_CASES = [(lv, f, False) for lv in (1, 2, 6) for f in (er.RAW, er.BGZF, er.ZLIB, er.MIGZ)] + [(lv, er.RAW, True) for lv in (1, 2, 6)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level,frame,latency", A_CASES,
                         ids=["l%d-%s%s" % (lv, er.FRAME_NAMES[f], "-latency" if lat else "") for lv, f, lat in A_CASES])
def test_encode_far_input_and_far_output(pkg, torch, room, level, frame, latency):
    """hipdeflate_batch_deflate_dev: blocks at every edge offset of a 6.06 GiB input, members at i * (256 MiB + 16) -- past
    2^32 from row 16 on.  Every member, out_len, crc and status is the twin's; the guards at both ends of every far room and
    at the alias of every far member are intact."""
    room(BIG + A_ROWS * A_STRIDE)
    stalls = pkg.lib().hipdeflate_stall_count()
    writes, rows = encode_layout()
    datas = [read_back(writes, o, n) for o, n in rows]
    payload_room = er.payload_room(frame, A_STRIDE, A_CAP)
    wants = [model(d, level).choose(payload_room, latency, device=True) for d in datas]
    members = [er.frame_member(frame, w.member, d) if w.fits else None for w, d in zip(wants, datas)]
    assert all(m is not None and len(m) <= 256 for m in members[:8])
    assert sum(o >= P32 for o, _ in rows) >= 10 and any(o < P32 < o + n for o, n in rows)

    src = empty(torch, BIG)
    in_regs = fo.regions([(o, len(d)) for o, d in writes], BIG, ends=False)         # a narrowed in_off reads sentinels
    fo.fill(src, in_regs)
    for at, d in writes:
        put(torch, src, at, d)
    out = empty(torch, A_ROWS * A_STRIDE)
    slot = [i * A_STRIDE for i in range(A_ROWS)]
    assert slot[16] == P32 + 256
    # the guards at the ends belong to the ROOMS (an encoder may use all of its room), the aliases to the far members;
    # the first 256 bytes of rows 0..7 are theirs
    regs = fo.regions([(s, A_CAP) for s in slot], out.numel(), alias=False) + \
        fo.regions([(s, len(m) if m is not None else 0) for s, m in zip(slot, members)][8:], out.numel(), ends=False,
                   others=[(s, 256) for s in slot[:8]])
    for s in slot:                                    # (no stale members of an earlier case where this one must write)
        out[s:s + A_CAP] = 0
    fo.fill(out, regs)
    olen = torch.zeros(A_ROWS, dtype=torch.int32, device="cuda")
    crc = torch.zeros(A_ROWS, dtype=torch.int32, device="cuda")
    st = torch.full((A_ROWS,), -7, dtype=torch.int32, device="cuda")
    in_off, in_len = u64(torch, [o for o, _ in rows]), u32(torch, [n for _, n in rows])       # (named: they must outlive the launch)
    rc = pkg.lib().hipdeflate_batch_deflate_dev(
        vp(src), vp(in_off), vp(in_len), A_ROWS, level,
        frame | (er.LATENCY if latency else 0), vp(out), A_STRIDE, A_CAP, vp(olen), vp(crc), vp(st), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0 if w.fits else 1 for w in wants]
    fits = [i for i, w in enumerate(wants) if w.fits]
    assert len(fits) >= 20 and [host_u32(olen)[i] for i in fits] == [len(members[i]) for i in fits]
    assert [host_u32(crc)[i] for i in fits] == [zlib.crc32(datas[i]) for i in fits]
    assert fo.check_rows(out, [(slot[i], members[i]) for i in fits], regs) == []
    assert fo.intact(in_regs, src)
    assert pkg.lib().hipdeflate_stall_count() == stalls
    del src, out


# ---- B. many rows: i * out_stride and the scratch records past 2^32 ---------------------------------------------------

B_ROWS, B_STRIDE, B_CAP, B_DISTINCT = 4200, 1 << 20, 96 << 10, 32


def distinct_blocks(count, longest=65536):
    """`count` blocks of 5 .. `longest` bytes of the four kinds, no two alike"""
    c = corpus()
    rng = np.random.default_rng(77)
    out = []
    for k in range(count):
        kind = ("text", "fastq", "zeros", "noise")[k % 4]
        n = [5, longest, 0xff00, 777][k] if k < 4 else int(rng.integers(100, 8192 if kind == "noise" else longest + 1))
        at = int(rng.integers(0, len(c[kind]) - n))
        out.append(c[kind][at:at + n] if kind != "zeros" else bytes(n))
    assert len(set(out)) == count
    return out


def which_block(i, distinct):
    """the block of row i: rows i and i + 4096 (whose slots lie exactly 2^32 apart) never share one"""
    return (i + i // 4096) % distinct


def pack_blocks(torch, blocks):
    blob, offs = bytearray(), []
    for i, d in enumerate(blocks):
        blob += bytes((-len(blob) % 16) + (i % 3))
        offs.append(len(blob))
        blob += d
    return torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda(), offs


def encode_aliased_rows(pkg, torch, blocks, nrows, level, stride, cap, out):
    """nrows rows over the distinct blocks -> (out_len, crc, status) device tensors"""
    src, offs = pack_blocks(torch, blocks)
    pick = [which_block(i, len(blocks)) for i in range(nrows)]
    olen = torch.zeros(nrows, dtype=torch.int32, device="cuda")
    crc = torch.zeros(nrows, dtype=torch.int32, device="cuda")
    st = torch.full((nrows,), -7, dtype=torch.int32, device="cuda")
    in_off, in_len = u64(torch, [offs[k] for k in pick]), u32(torch, [len(blocks[k]) for k in pick])      # (they outlive the launch)
    rc = pkg.lib().hipdeflate_batch_deflate_dev(
        vp(src), vp(in_off), vp(in_len), nrows, level, er.RAW,
        vp(out), stride, cap, vp(olen), vp(crc), vp(st), None)
    assert rc == 0
    torch.cuda.synchronize()
    return olen, crc, st, pick


def check_aliased_rows(torch, blocks, members, out, nrows, stride, cap, olen, crc, st, pick, filled):
    assert not st.cpu().numpy().any()
    assert host_u32(olen) == [len(members[k]) for k in pick]
    assert host_u32(crc) == [zlib.crc32(blocks[k]) for k in pick]
    view = out[:nrows * stride].view(nrows, stride)
    pick_t = torch.tensor(pick, device="cuda")
    bad = []
    for k, m in enumerate(members):                                       # on the device, against the uploaded members
        rows_k = torch.nonzero(pick_t == k).flatten()
        want = torch.from_numpy(np.frombuffer(m, dtype=np.uint8).copy()).cuda()
        same = (view[rows_k, :len(m)] == want[None, :]).all(dim=1)
        bad += [(int(r), k) for r in rows_k[~same].tolist()]
    assert bad == [], bad[:10]
    if filled:                                                            # nothing behind any room: the slots' tails
        room_end = (cap + 3) & ~3
        for a in range(0, nrows, 512):
            assert bool((view[a:a + 512, room_end:] == SENT).all()), ("behind the room of rows", a)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level", [1, 6])
def test_rows_times_stride(pkg, torch, room, level):
    """4,200 rows of 1 MiB stride over 32 distinct blocks: rows 4096.. lie past 2^32, exactly 2^32 behind rows 0.. (which
    hold OTHER blocks).  Every row is its block's twin; every byte behind every room (96 KiB) still holds the sentinel the
    whole 4.1 GiB were filled with."""
    room(B_ROWS * B_STRIDE + GIB)
    stalls = pkg.lib().hipdeflate_stall_count()
    blocks = distinct_blocks(B_DISTINCT)
    members = []
    for d in blocks:
        r, m = hdtest.oracle_twin(d, level, cap=B_CAP)
        assert r == 0
        members.append(m)
    out = empty(torch, B_ROWS * B_STRIDE)
    out.fill_(SENT)
    assert (B_ROWS - 1) * B_STRIDE > P32
    got = encode_aliased_rows(pkg, torch, blocks, B_ROWS, level, B_STRIDE, B_CAP, out)
    check_aliased_rows(torch, blocks, members, out, B_ROWS, B_STRIDE, B_CAP, *got, filled=True)
    assert pkg.lib().hipdeflate_stall_count() == stalls
    del out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level", [2, 6])
def test_scratch_records_past_4gib(pkg, torch, room, level):
    """The records a launch keeps per block between its parse and its emit (hd_deflate_dynamic.hpp): a region of
    sub x layout.bytes behind the overflow flags, sub = the blocks of a sub-batch, block j's record at j * layout.bytes.
      level 6 (wg_scratch_bytes): layout = 4 B per input byte of the slot + the pieces' records; sub = min(17408 MiB /
        layout, 65536, nblocks).  Slots of hipdeflate_bound(0xff00) = 65.6 KiB: layout ~ 263 KiB, the cap on sub is 65536,
        so the region passes 2^32 from about 16,350 blocks on and reaches 16.4 GiB.
      level 2 (dynamic_scratch_bytes): layout = the split path's tokens and histograms, 3 B per byte of the slot + 4 KiB
        ~ 201 KiB; sub = min(12672 MiB / layout, 65536) in whole rounds of 4608 resident waves = 64512, or nblocks if
        that is less -- past 2^32 from about 21,400 blocks on.
    So neither level's sub-batch cap keeps the records below 2^32, and both run here: 24,000 rows over 64 distinct
    0xff00-byte blocks.  The test does not restate the layouts: it reads hipdeflate_scratch_bytes -- total past 2^32,
    growing by one record for one more block (the sub-batch is not the cap yet), and the LAST row's record offset, rows - 1
    records, past 2^32 -- and holds every row to the twin."""
    rows, n = 24000, 0xff00
    L = pkg.lib()
    slot = int(L.hipdeflate_bound(n, level))
    scratch = int(L.hipdeflate_scratch_bytes(rows, slot, level))
    record = scratch - int(L.hipdeflate_scratch_bytes(rows - 1, slot, level))
    print("level %d: slot %d, scratch %d bytes for %d rows, %d per row" % (level, slot, scratch, rows, record))
    assert scratch > P32 and record >= 2 * n, "the records of %d rows stay below 2^32: choose more rows" % rows
    assert (rows - 1) * (record - 256) > P32                 # (256: what a row adds outside its record -- flags, a flag line)
    room(scratch + rows * slot + GIB)
    stalls = L.hipdeflate_stall_count()
    c = corpus()
    blocks = [(c["text"], c["fastq"])[k & 1][k * 3001:k * 3001 + n] for k in range(64)]
    assert len(set(blocks)) == 64
    members = []
    for d in blocks:
        r, m = hdtest.oracle_twin(d, level, cap=slot)
        assert r == 0
        members.append(m)
    out = empty(torch, rows * slot)
    out.zero_()
    got = encode_aliased_rows(pkg, torch, blocks, rows, level, slot, slot, out)
    check_aliased_rows(torch, blocks, members, out, rows, slot, slot, *got, filled=False)
    assert L.hipdeflate_stall_count() == stalls
    del out


# ---- C. scan and gather at far addresses ------------------------------------------------------------------------------

@pytest.mark.timeout(300)
def test_scan_and_gather_at_far_addresses(pkg, torch, room):
    """hipdeflate_scan_sizes_dev, hipdeflate_compact_dev, hipdeflate_compact_span_dev on the slots of test_rows_times_stride
    (level 1): slots at i * stride past 2^32, and a destination of 2^32 + 64 MiB in which the members start at 2^32 - 8 MiB
    - 3 (the scan's base) and run on past 2^32; then the same through a span whose span_base is 2^40 + 5.  Held to a
    byte-by-byte placement: dst_off, total, every member's bytes, the guards around the run and its alias at the
    destination's start."""
    dst_size = P32 + (64 << 20)
    room(B_ROWS * B_STRIDE + dst_size + GIB)
    L = pkg.lib()
    blocks = distinct_blocks(B_DISTINCT, longest=24000)
    members = []
    for d in blocks:
        r, m = hdtest.oracle_twin(d, 1, cap=B_CAP)
        assert r == 0
        members.append(m)
    slots = empty(torch, B_ROWS * B_STRIDE)
    slots.zero_()
    olen, crc, st, pick = encode_aliased_rows(pkg, torch, blocks, B_ROWS, 1, B_STRIDE, B_CAP, slots)
    check_aliased_rows(torch, blocks, members, slots, B_ROWS, B_STRIDE, B_CAP, olen, crc, st, pick, filled=False)
    lens = np.array([len(members[k]) for k in pick], dtype=np.uint64)
    total = int(lens.sum())
    first = P32 - (8 << 20) - 3
    assert first + total + fo.GUARD <= dst_size and first + total > P32 + (8 << 20)
    run = b"".join(members[k] for k in pick)
    regs = fo.regions([(first, total)], dst_size)
    dst = empty(torch, dst_size)
    stream = torch.cuda.current_stream().cuda_stream
    for span_base in (0, 2 ** 40 + 5):
        base = span_base + first
        want_off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens)[:-1]]) + np.uint64(base)
        fo.fill(dst, regs)
        dst[first:first + total] = 0
        d_off = torch.full((B_ROWS + 8,), -3, dtype=torch.int64, device="cuda")
        d_total = torch.full((1,), -3, dtype=torch.int64, device="cuda")
        assert L.hipdeflate_scan_sizes_dev(vp(olen), B_ROWS, base, vp(d_off), vp(d_total), stream) == 0
        if span_base:
            rc = L.hipdeflate_compact_span_dev(vp(slots), B_STRIDE, vp(olen), vp(d_off), B_ROWS, vp(dst), span_base, stream)
        else:
            rc = L.hipdeflate_compact_dev(vp(slots), B_STRIDE, vp(olen), vp(d_off), B_ROWS, vp(dst), stream)
        assert rc == 0
        torch.cuda.synchronize()
        got_off = d_off.cpu().numpy()
        assert fo.check_table(got_off[:B_ROWS].view(np.uint64), want_off, "dst_off") == [] and np.all(got_off[B_ROWS:] == -3)
        assert int(want_off[-1]) - span_base > P32 and int(d_total.item()) == total
        assert fo.check_rows(dst, [(first, run)], regs) == [], span_base
    del slots, dst


# ---- D. batch inflate: far input, far output --------------------------------------------------------------------------

def raw_deflate(data, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    return z.compress(data) + z.flush()


def flushed_chunk(data, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    return z.compress(data) + z.flush(zlib.Z_FULL_FLUSH)


def inflate_streams(flushed):
    """[(stream, contents)]: zlib at levels 0, 1, 6, 9 and the twin, several with more than 64 KiB of output (their match
    sources are read back from output that has left the decoder's ring), a five-byte one, noise"""
    c = corpus()
    plain = [c["text"][:300000], c["fastq"][:200000], c["noise"][:66000], c["text"][5000:5005], c["fastq"][100:100 + 0xff00],
             c["zeros"][:70000], c["text"][70000:70000 + 150000], c["fastq"][200000:200000 + 90000]]
    out = []
    for k, d in enumerate(plain):
        lv = (0, 1, 6, 9)[k % 4]
        out.append(((flushed_chunk if flushed else raw_deflate)(d, lv), d))
    for lv, d in ((1, plain[4]), (2, plain[7][:0xff00]), (6, plain[4]), (1, plain[0][:SEG_LIMIT + 1])):
        r, s = (hdtest.oracle_twin_flush if flushed else hdtest.oracle_twin)(d, lv)
        assert r == 0
        out.append((s, d))
    return out


def inflate_rounds(streams):
    """four launches: in each, one stream at a boundary edge of the input buffer whose output lies at ANOTHER boundary edge of
    the output buffer, and far / low / end rows crossed the other way -> [(stream index, in Row, out Row)] per launch"""
    per, plan_in, plan_out, which = 5, [], [], []
    for r in range(4):
        ks = [(r * per + j) % len(streams) for j in range(per)]
        kin = [fo.BOUNDARY[r], "high", "low", "end", "low"]
        kout = [fo.BOUNDARY[(r + 1) % 4], "low", "high", "end", "high"]
        which += ks
        plan_in += [(k, len(streams[s][0])) for k, s in zip(kin, ks)]
        plan_out += [(k, len(streams[s][1])) for k, s in zip(kout, ks)]
    rin, rout = fo.rounds(BIG, plan_in), fo.rounds(BIG, plan_out)
    assert [len(x) for x in rin] == [len(x) for x in rout] == [per] * 4
    return [[(which[a.index], a, b) for a, b in zip(x, y)] for x, y in zip(rin, rout)]


def run_inflate(pkg, torch, dev, launch, streams, src, out, flushed, short=None):
    """one launch of a round in shuffled table order; short: the position whose out_cap is one below its output.
    -> the problems found"""
    order = list(np.random.default_rng(len(launch) + (short or 0)).permutation(len(launch)))
    launch = [launch[i] for i in order]
    short = None if short is None else order.index(short)
    in_regs = fo.regions([a for _, a, _ in launch], BIG, ends=False)
    fo.fill(src, in_regs)
    for s, a, _ in launch:
        put(torch, src, a.offset, streams[s][0])
    caps = [b.length - (1 if i == short else 0) for i, (_, _, b) in enumerate(launch)]
    regs = fo.regions([(b.offset, cap) for (_, _, b), cap in zip(launch, caps)], BIG)
    fo.fill(out, regs)
    for (_, _, b), cap in zip(launch, caps):          # (no stale bytes of an earlier launch where this one must write)
        out[b.offset:b.offset + cap] = 0
    n = len(launch)
    olen = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    args = (src, u64(torch, [a.offset for _, a, _ in launch]), u32(torch, [a.length for _, a, _ in launch]), out,
            u64(torch, [b.offset for _, _, b in launch]), u32(torch, caps), olen, crc, st)
    if flushed:
        rc = pkg.lib().hipdeflate_batch_inflate_flush_dev(vp(args[0]), vp(args[1]), vp(args[2]), n, *[vp(t) for t in args[3:]],
                                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        dev.device_inflate(*args)
    torch.cuda.synchronize()
    oracle = hdtest.oracle_inflate_flushed if flushed else hdtest.oracle_inflate
    want_st = [oracle(streams[s][0], cap)[0] for (s, _, _), cap in zip(launch, caps)]
    bad = []
    if st.cpu().tolist() != want_st:
        bad.append(("status", st.cpu().tolist(), want_st))
    ok = [i for i in range(n) if want_st[i] == 0]
    if [host_u32(olen)[i] for i in ok] != [launch[i][2].length for i in ok]:
        bad.append(("out_len", host_u32(olen)))
    if [host_u32(crc)[i] for i in ok] != [zlib.crc32(streams[launch[i][0]][1]) for i in ok]:
        bad.append(("crc",))
    bad += fo.check_rows(out, [(launch[i][2].offset, streams[launch[i][0]][1]) for i in ok], regs)
    if not fo.intact(in_regs, src):
        bad.append(("input alias",))
    return bad, want_st


@pytest.mark.timeout(300)
@pytest.mark.parametrize("flushed", [False, True], ids=["final", "flush-form"])
def test_inflate_far_input_and_far_output(pkg, torch, dev, room, flushed):
    """hipdeflate_batch_inflate_dev (through device.device_inflate) and hipdeflate_batch_inflate_flush_dev: streams at the edge
    offsets of a 6.06 GiB input, out_off at the edge offsets of a 6.06 GiB output.  Bytes, out_len, CRC and status are the
    oracle's; with out_cap one short on a far row the verdict is the oracle's and the guard behind the room is intact."""
    room(2 * BIG)
    streams = inflate_streams(flushed)
    launches = inflate_rounds(streams)
    far_in = sum(a.offset >= P32 for l in launches for _, a, _ in l)
    far_out = sum(b.offset >= P32 for l in launches for _, _, b in l)
    assert far_in >= 10 and far_out >= 10 and any(len(streams[s][1]) > 65536 and b.offset >= P32 for l in launches for s, _, b in l)
    src, out = empty(torch, BIG), empty(torch, BIG)
    for launch in launches:
        bad, want_st = run_inflate(pkg, torch, dev, launch, streams, src, out, flushed)
        assert bad == [] and not any(want_st), (launch, bad)
    for launch in (launches[1], launches[0]):         # out_cap one short: the row at 2^32 itself, the one straddling it
        bad, want_st = run_inflate(pkg, torch, dev, launch, streams, src, out, flushed, short=0)
        assert bad == [] and sum(1 for s in want_st if s) == 1, (launch, bad, want_st)
    del src, out


# ---- D2. raw, zlib and gzip members: far input, far output ---------------------------------------------------------------

def run_members(torch, dev, frame, launch, src, out, short=None, bare=False):
    """one launch of far_framed.launches(): the size pass and the framed call over the same shuffled tables (bare: the framed
    call alone, check and in_used both NULL), then, where a member has another behind it, that one from in_off + in_used
    -- formed on the device as a 64-bit tensor.  short: the position whose out_cap is one below its output.
    -> the problems found"""
    n = len(launch)
    caps = ff.caps_of(launch, short)
    in_regs = ff.lay_input(src, launch, write=lambda mem, at, data: put(torch, mem, at, data))
    regs = ff.lay_output(out, launch, caps)
    in_off, in_len = u64(torch, [p.a.offset for p in launch]), u32(torch, [p.a.length for p in launch])
    out_off, out_cap = u64(torch, [p.b.offset for p in launch]), u32(torch, caps)
    osz, used0, st0, olen, chk, used, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(7))
    bad = []
    if not bare:
        dev.inflate_size_call(src, in_off, in_len, frame, osz, used0, st0)
        torch.cuda.synchronize()
        bad += ff.size_problems(launch, list(zip(st0.cpu().tolist(), host_u32(osz), host_u32(used0))))
    dev.inflate_framed_call(src, in_off, in_len, frame, out, out_off, out_cap, olen, None if bare else chk, None if bare else used, st)
    torch.cuda.synchronize()
    none = [None] * n
    got = list(zip(st.cpu().tolist(), host_u32(olen), none if bare else host_u32(used), none if bare else host_u32(chk)))
    bad += ff.framed_problems(launch, caps, got, out, regs, src, in_regs)
    for i, p in enumerate(launch):
        if p.b2 is None or bare or bad:
            continue
        m2, d2 = p.case.follow
        off2 = in_off[i:i + 1] + used0[i:i + 1].to(torch.int64)          # where the second member starts: never on the host
        len2 = in_len[i:i + 1] - used0[i:i + 1]
        assert int(off2.item()) == p.a.offset + len(p.case.data) - len(m2) and int(len2.item()) == len(m2)
        r = [torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(7)]
        dev.inflate_size_call(src, off2, len2, frame, r[0], r[1], r[2])
        o2, c2 = u64(torch, [p.b2.offset]), u32(torch, [len(d2)])
        dev.inflate_framed_call(src, off2, len2, frame, out, o2, c2, r[3], r[4], r[5], r[6])
        torch.cuda.synchronize()
        w = fm.framed(m2, frame, len(d2))
        assert w[4] == d2
        if (r[2].item(), host_u32(r[0])[0], host_u32(r[1])[0]) != fm.size(m2, frame):
            bad.append(("size of the second", p.a.kind))
        if (r[6].item(), host_u32(r[3])[0], host_u32(r[5])[0], host_u32(r[4])[0]) != w[:4]:
            bad.append(("framed second", p.a.kind, p.b2.kind))
        bad += fo.check_rows(out, [(p.b2.offset, d2)], regs)
    return bad


@pytest.mark.timeout(300)
@pytest.mark.parametrize("frame", ff.FRAMES, ids=[ff.FRAME_NAMES[f] for f in ff.FRAMES])
def test_members_far_input_and_far_output(pkg, torch, dev, room, frame):
    """hipdeflate_batch_inflate_size_dev and hipdeflate_batch_inflate_framed_dev (through device.inflate_size_call /
    inflate_framed_call): members at the edge offsets of a 6.06 GiB input, out_off at the edge offsets of a 6.06 GiB output
    (tests/far_framed.py: the layout, pinned on the CPU by test_far_offsets.py).  Held to framed_model: (status, out_size,
    in_used) of the size pass and (status, out_len, in_used, check) of the framed call for every member, the bytes, the
    guards around and the aliases of every far room, the sentinel-filled aliases of the input.  Among the members: a gzip
    name whose NUL lies behind 2^32, an extra field of 65535 bytes that ends at 2^32, trailers cut by 2^32 (gzip 4 | 4, zlib
    2 | 2), refused headers and trailers on far rows between valid neighbours, a name without NUL whose scan must stop at a
    far in_off + in_len, and a pair whose second member is found by in_used.  Once with check and in_used NULL; the
    launches whose boundary output starts at 2^32 and straddles it once more with out_cap one short: status 3, the guard
    behind the room intact."""
    room(2 * BIG)
    launches = ff.launches(frame)
    refused_far = ff.honest(launches)                 # >= 10 far inputs and outputs, an output > 64 KiB at out_off >= 2^32
    assert refused_far >= (6 if frame == fm.GZIP else 4)
    src, out = empty(torch, BIG), empty(torch, BIG)
    for launch in launches:
        bad = run_members(torch, dev, frame, launch, src, out)
        assert bad == [], (frame, [p.case.name for p in launch], bad)
    assert run_members(torch, dev, frame, launches[2], src, out, bare=True) == []
    for launch in launches[:2]:
        short = ff.boundary_position(launch)
        assert launch[short].b.kind in ("straddle", "starts_at")
        assert ff.want_framed(launch[short].case, launch[short].case.room - 1)[:4] == (3, 0, 0, 0)
        bad = run_members(torch, dev, frame, launch, src, out, short=short)
        assert bad == [], (frame, launch[short].case.name, bad)
    assert pkg.lib().hipdeflate_stall_count() == 0
    del src, out


# ---- E. member index, verify and ranged read on a container past 4 GiB --------------------------------------------------

E_TILE = (64 << 20) - 4080                           # repeat k starts at k * E_TILE: 2^32 lies 64 * 4080 bytes into repeat 64
E_REPEATS = 71                                       # 4.44 GiB
E_AT = P32 - 64 * E_TILE                             # where, in the VARIANT (repeat 64), a member starts exactly at 2^32


def zlib_member(kind, data):
    return mm.gz_member(kind, raw_deflate(data, 6), zlib.crc32(data), len(data)), data


class Container:
    """the blob of E_REPEATS tiles on the device, its expected table (far_offsets + member_index_model) and the tiles'
    contents on the device and on the host"""

    def __init__(self, torch):
        rng = np.random.default_rng(2032)
        c = corpus()
        noise = bytes(rng.integers(0, 256, 64 << 20, dtype=np.uint8))
        n = 0xff00

        def stored(kind, at, size=n):
            d = noise[at:at + size]
            return fo.stored_member(kind, d), d
        coded = [zlib_member("BC", c["text"][k * 40000:k * 40000 + n]) for k in range(6)] + \
                [zlib_member("BC", c["fastq"][k * 40000:k * 40000 + n]) for k in range(6)]
        base = [stored("BC", k * n) for k in range(1000)]
        for k, m in enumerate(coded):                                   # the coded members among the stored ones
            base.insert(80 * k + 7, m)
        lead, lead_data = fo.pad_member(E_AT, rng)                      # the variant: its second member starts at 2^32
        other = [stored("IG1", 5), stored("IG2", 70001, 200000), stored("MG", 300017, 150000),
                 (mm.gz_member("MZ", raw_deflate(c["text"][:300000], 6), zlib.crc32(c["text"][:300000]), 300000), c["text"][:300000]),
                 stored("MZ", 500003, 1 << 20), stored("IG1", 1600001, 12345)]
        variant = [(lead, lead_data)] + other + [stored("BC", (1 << 21) + 3 + k * n) for k in range(900)] + coded[::-1]
        self.tiles, self.plain = {}, {}
        for name, members in (("base", base), ("variant", variant)):
            self.tiles[name], self.plain[name] = fo.container_tile(members, E_TILE, rng)
        self.order = ["base"] * 64 + ["variant"] + ["base"] * (E_REPEATS - 65)
        self.walks = {k: mm.walk(v) for k, v in self.tiles.items()}
        assert all(w[1] == mm.OK and w[2] == E_TILE for w in self.walks.values())
        self.ext = fo.extend_member_table({k: (w[0], E_TILE) for k, w in self.walks.items()}, self.order)
        self.n = self.ext["nmembers"]
        self.nbytes = E_TILE * E_REPEATS
        need_room(torch, 2 * self.nbytes + GIB)
        dev_tiles = {k: torch.from_numpy(np.frombuffer(v, dtype=np.uint8).copy()).cuda() for k, v in self.tiles.items()}
        self.blob = empty(torch, self.nbytes)
        self.blob.view(E_REPEATS, E_TILE)[:] = dev_tiles["base"][None, :]
        self.blob[64 * E_TILE:65 * E_TILE] = dev_tiles["variant"]
        self.plain_dev = {k: torch.from_numpy(np.frombuffer(v, dtype=np.uint8).copy()).cuda() for k, v in self.plain.items()}
        self.plain_at = np.concatenate([[0], np.cumsum([len(self.plain[o]) for o in self.order])]).astype(np.int64)
        self.at_p32 = 64 * len(self.walks["base"][0]) + 1               # the member that starts exactly at 2^32
        assert int(self.ext["in_off"][self.at_p32]) - fo.MEMBER_HEADER["IG1"] == P32
        assert self.ext["out_bytes"] > P32 and self.ext["end_offset"] == self.nbytes > P32

    def slice(self, b, e):
        """plain bytes [b, e) from the tiles' contents (short ranges)"""
        out = bytearray()
        while b < e:
            k = int(np.searchsorted(self.plain_at, b, side="right")) - 1
            p = self.plain[self.order[k]]
            take = min(e, int(self.plain_at[k + 1])) - b
            out += p[b - int(self.plain_at[k]):b - int(self.plain_at[k]) + take]
            b += take
        return bytes(out)

    def contents_damaged(self, torch, out):
        return [k for k, o in enumerate(self.order)
                if not torch.equal(out[int(self.plain_at[k]):int(self.plain_at[k + 1])], self.plain_dev[o])]


@pytest.fixture(scope="module")
def container(torch, pkg):
    c = Container(torch)
    yield c
    c.blob = c.plain_dev = None
    gc.collect()
    torch.cuda.empty_cache()


E_S64, E_S32 = 0x5a5a5a5a5a5a5a5a, 0x5a5a5a5a


def sentinel_index(torch, dev, cap):
    d = dev.DeviceInflate(cap + 8)
    d.max_members = cap
    for t in (d.in_off, d.out_off):
        t.fill_(E_S64)
    for t in (d.in_len, d.out_size, d.crc_want):
        t.fill_(E_S32)
    return d


def index_tables(d):
    return [x.cpu().numpy().view(np.uint64 if wide else np.uint32).astype(np.uint64)
            for x, wide in ((d.in_off, 1), (d.in_len, 0), (d.out_size, 0), (d.out_off, 1), (d.crc_want, 0))]


@pytest.mark.timeout(300)
def test_index_and_run_on_a_container_past_4gib(pkg, torch, dev, container, room):
    """hipdeflate_index_members_dev, DeviceInflate.index / run / verify on 4.44 GiB of members: a tile of about 1000 stored
    noise members (blob ~ contents) with text and FASTQ-like ones among them, repeated 71 times; repeat 64 is a variant of the
    same length in which a member starts exactly at 2^32, followed by the other member kinds.  The summary, the four tables
    and the trailer CRCs are the extended model's; run gives the tiles' contents; a blob cut at 2^32 + 1000 answers CUT
    at 2^32; a flipped trailer bit in a member past 2^32 is named."""
    c = container
    room(2 * c.nbytes + GIB)
    stalls = pkg.lib().hipdeflate_stall_count()
    d = sentinel_index(torch, dev, c.n + 3)
    s = d.index(c.blob)
    assert (s.nmembers, s.out_bytes, s.end_offset, s.status) == (c.n, c.ext["out_bytes"], c.nbytes, 0)
    for got, name, sent in zip(index_tables(d), ("in_off", "in_len", "out_size", "out_off", "crc"),
                               (E_S64, E_S32, E_S32, E_S64, E_S32)):
        assert fo.check_table(got[:c.n], c.ext[name], name) == [] and np.all(got[c.n:] == sent), name
    assert int(c.ext["in_off"].max()) > P32 and int(c.ext["out_off"].max()) > P32
    out = empty(torch, c.ext["out_bytes"] + fo.GUARD)
    out[c.ext["out_bytes"]:] = SENT
    out[P32 - 65536:P32 + 65536] = 0
    s2 = d.run(c.blob, out[:c.ext["out_bytes"]], s)
    assert s2.out_bytes == c.ext["out_bytes"] and d.verify(c.n) == c.n
    assert c.contents_damaged(torch, out) == []
    assert bool((out[c.ext["out_bytes"]:] == SENT).all())
    # cut 1000 bytes behind 2^32: inside the member that starts there
    rows_v, status_v, end_v = mm.walk(c.tiles["variant"], E_AT + 1000)
    assert (status_v, end_v) == (mm.CUT, E_AT) and len(rows_v) == 1
    d = sentinel_index(torch, dev, c.n + 3)
    s = d.index(c.blob[:P32 + 1000])
    assert (s.nmembers, s.end_offset, s.status) == (c.at_p32, P32, mm.CUT)
    assert s.out_bytes == int(c.ext["out_off"][c.at_p32])
    for got, name in zip(index_tables(d), ("in_off", "in_len", "out_size", "out_off", "crc")):
        assert fo.check_table(got[:c.at_p32], c.ext[name][:c.at_p32], name) == []
    # one flipped trailer bit in a member past 2^32
    g = c.at_p32 + 1500
    end = int(c.ext["in_off"][g]) + int(c.ext["in_len"][g])
    assert end - 8 > P32 + (64 << 20)
    d = dev.DeviceInflate(c.n)
    c.blob[end - 8] ^= 1
    try:
        with pytest.raises(pkg.HipDeflateError, match=r"member %d:" % g):
            d.run(c.blob, out[:c.ext["out_bytes"]])
        assert d.verify(c.n) == g
    finally:
        c.blob[end - 8] ^= 1
    assert pkg.lib().hipdeflate_stall_count() == stalls
    del out


@pytest.mark.timeout(300)
def test_ranged_reads_past_4gib(pkg, torch, dev, container, room):
    """hipdeflate_read_ranges_dev / DeviceInflate.read_ranges on the same blob, held to range_read_model.plan on the extended
    table: two ranges of 33 tiles each (2.06 GiB: dst_off of everything behind them is past 2^32), ranges ending just below,
    at and just past plain offset 2^32, 100 bytes wholly past it, and virtual offsets whose coffset exceeds 2^32 -- the
    member that starts at 2^32 among them."""
    c = container
    rows = fo.table_rows(c.ext)
    pb = len(c.plain["base"])
    total = c.ext["out_bytes"]
    begins = [0, 10 * pb, P32 - 100, P32 - 50, P32 - 10, P32 + 777, total - 5, 64 * pb - 3]
    ends = [33 * pb, 43 * pb, P32 - 1, P32, P32 + 1, P32 + 877, total + 9, 64 * pb + 70000]
    p = rm.plan(rows, rm.BYTES, begins, ends)
    assert p["q_status"] == [0] * len(begins) and p["dst_off"][2] > P32 and p["q_len"][5] == 100
    room(c.nbytes + p["out_bytes"] + p["sel_bytes"] + GIB)
    d = dev.DeviceInflate(c.n)
    assert d.index(c.blob).status == 0
    buf = empty(torch, fo.GUARD + p["out_bytes"] + fo.GUARD)
    buf[:fo.GUARD] = SENT
    buf[fo.GUARD + p["out_bytes"]:] = SENT
    dst = buf[fo.GUARD:]

    def call(kind, b, e, plan, cap):
        dst_off, q_len, q_status, s = d.ranges_call(c.blob, u64(torch, b), u64(torch, e), kind, c.n, dst, cap)
        assert host_u32(q_len) == plan["q_len"] and q_status.cpu().tolist() == plan["q_status"]
        assert fo.check_table(dst_off.cpu().numpy().view(np.uint64), plan["dst_off"], "dst_off") == []
        assert (s.out_bytes, s.nrefused, s.nselected, s.sel_bytes) == \
            (plan["out_bytes"], plan["nrefused"], plan["nselected"], plan["sel_bytes"])
        assert (s.status, s.bad_member) == (0, c.n)
        assert bool((buf[:fo.GUARD] == SENT).all()) and bool((buf[fo.GUARD + p["out_bytes"]:] == SENT).all())

    call(rm.BYTES, begins, ends, p, p["out_bytes"])
    for q in (0, 1):                                                    # the two long ones: tile by tile on the device
        assert fo.tiles_damaged(dst, p["dst_off"][q], [c.plain_dev["base"]], [0] * 33, torch.equal) == [], q
    small = [(p["dst_off"][q], c.slice(*p["spans"][q])) for q in range(2, len(begins))]
    assert all(off > P32 for off, _ in small)
    assert fo.check_rows(dst, small, []) == []
    # virtual offsets: members that start past 2^32
    starts, _ = rm.member_starts(rows)
    m0 = c.at_p32
    assert starts[m0] == P32
    vb = [rm.voffset(starts[m0], 5), rm.voffset(starts[m0 + 1], 0), rm.voffset(starts[m0 + 900], 0xfeff), rm.voffset(starts[m0], 0),
          rm.voffset(P32 + 1, 0)]
    ve = [rm.voffset(starts[m0 + 1], 100), rm.voffset(starts[m0 + 3], 17), rm.voffset(starts[m0 + 902], 1), rm.voffset(starts[m0], 0),
          rm.voffset(starts[m0 + 1], 0)]
    pv = rm.plan(rows, rm.VOFFSET, vb, ve)
    assert pv["q_status"] == [0, 0, 0, 0, 1] and min(v >> 16 for v in vb + ve) >= P32
    buf[fo.GUARD:fo.GUARD + pv["out_bytes"]] = 0
    call(rm.VOFFSET, vb, ve, pv, p["out_bytes"])
    assert fo.check_rows(dst, [(pv["dst_off"][q], c.slice(*pv["spans"][q])) for q in range(len(vb))], []) == []
    # ... and the wrapper, which sizes dst itself
    got, dst_off, q_len, q_status, s = d.read_ranges(c.blob, begins[2:], ends[2:])
    assert bytes(got.cpu().numpy()) == b"".join(x for _, x in small) and s.status == 0
    del buf, dst, got


# ---- F. one stream past 4 GiB -------------------------------------------------------------------------------------------

F_CHUNK = 256 << 10
F_TILE_CHUNKS = 256                                  # a 64 MiB tile
F_NBYTES = P32 + (1 << 29) + 48                      # 72 tiles and a ragged chunk of 48 bytes
F_FIELDS = ("out_bytes", "in_bytes", "bad_chunk", "nchunks", "check", "status")


def stream_tile(level, frame, text_share):
    """the 64 MiB tile: 256 chunks drawn from 16 distinct ones (the twin codes each once), noise : text = 3 : 1 at level 6
    and 7 : 1 at level 1 -- mostly noise, so that the stream passes 2^32 as its input does"""
    c = corpus()
    rng = np.random.default_rng(900 + level)
    distinct = [bytes(rng.integers(0, 256, F_CHUNK, dtype=np.uint8)) for _ in range(16 - text_share)] + \
               [(c["text"] + c["fastq"])[k * 100000:k * 100000 + F_CHUNK] for k in range(text_share)]
    pick = list(range(16)) + [int(v) for v in rng.integers(0, 16, F_TILE_CHUNKS - 16)]
    rng.shuffle(pick)
    return fo.StreamTile(b"".join(distinct[k] for k in pick), level, frame, F_CHUNK)


def fields(s):
    return {f: getattr(s, f) for f in F_FIELDS}


F_CASES = [(1, sm.FRAME_GZIP, 2, False), (1, sm.FRAME_ZLIB, 2, True), (6, sm.FRAME_GZIP, 4, False)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("level,frame,text_share,wrappers", F_CASES, ids=["l1-gzip", "l1-zlib-wrappers", "l6-gzip"])
def test_one_stream_past_4gib(pkg, torch, dev, room, level, frame, text_share, wrappers):
    """hipdeflate_stream_deflate_dev / _inflate_dev (and device.deflate_stream / inflate_stream) on 2^32 + 2^29 + 48 bytes in
    chunks of 256 KiB, the real windows of 1 GiB of slots: the stream (repeat by repeat on the device), the chunk table with
    entries past 2^32, out_bytes, in_bytes, check, ISIZE = nbytes - 2^32 and status 0 are the tiled model's; dst_cap one
    short gives status 3 and the same out_bytes; the decode gives the tiled input back; a damaged chunk past stream offset
    2^32 is named; an ISIZE rewritten to the low 32 bits + 1 is refused."""
    t = stream_tile(level, frame, text_share)
    e = t.expected(F_NBYTES)
    want = e["summary"]
    need, nchunks = want["out_bytes"], want["nchunks"]
    assert e["repeats"] == 72 and nchunks == 72 * 256 + 1 and want["in_bytes"] > P32
    # (level 1 keeps 7 : 1 as stored blocks and text at ~ 0.6: a stream of 4.6e9 bytes.  Level 6 at the 3 : 1 the case is given
    # brings it to 3.9e9, below 2^32: there the chunks READ past 2^32 and the counts pass it, the stream's own offsets do not)
    assert (need > P32 and int(e["chunk_off"][-1]) > P32) == (level == 1)
    bound = int(pkg.lib().hipdeflate_stream_bound(F_NBYTES, F_CHUNK, level, frame))
    assert need <= bound
    room(F_NBYTES + (bound + F_NBYTES if wrappers else need) + GIB)
    stalls = pkg.lib().hipdeflate_stall_count()
    tile_dev = torch.from_numpy(np.frombuffer(t.tile, dtype=np.uint8).copy()).cuda()
    coded_dev = torch.from_numpy(np.frombuffer(t.stream, dtype=np.uint8).copy()).cuda()
    whole = empty(torch, F_NBYTES + fo.GUARD)                               # the input; later the decode's output and its guard
    whole[:72 * len(t.tile)].view(72, len(t.tile))[:] = tile_dev[None, :]
    whole[72 * len(t.tile):F_NBYTES] = tile_dev[:48]
    data = whole[:F_NBYTES]
    if wrappers:
        stream, tab, s = dev.deflate_stream(data, level, frame, F_CHUNK)
        assert fields(s) == want and stream.numel() == need
    else:
        buf = empty(torch, fo.GUARD + need + fo.GUARD)
        buf[:fo.GUARD] = SENT
        buf[fo.GUARD + need - 1:] = SENT
        tab = torch.full((nchunks + 3,), -2, dtype=torch.int64, device="cuda")
        s = dev.deflate_stream_call(data, level, frame, F_CHUNK, buf[fo.GUARD:], need - 1, tab[1:])     # one byte short
        assert fields(s) == dict(want, status=3)
        assert bool((buf[:fo.GUARD] == SENT).all()) and bool((buf[fo.GUARD + need - 1:] == SENT).all())
        s = dev.deflate_stream_call(data, level, frame, F_CHUNK, buf[fo.GUARD:], need, tab[1:])
        assert fields(s) == want
        assert bool((buf[:fo.GUARD] == SENT).all()) and bool((buf[fo.GUARD + need:] == SENT).all())
        assert int(tab[0]) == -2 and int(tab[-1]) == -2
        stream, tab = buf[fo.GUARD:fo.GUARD + need], tab[1:-1]
    assert fo.check_table(tab.cpu().numpy().view(np.uint64), e["chunk_off"], "chunk_off") == []
    assert fo.check_stream(stream, e, coded_dev, torch.equal) == []
    if frame == sm.FRAME_GZIP:
        assert fo.gzip_isize(fo.to_bytes(stream[need - 4:])) == F_NBYTES - P32 == e["isize"]
    # the decode, into the input's own buffer: zeroed first, so that nothing of the input is left to pass for output
    del data
    out = whole
    out.zero_()
    out[F_NBYTES:] = SENT
    if wrappers:
        back = dev.inflate_stream(stream, tab, F_CHUNK, F_NBYTES, frame)
        assert fo.tiles_damaged(back, 0, [tile_dev], [0] * 72, torch.equal) == [] and fo.to_bytes(back[72 * len(t.tile):]) == t.tile[:48]
        del back
    s = dev.inflate_stream_call(stream, frame, tab, nchunks, F_CHUNK, F_NBYTES, out, F_NBYTES)
    assert fields(s) == dict(want, out_bytes=F_NBYTES, in_bytes=need)
    assert fo.tiles_damaged(out, 0, [tile_dev], [0] * 72, torch.equal) == []
    assert fo.to_bytes(out[72 * len(t.tile):F_NBYTES]) == t.tile[:48] and bool((out[F_NBYTES:] == SENT).all())
    # a chunk past stream offset 2^32 (level 6: past input offset 2^32) whose first block header is damaged: the first
    # one the model's inflate refuses
    k = int(np.searchsorted(e["chunk_off"], P32 + (1 << 20))) if level == 1 else P32 // F_CHUNK + 5
    while True:
        at = int(e["chunk_off"][k])
        coded = bytearray(fo.to_bytes(stream[at:int(e["chunk_off"][k + 1])]))
        coded[1] ^= 0x55
        r, b = hdtest.oracle_inflate_flushed(bytes(coded), F_CHUNK)
        if r != 0 or len(b) != F_CHUNK:
            break
        k += 1
    assert (at > P32 or level != 1) and k * F_CHUNK > P32 and k < nchunks - 1
    stream[at + 1] ^= 0x55
    s = dev.inflate_stream_call(stream, frame, tab, nchunks, F_CHUNK, F_NBYTES, out, F_NBYTES)
    stream[at + 1] ^= 0x55
    assert (s.status, s.bad_chunk) == (2, k)
    if frame == sm.FRAME_GZIP:
        wrong = ((F_NBYTES & 0xffffffff) + 1).to_bytes(4, "little")
        put(torch, stream, need - 4, wrong)
        s = dev.inflate_stream_call(stream, frame, tab, nchunks, F_CHUNK, F_NBYTES, out, F_NBYTES)
        put(torch, stream, need - 4, e["tail"][-4:])
        assert (s.status, s.bad_chunk) == (2, nchunks)
    assert pkg.lib().hipdeflate_stall_count() == stalls
    del out, whole, stream


# ---- G. one stream at the ends of its own 32-bit counters ---------------------------------------------------------------

MAX_IN = 1 << 28                                     # include/hipdeflate_params.h HD_INFLATE_MAX_IN


static_code, static_match = fo.static_code, fo.static_match                # (the generators live in far_offsets.py: the CPU pins use them too)
long_input_stream, long_output_stream = fo.long_input_stream, fo.long_output_stream


@pytest.mark.timeout(300)
def test_inflate_input_of_max_in(pkg, torch, dev, room):
    """k_inflate through hipdeflate_batch_inflate_dev on a stream of HD_INFLATE_MAX_IN - 1 bytes -- stored blocks and a short
    static block, so that bit positions run up to 2^31 - 8 -- and the answers include/hipdeflate.h gives for a stream of exactly
    HD_INFLATE_MAX_IN bytes: HD_E_ARG from the host entries, status 1 / out_len 0 from the _dev entry."""
    room(3 * MAX_IN)
    rng = np.random.default_rng(28)
    host, pattern, reps, rest = long_input_stream(MAX_IN - 1, rng)
    total = reps * 65535 + len(rest)
    src = empty(torch, MAX_IN + 16)
    src[:MAX_IN - 1] = torch.from_numpy(host).cuda()
    src[MAX_IN - 1:] = 0
    out = empty(torch, total + fo.GUARD)
    out[total:] = SENT
    pat = torch.from_numpy(pattern).cuda()
    olen, crc = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    zero, n_in, n_max, cap = u64(torch, [0]), u32(torch, [MAX_IN - 1]), u32(torch, [MAX_IN]), u32(torch, [total])
    dev.device_inflate(src, zero, n_in, out, zero, cap, olen, crc, st)
    torch.cuda.synchronize()
    assert (st.item(), host_u32(olen)[0]) == (0, total)
    assert bool((out[:reps * 65535].view(reps, 65535) == pat[None, :]).all())
    assert fo.to_bytes(out[reps * 65535:total]) == rest and bool((out[total:] == SENT).all())
    checks = [zlib.crc32(pattern.tobytes())] * reps + [zlib.crc32(rest)]
    assert host_u32(crc)[0] == sm.fold(checks, [65535] * reps + [len(rest)], sm.CRC32)
    # exactly HD_INFLATE_MAX_IN: the _dev entry cannot see in_len and reports status 1 / out_len 0, writing nothing
    out[:4096] = SENT
    olen.fill_(-1)
    dev.device_inflate(src, zero, n_max, out, zero, cap, olen, crc, st)
    torch.cuda.synchronize()
    assert (st.item(), host_u32(olen)[0]) == (1, 0) and bool((out[:4096] == SENT).all())
    del src, out
    # ... the host entries answer HD_E_ARG before they launch
    big = np.concatenate([host, np.zeros(1, dtype=np.uint8)])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    room_ = np.zeros(4096, dtype=np.uint8)
    one = [np.zeros(1, dtype=np.uint64), np.array([MAX_IN], dtype=np.uint32), np.zeros(1, dtype=np.uint64),
           np.array([4096], dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)]
    for fn in (pkg.lib().hipdeflate_batch_inflate, pkg.lib().hipdeflate_batch_inflate_flush):
        assert fn(p(big), p(one[0]), p(one[1]), 1, p(room_), p(one[2]), p(one[3]), p(one[4]), p(one[5]), p(one[6])) == pkg.HD_E_ARG
    n = ctypes.c_size_t(4096)
    assert pkg.lib().hip_inflate(p(room_), ctypes.byref(n), p(big), MAX_IN) == pkg.HD_E_ARG


def run_long_output(pkg, torch, dev, total, short):
    """-> (status, out_len, crc, the output tensor with a guard behind out_cap, seconds)"""
    import time
    host, pattern = long_output_stream(total)
    src = torch.from_numpy(np.concatenate([host, np.zeros(16, dtype=np.uint8)])).cuda()
    cap = total - (1 if short else 0)
    out = empty(torch, total + fo.GUARD)
    out[cap:] = SENT
    olen, crc = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    zero, n_in, n_cap = u64(torch, [0]), u32(torch, [len(host)]), u32(torch, [cap])
    dev.device_inflate(src, zero, n_in, out, zero, n_cap, olen, crc, st)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool((out[cap:] == SENT).all()), "written behind out_cap"
    return st.item(), host_u32(olen)[0], host_u32(crc)[0], out, pattern, host, dt


def check_long_output(torch, total, res):
    st, olen, crc, out, pattern, host, dt = res
    assert (st, olen) == (0, total)
    pat = torch.from_numpy(pattern).cuda()
    view = out[:total].view(total // 32768, 32768)
    for a in range(0, total // 32768, 8192):
        assert bool((view[a:a + 8192] == pat[None, :]).all()), a
    assert crc == sm.fold([zlib.crc32(pattern.tobytes())] * (total // 32768), [32768] * (total // 32768), sm.CRC32)


@pytest.mark.timeout(60)
def test_inflate_output_of_128_mib(pkg, torch, dev, room):
    """the stream of test_inflate_output_past_2_31 at 128 MiB of output, exact and one short: here the oracle's inflate
    can still answer for both, and the stream reads as zlib's.  Its kernel time is what decides whether the 2^31 case may
    stay: 0.86 s on an MI355X (printed at every run)."""
    total = 128 << 20
    room(2 * total)
    res = run_long_output(pkg, torch, dev, total, short=False)
    print("128 MiB of output from one stream: %.3f s" % res[-1])
    check_long_output(torch, total, res)
    stream = res[5].tobytes()
    assert zlib.decompress(stream, -15) == res[4].tobytes() * (total // 32768)
    assert hdtest.oracle_inflate(stream, total - 1)[0] == 3
    st, olen, _, _, _, _, _ = run_long_output(pkg, torch, dev, total, short=True)
    assert st == 3


G2_TOTAL = (1 << 31) + 65536


@pytest.mark.timeout(42)
@pytest.mark.parametrize("short", [False, True], ids=["exact", "one-short"])
def test_inflate_output_past_2_31(pkg, torch, dev, room, short):
    """2^31 + 65,536 bytes of output from a stream of 27 MB -- one stored 32 KiB block of noise, then 8.3 million static
    matches of length 258 at distance 32768 -- with out_cap exact and one short: output positions, out_len and out_cap
    past 2^31 in the one wavefront that writes it all.  The output is the 32 KiB pattern 65,538 times (compared through a
    reshaped view), the CRC-32 stream_model.fold's; one short, the status is 3 and nothing lies behind out_cap.
    Time guard: test_inflate_output_of_128_mib's call took 0.86 s of kernel time on an MI355X (156 MB/s for one
    wavefront); sixteen times that, 13.7 s, is under the 20 s this case may cost, so it stays, under a timeout of three
    times the projection."""
    room(G2_TOTAL + GIB)
    res = run_long_output(pkg, torch, dev, G2_TOTAL, short)
    print("2^31 + 64 KiB of output from one stream (%s): %.3f s" % ("one short" if short else "exact", res[-1]))
    if short:
        assert res[0] == 3
    else:
        check_long_output(torch, G2_TOTAL, res)


# ---- G2. the size pass and the framed decode at the end of the 32-bit bit position ---------------------------------------

def max_in_member(torch, frame):
    """the stream of test_inflate_input_of_max_in in a frame, HD_INFLATE_MAX_IN - 1 bytes with header and trailer, on the
    device in a buffer of HD_INFLATE_MAX_IN + 16 -> (src, pattern, reps, rest, check, total)"""
    host, pattern, reps, rest = long_input_stream(MAX_IN - 1 - fo.LONG_OVERHEAD[frame], np.random.default_rng(28))
    member, check, total = fo.framed_long_member(frame, host, pattern, reps, rest)
    assert len(member) == MAX_IN - 1 and total == reps * 65535 + len(rest)
    src = empty(torch, MAX_IN + 16)
    src[:MAX_IN - 1] = torch.from_numpy(member).cuda()
    src[MAX_IN - 1:] = 0
    return src, pattern, reps, rest, check, total


def timed(torch, call):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


@pytest.mark.timeout(1, func_only=True)
@pytest.mark.parametrize("frame", ff.FRAMES, ids=[ff.FRAME_NAMES[f] for f in ff.FRAMES])
def test_size_pass_input_of_max_in(pkg, torch, dev, room, frame):
    """k_inflate_size on a member of HD_INFLATE_MAX_IN - 1 bytes: 4096 stored blocks, each a seek of its own 32-bit bit
    reader, up to bit 2^31 - 8 and some; the answer is (0, total, HD_INFLATE_MAX_IN - 1), by construction (the CPU pin:
    test_long_streams_in_a_frame_are_what_the_gpu_tests_take_them_for).  gzip: with ISIZE off by one the status is 1 -- the
    read at src + used + 4 with used near 2^28.  raw: a real buffer of exactly HD_INFLATE_MAX_IN bytes answers status 1
    and zeros from both _dev calls and leaves a sentinel-filled output alone.
    Time (printed at every run), first measured on an MI355X: the call 0.0044 s (raw), 0.0045 s (zlib, gzip) -- nearly all of it
    stored-block seeks; the whole test with the 256 MiB it makes and uploads 0.17 / 0.15 / 0.18 s.  The timeout is three
    times the slowest, in whole seconds, on the test's own body."""
    import time
    t_test = time.perf_counter()
    room(2 * MAX_IN)
    src, pattern, reps, rest, check, total = max_in_member(torch, frame)
    zero, n_in = u64(torch, [0]), u32(torch, [MAX_IN - 1])
    osz, used, st = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dt = timed(torch, lambda: dev.inflate_size_call(src, zero, n_in, frame, osz, used, st))
    print("size pass over a %s member of 2^28 - 1 bytes: %.4f s" % (ff.FRAME_NAMES[frame], dt))
    assert (st.item(), host_u32(osz)[0], host_u32(used)[0]) == (0, total, MAX_IN - 1)
    if frame == fm.GZIP:
        put(torch, src, MAX_IN - 1 - 4, ((total + 1) & 0xffffffff).to_bytes(4, "little"))
        dev.inflate_size_call(src, zero, n_in, frame, osz, used, st)
        torch.cuda.synchronize()
        assert (st.item(), host_u32(osz)[0], host_u32(used)[0]) == (1, 0, 0)
    if frame == fm.RAW:
        n_max, cap = u32(torch, [MAX_IN]), u32(torch, [4096])
        out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
        olen, chk = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        dev.inflate_size_call(src, zero, n_max, frame, osz, used, st)
        torch.cuda.synchronize()
        assert (st.item(), host_u32(osz)[0], host_u32(used)[0]) == (1, 0, 0)
        dev.inflate_framed_call(src, zero, n_max, frame, out, zero, cap, olen, chk, used, st)
        torch.cuda.synchronize()
        assert (st.item(), host_u32(olen)[0], host_u32(used)[0], host_u32(chk)[0]) == (1, 0, 0, 0) and bool((out == SENT).all())
    assert pkg.lib().hipdeflate_stall_count() == 0
    del src
    print("the whole test: %.2f s" % (time.perf_counter() - t_test))


@pytest.mark.timeout(5, func_only=True)
@pytest.mark.parametrize("frame", [fm.GZIP, fm.ZLIB], ids=["gzip", "zlib"])
def test_framed_decode_input_of_max_in(pkg, torch, dev, room, frame):
    """k_frame_open, k_inflate_framed, k_chunk_adler (zlib) and k_frame_close on the same member: (0, total, in_used =
    HD_INFLATE_MAX_IN - 1, check), the bytes consumed and the trailer's address both near 2^28; the output is the 65535-byte
    pattern 4096 times and the rest (compared through a reshaped view), the guard behind it intact.
    Time (printed at every run), first measured on an MI355X: the call 1.26 s (gzip), 1.29 s (zlib: k_chunk_adler's one
    wavefront over 256 MiB is the 0.03 s), the whole test 1.45 s either way -- 256 MiB of stored blocks through one wavefront
    are well under 10 s, so both frames stay.  The timeout is three times 1.45 s, in whole seconds, on the test's own body."""
    import time
    t_test = time.perf_counter()
    room(3 * MAX_IN)
    src, pattern, reps, rest, check, total = max_in_member(torch, frame)
    out = empty(torch, total + fo.GUARD)
    out[:total] = 0
    out[total:] = SENT
    zero, n_in, cap = u64(torch, [0]), u32(torch, [MAX_IN - 1]), u32(torch, [total])
    olen, chk, used, st = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
    dt = timed(torch, lambda: dev.inflate_framed_call(src, zero, n_in, frame, out, zero, cap, olen, chk, used, st))
    print("framed decode of a %s member of 2^28 - 1 bytes: %.4f s" % (ff.FRAME_NAMES[frame], dt))
    assert (st.item(), host_u32(olen)[0], host_u32(used)[0], host_u32(chk)[0]) == (0, total, MAX_IN - 1, check)
    pat = torch.from_numpy(pattern).cuda()
    assert bool((out[:reps * 65535].view(reps, 65535) == pat[None, :]).all())
    assert fo.to_bytes(out[reps * 65535:total]) == rest and bool((out[total:] == SENT).all())
    assert pkg.lib().hipdeflate_stall_count() == 0
    del src, out
    print("the whole test: %.2f s" % (time.perf_counter() - t_test))


# ---- H. device.inflate_members: the prefix sum it hands to the decoder passes 2^32 --------------------------------------

H_BIG = 64 << 20


@pytest.mark.timeout(4, func_only=True)
@pytest.mark.parametrize("frame", [fm.GZIP, fm.ZLIB], ids=["gzip", "zlib"])
def test_inflate_members_prefix_sum_past_4gib(pkg, torch, dev, room, frame):
    """device.inflate_members -- the size pass, hipdeflate_scan_sizes_dev, one allocation, the framed decode -- over 69 rows:
      0       100 bytes of text, made by zlib
      1..64   long_output_stream(64 MiB) in the frame, all rows pointing at ONE copy: row 64's output starts at 2^32 - 64 MiB
              + 100 and straddles 2^32
      65      gzip: the same member with ISIZE off by one; zlib: with a bad FCHECK.  The size pass refuses it: no room
      66      70,000 FASTQ-like bytes, made by zlib: out_off 2^32 + 100
      67      the 64 MiB member with one bit of its CRC-32 (Adler-32) flipped: the size pass accepts it, the decode refuses
              it -- status 1, out_len 0, and its 64 MiB of room are allocated
      68      5 bytes, made by zlib
    (three copies of the 64 MiB member's 0.85 MB in the blob, 2.6 MB.)  out_off is the exclusive prefix sum of the model's
    size-pass sizes, out.numel() their sum, status and out_len the framed model's in exactly that room; the 64 MiB rows
    are compared through a (2048, 32768) view against the pattern, the small rows as bytes.
    Time (printed at every run), first measured on an MI355X: the call -- both passes, 66 wavefronts side by side on 64 MiB
    each -- 0.455 s (gzip), 0.521 s (zlib); the whole test, with the model's three 64 MiB decodes on the host, 1.20 / 0.81 s.
    The timeout is three times 1.20 s, in whole seconds, on the test's own body."""
    import time
    t_test = time.perf_counter()
    room(6 * GIB)
    stream, pattern = long_output_stream(H_BIG)
    member, check, total = fo.framed_long_member(frame, stream, pattern, H_BIG // 32768)
    big = member.tobytes()
    assert total == H_BIG
    c = corpus()
    wbits = sm.WBITS[frame]

    def made(d):
        z = zlib.compressobj(6, zlib.DEFLATED, wbits)
        return z.compress(d) + z.flush()
    small = [c["text"][:100], c["fastq"][:70000], c["text"][5000:5005]]
    if frame == fm.GZIP:
        refused_early = big[:-4] + ((H_BIG + 1) & 0xffffffff).to_bytes(4, "little")
        refused_late = big[:-8] + bytes([big[-8] ^ 0x10]) + big[-7:]
    else:
        refused_early = big[:1] + bytes([big[1] ^ 1]) + big[2:]
        refused_late = big[:-4] + bytes([big[-4] ^ 0x10]) + big[-3:]
    distinct = [made(small[0]), big, refused_early, made(small[1]), refused_late, made(small[2])]
    which = [0] + [1] * 64 + [2, 3, 4, 5]
    blob, offs = bytearray(), []
    for i, m in enumerate(distinct):
        blob += bytes(range(1, 1 + (i * 5 - len(blob)) % 16))
        offs.append(len(blob))
        blob += m
    blob += bytes(range(1, 65))
    sizes = [fm.size(m, frame) for m in distinct]
    wants = [fm.framed(m, frame, s[1]) for m, s in zip(distinct, sizes)]
    assert [s[0] for s in sizes] == [0, 0, 1, 0, 0, 0] and sizes[1][1] == sizes[4][1] == H_BIG
    assert wants[1][:4] == (0, H_BIG, len(big), check) and wants[4][:4] == (1, 0, 0, 0)
    assert [w[4] for w in (wants[0], wants[3], wants[5])] == small
    want_size = np.array([sizes[k][1] for k in which], dtype=np.uint64)
    want_off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(want_size)[:-1]])
    assert int(want_off[64]) == P32 - H_BIG + 100 and int(want_off[65]) == int(want_off[66]) == P32 + 100
    assert int(want_off[68]) == P32 + 100 + 70000 + H_BIG
    d_blob = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    in_off, in_len = u64(torch, [offs[k] for k in which]), u32(torch, [len(distinct[k]) for k in which])
    res = []
    dt = timed(torch, lambda: res.extend(dev.inflate_members(d_blob, in_off, in_len, frame)))
    print("inflate_members, 66 members of 64 MiB among 69 (%s): %.3f s" % (ff.FRAME_NAMES[frame], dt))
    out, out_off, out_len, status = res
    assert out.numel() == int(want_size.sum()) == 65 * H_BIG + 70105
    assert fo.check_table(out_off.cpu().numpy().view(np.uint64), want_off, "out_off") == []
    assert status.cpu().tolist() == [wants[k][0] for k in which] and status[67].item() == 1
    assert host_u32(out_len) == [wants[k][1] for k in which] and host_u32(out_len)[67] == 0
    pat = torch.from_numpy(pattern).cuda()
    for row in range(1, 65):
        at = int(want_off[row])
        assert bool((out[at:at + H_BIG].view(H_BIG // 32768, 32768) == pat[None, :]).all()), row
    assert fo.check_rows(out, [(int(want_off[r]), wants[which[r]][4]) for r in (0, 66, 68)], []) == []
    assert pkg.lib().hipdeflate_stall_count() == 0
    del out, res
    print("the whole test: %.2f s" % (time.perf_counter() - t_test))


# ---- I. the host-buffer forms: 64-bit offsets into host memory ----------------------------------------------------------

I_SIZE = P32 + (8 << 20)
I_MEMBERS = {fm.GZIP: ("all_fields", "name300", "fastq70k", "five"), fm.ZLIB: ("fastq70k", "garbage7", "text300k", "five")}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("frame", [fm.GZIP, fm.ZLIB], ids=["gzip", "zlib"])
def test_host_forms_with_far_host_offsets(pkg, frame):
    """hipdeflate_batch_inflate_size and hipdeflate_batch_inflate_framed (through the library itself: the list wrappers cannot
    state an offset) on two host arrays of 2^32 + 8 MiB whose pages are never touched but where the members are: a member
    ending at, straddling, starting at and just behind offset 2^32 of the input, its output at the same kind of the output
    between 4096-byte sentinel guards, a low-offset control beside each.  The answers and the bytes are the model's."""
    with open("/proc/meminfo") as f:
        avail = next(int(line.split()[1]) * 1024 for line in f if line.startswith("MemAvailable:"))
    assert avail >= 2 * I_SIZE, "needs %.1f GiB of host memory, %.1f are available" % (2 * I_SIZE / GIB, avail / GIB)
    L = pkg.lib()
    hin, hout = np.empty(I_SIZE, dtype=np.uint8), np.empty(I_SIZE, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    c = ff.cases(frame)
    control = c["twin1"]
    for kind, name in zip(fo.BOUNDARY, I_MEMBERS[frame]):
        ms = [c[name], control]
        a = [fo.edge_offset(kind, len(ms[0].data), I_SIZE), fo.edge_offset("low", len(control.data), I_SIZE)]
        b = [fo.edge_offset(kind, ms[0].room, I_SIZE), fo.edge_offset("low", control.room, I_SIZE)]
        assert fo.is_far(a[0], len(ms[0].data)) and fo.is_far(b[0], ms[0].room)
        for m, ai, bi in zip(ms, a, b):
            hin[ai:ai + len(m.data)] = np.frombuffer(m.data, dtype=np.uint8)
            hin[ai + len(m.data):ai + len(m.data) + 16] = 0x77
            hout[bi - fo.GUARD:bi] = SENT
            hout[bi:bi + m.room] = 0
            hout[bi + m.room:bi + m.room + fo.GUARD] = SENT
        in_off, in_len = np.array(a, dtype=np.uint64), np.array([len(m.data) for m in ms], dtype=np.uint32)
        out_off, cap = np.array(b, dtype=np.uint64), np.array([m.room for m in ms], dtype=np.uint32)
        r = [np.full(2, 0xfffffff9, dtype=np.uint32) for _ in range(6)]
        st0, st = np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int32)
        assert L.hipdeflate_batch_inflate_size(p(hin), p(in_off), p(in_len), 2, frame, p(r[0]), p(r[1]), p(st0)) == 0
        assert [(int(st0[i]), int(r[0][i]), int(r[1][i])) for i in range(2)] == [ff.want_size(m) for m in ms], (kind, name)
        assert L.hipdeflate_batch_inflate_framed(p(hin), p(in_off), p(in_len), 2, frame, p(hout), p(out_off), p(cap), p(r[2]), p(r[3]),
                                                 p(r[4]), p(st)) == 0
        wants = [ff.want_framed(m, m.room) for m in ms]
        assert [(int(st[i]), int(r[2][i]), int(r[4][i]), int(r[3][i])) for i in range(2)] == [w[:4] for w in wants], (kind, name)
        for m, w, bi in zip(ms, wants, b):
            assert w[0] == 0 and hout[bi:bi + m.room].tobytes() == w[4] == m.plain, (kind, m.name)
            assert np.all(hout[bi - fo.GUARD:bi] == SENT) and np.all(hout[bi + m.room:bi + m.room + fo.GUARD] == SENT), (kind, m.name)
    assert L.hipdeflate_stall_count() == 0
    del hin, hout
