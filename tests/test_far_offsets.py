"""far_offsets.py pinned on the CPU: the tiling arithmetic against the real concatenation, and every family's checker
against the MUTANTS -- what a kernel would leave whose offset is masked to 32 bits (the data at X - 2^32, nothing at X),
kept in a signed 32-bit word, or whose gzip ISIZE is the full length.  A checker that passes a mutant is a bug in the test.
No GPU; the fake address space is far_offsets.Sparse (pages), or the whole scheme at a scaled-down "2^32"."""
import zlib

import numpy as np
import pytest

import far_framed as ff
import far_offsets as fo
import hdtest
import member_index_model as mm
import stream_model as sm

BIG = fo.P32 + (1 << 31) + (64 << 20)                # the buffers of test_gpu_far_offsets.py
MUTANTS = [fo.mask32, fo.signed31]


# ---- placement and regions -------------------------------------------------------------------------------------------

def test_edge_offsets_are_the_stated_ones():
    rows = {r.kind: r for rd in fo.rounds(BIG, [(k, 1000) for k in fo.EDGES + ("low",)]) for r in rd}
    assert rows["ends_at"].offset + 1000 == 2 ** 32 and rows["straddle"].offset == 2 ** 32 - 100
    assert rows["starts_at"].offset == 2 ** 32 and rows["plus1"].offset == 2 ** 32 + 1
    assert rows["high"].offset == 2 ** 32 + 2 ** 31 + 7 and rows["end"].offset + 1000 + fo.GUARD == BIG
    assert rows["low"].offset + 1000 < 2 ** 31
    assert [fo.is_far(r.offset, r.length) for r in rows.values()] == [True] * 6 + [False]


def test_rounds_keep_each_boundary_block_alone_and_every_block_once():
    blocks = [("low", 50), ("ends_at", 70000), ("high", 9), ("straddle", 300), ("starts_at", 5), ("end", 40), ("plus1", 77),
              ("high", 1), ("low", 8)]
    rds = fo.rounds(BIG, blocks)
    assert sorted(r.index for rd in rds for r in rd) == list(range(len(blocks)))
    assert [sum(r.kind in fo.BOUNDARY for r in rd) for rd in rds] == [1, 1, 1, 1]
    with pytest.raises(AssertionError):
        fo.place(BIG, [("ends_at", 10), ("ends_at", 10)])
    with pytest.raises(AssertionError):
        fo.place(BIG, [("straddle", 300), ("starts_at", 10)])                # they overlap


def test_regions_guard_both_ends_and_every_alias_and_refuse_a_block_in_an_alias():
    rows = fo.place(BIG, [("straddle", 5000), ("high", 300), ("low", 100), ("end", 64)])
    regs = fo.regions(rows, BIG)
    labels = [r.label for r in regs]
    for r in rows:
        if r.kind != "low":
            assert "in front of %d" % r.offset in labels and "behind %d" % r.offset in labels
            assert "alias 1 of %d" % r.offset in labels
    assert not [r for r in labels if str(rows[2].offset) in r]               # the low control needs none
    by = {r.label: r for r in regs}
    assert (by["alias 1 of %d" % rows[0].offset].begin, by["alias 1 of %d" % rows[0].offset].end) == (0, 4900 + fo.GUARD)
    a = by["alias 1 of %d" % rows[1].offset]
    assert (a.begin, a.end) == (2 ** 31 + 7 - fo.GUARD, 2 ** 31 + 7 + 300 + fo.GUARD)
    for r in regs:                                                           # no region covers a byte of a block
        for w in rows:
            assert r.end <= w.offset or r.begin >= w.offset + w.length
    with pytest.raises(AssertionError, match="alias"):
        fo.regions([(2 ** 32 + 8, 100), (50, 100)], BIG)
    # a buffer past 2^33 has a second alias
    assert fo.aliases(2 ** 33 + 5, 10) == [(2 ** 32 + 5, 2 ** 32 + 15), (5, 15)]


def test_sparse_memory_reads_back_what_was_written():
    m = fo.Sparse(BIG)
    data = bytes(range(256)) * 40
    m[2 ** 32 - 100:2 ** 32 - 100 + len(data)] = data
    assert bytes(m[2 ** 32 - 100:2 ** 32 - 100 + len(data)]) == data
    assert bytes(m[2 ** 32 - 101:2 ** 32 - 100]) == b"\x3c" and len(m.pages) <= 4
    m[5:9] = 7
    assert bytes(m[4:10]) == b"\x3c\x07\x07\x07\x07\x3c"


# ---- the mutants: blocks at offsets (families A, B, C, D, G and the ranged reads of E) ---------------------------------

def _copy_kernel(src, dst, in_rows, out_rows, read=fo.exact, write=fo.exact):
    """a stand-in for any kernel that reads block i at in_rows[i] and writes its result at out_rows[i]"""
    for (i_off, n), (o_off, _) in zip(in_rows, out_rows):
        dst.write(o_off, src.read(i_off, n, read), write)


def _blocks_case(seed):
    """a shuffled table over blocks at every edge of both buffers, low controls among them, one round per boundary kind
    -> [(data, in_rows, out_rows)]"""
    rng = np.random.default_rng(seed)
    kinds = ["low", "ends_at", "high", "end", "low", "straddle", "high", "starts_at", "end", "low", "plus1", "high"]
    lens = [int(rng.integers(1, 70000)) for _ in kinds]
    datas = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    ins = fo.rounds(BIG, list(zip(kinds, lens)))
    shifted = kinds[5:] + kinds[:5]                                     # outputs: another edge than the input's
    outs = fo.rounds(BIG, list(zip(shifted, lens[5:] + lens[:5])))
    return datas, ins, outs, lens


@pytest.mark.parametrize("side", ["read", "write"])
@pytest.mark.parametrize("mutant", [fo.exact] + MUTANTS, ids=lambda f: f.__name__)
def test_block_checker_rejects_every_address_mutant(mutant, side):
    datas, ins, _, lens = _blocks_case(3)
    caught = set()
    for rd in ins:                                                       # one launch per round
        out_rows = fo.place(BIG, [(r.kind, r.length) for r in rd])       # outputs at the same edges
        src, dst = fo.Sparse(BIG), fo.Sparse(BIG)
        in_regs = fo.regions(rd, BIG)
        out_regs = fo.regions(out_rows, BIG)
        fo.fill(src, in_regs)
        fo.fill(dst, out_regs)
        for r in rd:
            src[r.offset:r.offset + r.length] = datas[r.index]
        _copy_kernel(src, dst, [(r.offset, r.length) for r in rd], [(r.offset, r.length) for r in out_rows],
                     **{side: mutant})
        bad = fo.check_rows(dst, [(o.offset, datas[r.index]) for r, o in zip(rd, out_rows)], out_regs)
        if mutant is fo.exact:
            assert bad == []
            continue
        far = [k for k, r in enumerate(rd) if mutant(r.offset) != r.offset]   # (the straddling block's own offset is below 2^32:
        if not far:                                                          # test_block_checker_rejects_an_address_that_wraps_inside_a_block)
            assert bad == []
            continue
        assert {b[1] for b in bad if b[0] == "row"} == set(far), (rd, bad)      # every far row, no other
        if side == "write" and any(fo.mask32(rd[k].offset) + rd[k].length <= BIG and mutant(rd[k].offset) >= 0 for k in far):
            assert [b for b in bad if b[0] == "guard"], "the alias sentinels saw nothing"
        caught |= {rd[k].kind for k in far}
    if mutant is not fo.exact:
        assert caught >= {"starts_at", "plus1", "high", "end"}                # (a signed word also loses [2^31, 2^32))


def test_block_checker_rejects_an_address_that_wraps_inside_a_block():
    """the straddling block starts below 2^32: what it catches is an address that is advanced in 32 bits -- every 16
    bytes placed by the low half of their own address"""
    rng = np.random.default_rng(9)
    data = bytes(rng.integers(0, 256, 5000, dtype=np.uint8))
    (row,) = fo.place(BIG, [("straddle", len(data))])
    regs = fo.regions([row], BIG)
    for mutant in (fo.exact, fo.mask32):
        dst = fo.Sparse(BIG)
        fo.fill(dst, regs)
        for at in range(0, len(data), 16):
            dst.write(row.offset + at, data[at:at + 16], mutant)
        bad = fo.check_rows(dst, [(row.offset, data)], regs)
        assert (bad == []) == (mutant is fo.exact)
        assert mutant is fo.exact or {b[0] for b in bad} == {"row", "guard"}


@pytest.mark.parametrize("mutant", [fo.exact] + MUTANTS, ids=lambda f: f.__name__)
def test_stride_checker_rejects_a_narrow_row_times_stride(mutant):
    """family A / B: member i at i * out_stride, stride 256 MiB + 16, 24 rows -- rows 0..7 tiny, so that no block lies in
    the alias of rows 16..23"""
    stride, nrows = (256 << 20) + 16, 24
    rng = np.random.default_rng(5)
    members = [bytes(rng.integers(0, 256, 40 if i < 8 else 3000 + i, dtype=np.uint8)) for i in range(nrows)]
    rows = [(i * stride, len(m)) for i, m in enumerate(members)]
    assert rows[16][0] == 2 ** 32 + 256
    regs = fo.regions(rows, nrows * stride)
    dst = fo.Sparse(nrows * stride)
    fo.fill(dst, regs)
    for (off, _), m in zip(rows, members):
        dst.write(off, m, mutant)
    bad = fo.check_rows(dst, [(o, m) for (o, _), m in zip(rows, members)], regs)
    if mutant is fo.exact:
        assert bad == []
    else:
        assert {b[1] for b in bad if b[0] == "row"} >= set(range(16, 24))
        assert mutant is fo.signed31 or len([b for b in bad if b[0] == "guard"]) >= 8


def test_table_checker_rejects_narrow_entries():
    want = [5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 2 ** 31 + 7, 2 ** 40 + 5]
    assert fo.check_table(want, want) == []
    for mutant in MUTANTS:
        got = [mutant(v) % 2 ** 64 for v in want]
        assert fo.check_table(got, want)[0][1] == min(i for i, v in enumerate(want) if mutant(v) != v)
    assert fo.check_table(want[:-1], want)


# ---- tiling arithmetic: containers -----------------------------------------------------------------------------------

def _container_tiles(total=700000):
    rng = np.random.default_rng(21)
    s = hdtest.synth()
    noise = [bytes(rng.integers(0, 256, 0xff00, dtype=np.uint8)) for _ in range(6)]
    text = bytes(s.text_like(30000, seed=1))
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    text_member = mm.gz_member("BC", z.compress(text) + z.flush(), zlib.crc32(text), len(text))
    base = fo.container_tile([(fo.stored_member("BC", d), d) for d in noise] + [(text_member, text)], total, rng)
    lead, lead_data = fo.pad_member(123457, rng)                         # the variant: a member starts at 123457 exactly
    others = [(fo.stored_member(k, noise[i][:20000 + i], fname=b"n" if i & 1 else b""), noise[i][:20000 + i])
              for i, k in enumerate(["MZ", "IG1", "IG2", "MG", "BC"])]
    variant = fo.container_tile([(lead, lead_data)] + others, total, rng)
    return base, variant


def test_pad_member_has_exactly_its_size_and_inflates():
    rng = np.random.default_rng(1)
    for total in (33, 34, 100, 65535 + 33, 65535 + 34, 65535 + 38, 65535 + 39, 200000, 2 * 65535 + 20 + 8 + 10 + 3):
        m, data = fo.pad_member(total, rng)
        assert len(m) == total and zlib.decompress(m, 31) == data
        assert mm.walk(m) == ([(20, total - 20, len(data), 0, zlib.crc32(data))], mm.OK, total)


def test_extended_member_table_is_the_walk_of_the_real_concatenation():
    (base, base_data), (variant, var_data) = _container_tiles()
    assert len(base) == len(variant) == 700000
    tables = {"base": (mm.walk(base)[0], len(base)), "variant": (mm.walk(variant)[0], len(variant))}
    assert mm.walk(variant)[0][1][0] - fo.MEMBER_HEADER["MZ"] == 123457    # the member behind the lead starts there
    for order in (["base"] * 3, ["base", "variant", "base"], ["variant", "base", "base", "variant"]):
        blob = b"".join(base if o == "base" else variant for o in order)
        data = b"".join(base_data if o == "base" else var_data for o in order)
        ext = fo.extend_member_table(tables, order)
        rows, n, out_bytes, end, status = mm.summary(blob, 10 ** 6)
        assert status == mm.OK and (ext["nmembers"], ext["out_bytes"], ext["end_offset"]) == (n, out_bytes, end)
        assert fo.table_rows(ext) == rows
        assert out_bytes == len(data)
        # ... and the contents are the tiles' contents in the same order (what `run` is held to, tile by tile)
        out = bytearray()
        rest = blob
        while rest:
            d = zlib.decompressobj(31)
            out += d.decompress(rest)
            rest = d.unused_data
        assert bytes(out) == data


# ---- tiling arithmetic: streams --------------------------------------------------------------------------------------

def _stream_tile(level=6, frame=sm.FRAME_GZIP, chunk=4096, chunks=5):
    s = hdtest.synth()
    rng = np.random.default_rng(8)
    noise = bytes(rng.integers(0, 256, chunk, dtype=np.uint8))
    text = bytes(s.text_like(chunk * 2, seed=2))
    tile = (noise + text[:chunk] + noise + text[chunk:] + bytes(chunk))[:chunk * chunks]
    return fo.StreamTile(tile, level, frame, chunk)


@pytest.mark.parametrize("frame", [sm.FRAME_RAW, sm.FRAME_ZLIB, sm.FRAME_GZIP])
@pytest.mark.parametrize("level", [1, 6])
def test_tiled_stream_is_the_model_of_the_real_concatenation(level, frame):
    t = _stream_tile(level, frame)
    n_tile = len(t.tile)
    for nbytes in (3 * n_tile, 3 * n_tile + 48, 2 * n_tile + 4096, 2 * n_tile + 2 * 4096 + 1, 48, 0):
        data = (t.tile * 4)[:nbytes]
        stream, off, summary = sm.encode(data, level, frame, 4096)
        e = t.expected(nbytes)
        assert t.assemble(nbytes) == stream and e["chunk_off"].tolist() == off and e["summary"] == summary
        d = zlib.decompressobj(sm.WBITS[frame])
        assert d.decompress(stream) == data and d.eof
        mem = np.frombuffer(stream, dtype=np.uint8)
        assert fo.check_stream(mem, e, t.stream) == []


@pytest.mark.parametrize("kind", [sm.CRC32, sm.ADLER32])
def test_fold_of_the_tile_checks_is_zlibs_checksum_of_the_concatenation(kind):
    t = _stream_tile(1, sm.FRAME_ZLIB if kind == sm.ADLER32 else sm.FRAME_GZIP)
    for repeats in (1, 2, 7, 40):
        real = t.tile * repeats + t.tile[:48]
        assert t.expected(len(real))["summary"]["check"] == (zlib.adler32(real) if kind == sm.ADLER32 else zlib.crc32(real))


def test_isize_is_the_length_mod_2_32_and_the_checker_rejects_the_full_length():
    """the stream of test_gpu_far_offsets.py's family F -- 2^32 + 2^29 + 48 bytes -- as numbers alone: a tile of 1 MiB"""
    chunk = 256 << 10
    rng = np.random.default_rng(4)
    tile = bytes(rng.integers(0, 256, 4 * chunk, dtype=np.uint8))
    t = fo.StreamTile(tile, 1, sm.FRAME_GZIP, chunk)
    nbytes = 2 ** 32 + 2 ** 29 + 48
    e = t.expected(nbytes)
    assert e["isize"] == nbytes - 2 ** 32 == fo.gzip_isize(e["tail"]) and e["summary"]["in_bytes"] == nbytes
    assert e["summary"]["out_bytes"] > nbytes and int(e["chunk_off"][-1]) > 2 ** 32
    assert e["summary"]["nchunks"] == 4608 * 4 + 1 == len(e["chunk_off"]) - 1
    # the tail alone in a fake stream: the good one passes, a saturated ISIZE and one of the high half do not
    tail_at = e["summary"]["out_bytes"] - len(e["tail"])

    def problems(tail):
        mem = fo.Sparse(e["summary"]["out_bytes"])
        mem[tail_at:tail_at + len(tail)] = tail
        got = fo.to_bytes(mem[tail_at:tail_at + len(e["tail"])])
        return [] if got == e["tail"] else [("tail", got.hex())]
    assert problems(e["tail"]) == []
    for wrong in (min(nbytes, 0xffffffff), nbytes >> 32, nbytes & 0x7fffffff if nbytes & 0x80000000 else nbytes >> 1):
        bad_tail = e["tail"][:-4] + int(wrong).to_bytes(4, "little")
        assert problems(bad_tail), wrong


# ---- the mutants: tiled families (E: the container's contents, F: the stream) at a scaled-down 2^32 ---------------------

LIMIT = 1 << 20


@pytest.mark.parametrize("mutant", [fo.exact] + MUTANTS, ids=lambda f: f.__name__)
def test_tile_checker_rejects_repeats_written_through_a_narrow_position(mutant):
    rng = np.random.default_rng(12)
    tiles = [bytes(rng.integers(0, 256, 100000, dtype=np.uint8)) for _ in range(2)]
    order = [0] * 10 + [1] + [0] * 5                                      # repeat 10 holds LIMIT: the variant
    assert 10 * 100000 < LIMIT < 11 * 100000
    mem = fo.Sparse(16 * 100000)
    for k, which in enumerate(order):                                     # a writer that places every 1000 bytes by its position
        for at in range(0, 100000, 1000):
            mem.write(k * 100000 + at, tiles[which][at:at + 1000], mutant, LIMIT)
    bad = fo.tiles_damaged(mem, 0, tiles, order)
    if mutant is fo.exact:
        assert bad == []
    else:
        assert set(bad) >= set(range(10, 16))           # (masked, the far repeats also land on the first ones)


@pytest.mark.parametrize("what", ["exact", "chunk position masked", "chunk position signed", "table masked"])
def test_stream_checker_rejects_a_narrow_running_position(what):
    t = _stream_tile(1, sm.FRAME_GZIP, chunk=16384, chunks=5)            # noise-heavy: the stream grows like the input
    nbytes = 32 * len(t.tile) + 48
    e = t.expected(nbytes)
    assert e["summary"]["out_bytes"] > LIMIT + LIMIT // 2 and int(e["chunk_off"][-1]) > LIMIT
    address = {"chunk position masked": fo.mask32, "chunk position signed": fo.signed31}.get(what, fo.exact)
    mem = fo.Sparse(e["summary"]["out_bytes"])
    mem.write(0, e["header"])
    per = len(t.coded)
    chunks = t.coded * e["repeats"] + [e["rest"]]
    assert len(chunks) == len(e["chunk_off"]) - 1
    for off, c in zip(e["chunk_off"].tolist(), chunks):
        mem.write(off, c, address, LIMIT)
    mem.write(int(e["chunk_off"][-1]), e["tail"], address, LIMIT)
    table = [fo.mask32(v, LIMIT) if what == "table masked" else v for v in e["chunk_off"].tolist()]
    bad = fo.check_stream(mem, e, t.stream) + fo.check_table(table, e["chunk_off"], "chunk_off")
    assert (bad == []) == (what == "exact"), bad
    assert per == 5


# ---- the framed family (D2, G2): the layout through a stand-in, the trailer's address through the mutants ---------------

def _framed_standin(src, dst, frame, launch, caps, trailer=fo.exact, header_len=fo.exact):
    """a stand-in for hipdeflate_batch_inflate_framed_dev: the member is read at in_off, framed_model.framed decides --
    but the trailer is fetched the way k_frame_close fetches it, byte by byte at (in_off + header) + consumed + k, through
    `trailer`; header_len stands for the narrowing of p_off - in_off on the way into in_used"""
    M = ff.M
    got = []
    for p, cap in zip(launch, caps):
        m = src.read(p.a.offset, p.a.length)
        pos, foot = M.open_member(m, frame), M.FOOTER[frame]
        if pos is not None and foot:
            r, _, bits = M.oracle_inflate_bits(m[pos:len(m) - foot], cap)
            if r == 0:
                at = pos + (bits + 7) // 8
                t = b"".join(src.read(p.a.offset + at + k, 1, trailer) for k in range(foot))
                m = m[:at] + t + m[at + foot:]
        st, n, used, check, data = M.framed(m, frame, cap)
        if st == 0:
            p_off = p.a.offset + pos
            used = header_len(p_off - p.a.offset) + (used - pos)
            dst.write(p.b.offset, data)
        got.append((st, n, used, check))
    return got


def _standin_launch(frame, launch, short=None, **how):
    src, dst = fo.Sparse(ff.BIG), fo.Sparse(ff.BIG)
    caps = ff.caps_of(launch, short)
    in_regs, regs = ff.lay_input(src, launch), ff.lay_output(dst, launch, caps)
    sizes = [ff.M.size(src.read(p.a.offset, p.a.length), frame) for p in launch]
    got = _framed_standin(src, dst, frame, launch, caps, **how)
    return ff.size_problems(launch, sizes) + ff.framed_problems(launch, caps, got, dst, regs, src, in_regs)


@pytest.mark.parametrize("frame", [0, 4, 5], ids=["raw", "zlib", "gzip"])
def test_framed_layout_passes_its_own_expectations_through_an_exact_stand_in(frame):
    """section D2's layout, members and checker without a GPU: every launch, the launches with out_cap one short, and the
    conditions that keep it a far-offset test"""
    launches = ff.launches(frame)
    refused_far = ff.honest(launches)
    assert refused_far >= (8 if frame == ff.M.GZIP else 4)
    assert [len(l) for l in launches] == [8, 8, 8, 8] + [4] * (frame == ff.M.GZIP)
    for launch in launches:
        assert _standin_launch(frame, launch) == []
        for p in launch:
            if p.case.name in ("crc_flip", "isize_flip", "adler_flip", "bad_id", "reserved", "no_nul", "bad_fcheck", "cut1"):
                assert ff.want_framed(p.case, p.case.room)[:4] == (1, 0, 0, 0) and p.a.offset >= fo.P32, p.case.name
            if p.case.name == "garbage7":
                assert ff.want_framed(p.case, p.case.room)[2] == len(p.case.data) - 7
            if p.case.name == "pair":
                assert ff.want_size(p.case)[2] == len(p.case.data) - len(p.case.follow[0])
    for launch in launches[:2]:                       # the boundary outputs at 2^32 - 100 and at 2^32, one byte short
        short = ff.boundary_position(launch)
        assert launch[short].b.kind in ("straddle", "starts_at")
        assert _standin_launch(frame, launch, short=short) == []
        assert ff.want_framed(launch[short].case, launch[short].case.room - 1)[:4] == (3, 0, 0, 0)
    if frame == ff.M.GZIP:
        by = {p.case.name: p for l in launches for p in l if p.a.kind in fo.BOUNDARY}
        assert by["name300"].a.offset == 2 ** 32 - 100 and by["extra65535"].a.offset + len(by["extra65535"].case.data) == 2 ** 32
        assert ff.M.open_member(by["name300"].case.data, frame) == 311 and ff.M.open_member(by["extra65535"].case.data, frame) == 12 + 65535


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_framed_checker_rejects_a_narrow_trailer_address(mutant):
    """the one address of the framed family the block cases do not have: the gzip member of 104 bytes from 2^32 - 100 has its
    CRC-32 below 2^32 and its ISIZE at it, the zlib member of 102 bytes its Adler-32 cut 2 | 2.  A trailer read byte by byte
    through a narrowed address finds the alias sentinels (or nothing) where the upper bytes should be."""
    for frame, name in ((ff.M.GZIP, "g104"), (ff.M.ZLIB, "z102")):
        launch = next(l for l in ff.launches(frame) if any(p.case.name == name and p.a.kind == "straddle" for p in l))
        p = next(p for p in launch if p.case.name == name)
        assert p.a.offset == 2 ** 32 - 100 and p.a.offset + p.a.length == 2 ** 32 + (4 if frame == ff.M.GZIP else 2)
        assert _standin_launch(frame, launch) == []
        bad = _standin_launch(frame, launch, trailer=mutant)
        caught = {b[1] for b in bad if b[0] == "framed"}
        far_ok = {q.case.name for q in launch if q.a.offset >= fo.P32 and ff.want_framed(q.case, q.case.room)[0] == 0}
        assert name in caught and caught >= far_ok, (frame, bad)


def test_in_used_may_narrow_the_header_length():
    """k_frame_close and k_inflate_size form in_used from (uint32_t)(p_off - in_off): the narrowing of a DIFFERENCE of two
    64-bit offsets of one member, which is the header's length (< 2^28) whatever the offsets are.  mask32 on it changes
    nothing -- this is not a narrowed address and needs no fix."""
    for frame in ff.FRAMES:
        for launch in ff.launches(frame):
            assert _standin_launch(frame, launch, header_len=fo.mask32) == []


@pytest.mark.parametrize("frame", [0, 4, 5], ids=["raw", "zlib", "gzip"])
def test_long_streams_in_a_frame_are_what_the_gpu_tests_take_them_for(frame):
    """section G2 and H rest on members whose check value and ISIZE are by construction: the same wrapping at a scale zlib
    and the model can follow"""
    import framed_model as M
    over = fo.LONG_OVERHEAD[frame]
    host, pattern, reps, rest = fo.long_input_stream(200000 - over, np.random.default_rng(28))
    member, check, total = fo.framed_long_member(frame, host, pattern, reps, rest)
    m = member.tobytes()
    plain = pattern.tobytes() * reps + rest
    assert len(m) == 200000 and total == len(plain) and zlib.decompress(m, sm.WBITS[frame]) == plain
    assert M.size(m, frame) == (0, total, 200000) and M.framed(m, frame, total)[:4] == (0, total, 200000, check)
    if frame == M.GZIP:
        off = m[:-4] + ((total + 1) & 0xffffffff).to_bytes(4, "little")
        assert M.size(off, frame) == (1, 0, 0)
    total = 32768 * 8
    stream, pattern = fo.long_output_stream(total)
    member, check, n = fo.framed_long_member(frame, stream, pattern, 8)
    m = member.tobytes()
    assert n == total and zlib.decompress(m, sm.WBITS[frame]) == pattern.tobytes() * 8
    assert M.size(m, frame) == (0, total, len(m)) and M.framed(m, frame, total)[:4] == (0, total, len(m), check)
    assert M.framed(m, frame, total - 1)[:4] == (3, 0, 0, 0)
