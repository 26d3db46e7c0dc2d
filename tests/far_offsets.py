"""Test data at and past offset 2^32 of a device buffer, for a few seconds a test (the GPU half: test_gpu_far_offsets.py;
the helper itself is pinned on the CPU by test_far_offsets.py).  Nothing here calls a kernel.

Every device entry point of include/hipdeflate.h takes 64-bit offsets and sizes.  An offset X that loses its upper half on
the way to an address lands at X - 2^32 (kept in an int32 it lands there too while X < 2^32 + 2^31, and below the buffer
beyond that).  What shows it:

  * sparse placement -- the big buffer is never filled; a handful of small blocks sit at the EDGE offsets (ending exactly
    at 2^32, straddling it from 2^32 - 100, starting exactly at it, at 2^32 + 1, at 2^32 + 2^31 + 7, near the buffer's
    end), low-offset controls among them, and the table points at them in shuffled order: place(), rounds();
  * alias sentinels -- a guard of SENT bytes in front of and behind every far block and over its whole extent at
    X - 2^32 (and X - 2^33 where that is inside the buffer), filled before the call and intact behind it: regions(),
    fill(), damaged() / intact().  No legitimate block may lie in such a region: regions() refuses the layout otherwise;
  * tiling -- a container or a stream past 4 GiB is a tile repeated on the device; the expected table of R repeats is the
    tile's table plus k * tile_len (extend_member_table), the expected stream, chunk table and summary come from the
    tile's per-chunk bytes and stream_model.fold (StreamTile), and bytes are compared repeat by repeat (tiles_damaged).

`mem` is anything that slices like a flat uint8 array: a numpy array, a torch tensor on the device, or Sparse (a paged
fake address space, so that the CPU tests can put a byte at 2^32 + 2^31 + 7 without owning 6 GiB).  `limit` stands for
2^32 throughout; the CPU tests also run the tiled families at a scaled-down limit."""
import collections
import struct
import zlib

import numpy as np

import member_index_model as mm
import stream_model as sm

P32 = 1 << 32
SENT = 0xA5
GUARD = 4096
BOUNDARY = ("ends_at", "straddle", "starts_at", "plus1")        # the four that touch the limit: one per buffer and round
EDGES = BOUNDARY + ("high", "end")
STRADDLE = 100                                                    # the straddling block starts this far below the limit

Row = collections.namedtuple("Row", "index offset length kind")
Region = collections.namedtuple("Region", "begin end label")


def edge_offset(kind, length, buffer_size, limit=P32, guard=GUARD):
    """where a block of `length` bytes of edge kind `kind` starts"""
    at = {"ends_at": limit - length, "straddle": limit - STRADDLE, "starts_at": limit, "plus1": limit + 1,
          "high": limit + limit // 2 + 7, "end": buffer_size - length - guard, "low": limit // 512 + 3}[kind]
    assert 0 <= at and at + length + (guard if kind == "end" else 0) <= buffer_size, (kind, at, length, buffer_size)
    return at


def place(buffer_size, blocks, limit=P32, guard=GUARD):
    """blocks: [(kind, length)], kind one of EDGES or "low" -> [Row] in the blocks' order.  A boundary kind may appear
    once; further "high" and "low" blocks follow the first upwards, further "end" blocks downwards, 2 * guard + 1 apart
    (so that guards fit between them and alignments differ).  No two blocks overlap: the layout is refused otherwise."""
    rows, nxt = [], {}
    for i, (kind, length) in enumerate(blocks):
        if kind in nxt:
            assert kind not in BOUNDARY, "one %s block per placement" % kind
            at = nxt[kind] - length if kind == "end" else nxt[kind]
        else:
            at = edge_offset(kind, length, buffer_size, limit, guard)
        nxt[kind] = at - 2 * guard - 1 if kind == "end" else at + length + 2 * guard + 1
        assert 0 <= at and at + length <= buffer_size, (kind, at, length)
        rows.append(Row(i, at, length, kind))
    spans = sorted((r.offset, r.offset + r.length) for r in rows if r.length)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "blocks overlap: [%d, %d) and [%d, %d)" % (a0, a1, b0, b1)
    return rows


def rounds(buffer_size, blocks, limit=P32, guard=GUARD):
    """blocks as for place() -> [[Row]]: the blocks dealt into as few placements as keep each boundary kind alone at the
    boundary (its guards would lie in a neighbour otherwise); every round also gets the non-boundary blocks that follow
    its boundary block in `blocks`, so a round is a far block, the controls and the other edges"""
    out, cur = [], []
    for i, (kind, length) in enumerate(blocks):
        if kind in BOUNDARY and any(k in BOUNDARY for _, (k, _) in cur):
            out.append(cur)
            cur = []
        cur.append((i, (kind, length)))
    if cur:
        out.append(cur)
    return [[Row(i, r.offset, r.length, r.kind) for (i, _), r in zip(c, place(buffer_size, [b for _, b in c], limit, guard))]
            for c in out]


def is_far(offset, length, limit=P32):
    """does [offset, offset + length) hold a byte at or past the limit (or end exactly at it)"""
    return offset + length >= limit


def aliases(offset, length, limit=P32):
    """[(begin, end)]: where a block at `offset` lands when its offset loses a multiple of `limit`, clipped at 0"""
    out, k = [], 1
    while offset + length - k * limit > 0:
        out.append((max(0, offset - k * limit), offset + length - k * limit))
        k += 1
    return out


def _subtract(span, holes):
    """the parts of span = (a, b) outside every (h0, h1) of holes"""
    parts = [span]
    for h0, h1 in holes:
        parts = [p for a, b in parts for p in ((a, min(b, h0)), (max(a, h1), b)) if p[0] < p[1]]
    return parts


def regions(rows, buffer_size, limit=P32, guard=GUARD, others=(), ends=True, alias=True):
    """the guard regions of a placement: for every far row `guard` bytes in front of and behind it (cut where a
    neighbouring block lies) and its whole extent, `guard` more on either side, at each alias.  rows: [(offset, length)]
    or [Row]; others: further legitimate spans [(offset, length)] of the same buffer that are not far outputs themselves.
    A legitimate block inside an alias region is a mistake of the layout: refused.  ends / alias: leave either sort out
    (an encoder may use its whole ROOM, so the guards at the ends belong to the rooms and the aliases to the members)."""
    spans = [(r.offset, r.length) if isinstance(r, Row) else tuple(r) for r in rows]
    legit = [(o, o + n) for o, n in list(spans) + [tuple(x) for x in others] if n]
    out = []
    for o, n in spans:
        if not is_far(o, n, limit):
            continue
        for a, b in _subtract((max(0, o - guard), o), legit) if ends else ():
            out.append(Region(a, b, "in front of %d" % o))
        for a, b in _subtract((o + n, min(buffer_size, o + n + guard)), legit) if ends else ():
            out.append(Region(a, b, "behind %d" % o))
        for k, (a, b) in enumerate(aliases(o, n, limit) if alias else ()):
            a, b = max(0, a - guard), min(buffer_size, b + guard)
            core = (max(0, o - (k + 1) * limit), o + n - (k + 1) * limit)
            for l0, l1 in legit:
                assert l1 <= core[0] or l0 >= core[1], "block [%d, %d) lies in the alias of %d" % (l0, l1, o)
            for a2, b2 in _subtract((a, b), legit):
                out.append(Region(a2, b2, "alias %d of %d" % (k + 1, o)))
    return out


def fill(mem, regs, value=SENT):
    for r in regs:
        mem[r.begin:r.end] = value


def _all_equal(view, value):
    return bool((view == value).all())


def damaged(regs, mem, value=SENT):
    """the regions of regs that do not hold `value` in every byte"""
    return [r for r in regs if not _all_equal(mem[r.begin:r.end], value)]


def intact(regs, mem, value=SENT):
    return not damaged(regs, mem, value)


def to_bytes(view):
    """a slice of mem -> bytes"""
    if isinstance(view, (bytes, bytearray)):
        return bytes(view)
    if hasattr(view, "cpu"):
        view = view.cpu().numpy()
    return bytes(np.asarray(view, dtype=np.uint8))


def check_rows(mem, expected, regs):
    """the checker of every family whose output is blocks at offsets (encode slots, inflate outputs, gathered members,
    range queries): expected = [(offset, bytes)] -> [problem]; no problem means every block is at its offset, byte for
    byte, and every guard and alias region is intact"""
    bad = [("row", i, off) for i, (off, want) in enumerate(expected) if to_bytes(mem[off:off + len(want)]) != bytes(want)]
    return bad + [("guard", r.label, r.begin) for r in damaged(regs, mem)]


def check_table(got, want, what="table"):
    """the checker of every family whose output is numbers (dst_off, the index's tables, chunk_off, summary fields):
    -> [problem]; got / want: equal-length sequences or arrays of ints"""
    g, w = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    if g.shape != w.shape:
        return [(what, "shape", g.shape, w.shape)]
    diff = np.flatnonzero(g != w)
    return [(what, int(diff[0]), int(g[diff[0]]), int(w[diff[0]]))] if len(diff) else []


def tiles_damaged(mem, start, tiles, order, equal=None):
    """the checker of the tiled families: repeat k of the data at `start` is tiles[order[k]] (all tiles of one length)
    -> [k] of the repeats that differ.  equal(view, tile): torch.equal for device tensors, bytes by default"""
    equal = equal or (lambda v, t: to_bytes(v) == to_bytes(t))
    n = len(tiles[0])
    return [k for k, which in enumerate(order) if not equal(mem[start + k * n:start + (k + 1) * n], tiles[which])]


# ---- address mutants: what a kernel with a narrowed offset would do (test_far_offsets.py) --------------------------

def exact(x, limit=P32):
    return x


def mask32(x, limit=P32):
    """the offset's low half alone"""
    return x % limit


def signed31(x, limit=P32):
    """the offset kept in a signed word: past limit / 2 it is negative, i.e. below the buffer"""
    v = x % limit
    return v - limit if v >= limit // 2 else v


class Sparse:
    """a paged fake address space of `size` bytes; unwritten bytes read as `background`.  Slices only."""
    PAGE = 1 << 12

    def __init__(self, size, background=0x3c):
        self.size, self.background, self.pages = size, background, {}

    def _span(self, sl):
        a, b, step = sl.indices(self.size)
        assert step == 1 and 0 <= a <= b <= self.size
        return a, b

    def __setitem__(self, sl, value):
        a, b = self._span(sl)
        v = np.broadcast_to(np.frombuffer(value, dtype=np.uint8) if isinstance(value, (bytes, bytearray)) else
                            np.asarray(value, dtype=np.uint8), (b - a,))
        at = a
        while at < b:
            p, o = divmod(at, self.PAGE)
            n = min(self.PAGE - o, b - at)
            page = self.pages.setdefault(p, np.full(self.PAGE, self.background, dtype=np.uint8))
            page[o:o + n] = v[at - a:at - a + n]
            at += n

    def __getitem__(self, sl):
        a, b = self._span(sl)
        out = np.full(b - a, self.background, dtype=np.uint8)
        at = a
        while at < b:
            p, o = divmod(at, self.PAGE)
            n = min(self.PAGE - o, b - at)
            if p in self.pages:
                out[at - a:at - a + n] = self.pages[p][o:o + n]
            at += n
        return out

    def write(self, offset, data, address=exact, limit=P32):
        """what a kernel that forms its address with `address` does with data meant for `offset`: the bytes land at
        address(offset) -- or nowhere, where that is outside the buffer (the real thing would fault)"""
        at = address(offset, limit)
        if 0 <= at and at + len(data) <= self.size:
            self[at:at + len(data)] = data

    def read(self, offset, length, address=exact, limit=P32):
        at = address(offset, limit)
        if 0 <= at and at + length <= self.size:
            return bytes(self[at:at + length])
        return bytes(length)


# ---- tiling arithmetic: containers ----------------------------------------------------------------------------------

def extend_member_table(tables, order):
    """tables: {name: (rows, tile_len)} with rows = member_index_model.walk() of one tile (a whole number of members,
    tile_len bytes); order: the tile name of every repeat (the tiles that stand in for one another have one length)
    -> dict of numpy uint64 arrays in_off, in_len, out_size, out_off, crc and the ints nmembers, out_bytes, end_offset:
    what the walk gives on the concatenation"""
    cols = {n: np.array(rows, dtype=np.uint64).reshape(len(rows), 5) for n, (rows, _) in tables.items()}
    parts, pos, out = [], 0, 0
    for name in order:
        c = cols[name].copy()
        c[:, 0] += np.uint64(pos)
        c[:, 3] += np.uint64(out)
        parts.append(c)
        pos += tables[name][1]
        out += int(cols[name][:, 2].sum())
    t = np.concatenate(parts) if parts else np.zeros((0, 5), dtype=np.uint64)
    return {"in_off": t[:, 0], "in_len": t[:, 1], "out_size": t[:, 2], "out_off": t[:, 3], "crc": t[:, 4],
            "nmembers": len(t), "out_bytes": out, "end_offset": pos}


def table_rows(ext):
    """the extended table as the row tuples member_index_model / range_read_model work on"""
    return list(zip(*(ext[k].tolist() for k in ("in_off", "in_len", "out_size", "out_off", "crc"))))


MEMBER_HEADER = {"BC": 18, "MZ": 20, "IG1": 32, "IG2": 20, "MG": 16}


def stored_payload(data, blocks=None):
    """raw DEFLATE of stored blocks alone, the last one final; blocks: how many (default: as few as hold the data)"""
    data = bytes(data)
    nb = max(1, -(-len(data) // 65535)) if blocks is None else blocks
    assert nb >= 1 and len(data) <= 65535 * nb
    base, extra = divmod(len(data), nb)
    out, at = [], 0
    for k in range(nb):
        n = base + (1 if k < extra else 0)
        out.append(bytes([1 if k == nb - 1 else 0]) + struct.pack("<HH", n, n ^ 0xffff) + data[at:at + n])
        at += n
    return b"".join(out)


def stored_member(kind, data, **kw):
    """a member of the given kind that holds `data` in stored blocks: member ~ data, so a blob of them passes 2^32 when
    its contents do"""
    return mm.gz_member(kind, stored_payload(data), zlib.crc32(data), len(data), **kw)


def pad_member(total, rng, kind="MZ"):
    """a decodable member of exactly `total` bytes (noise in stored blocks): what puts the next member where it is wanted"""
    room = total - MEMBER_HEADER[kind] - 8
    nb = 1
    while room - 5 * nb > 65535 * nb:
        nb += 1
    n = room - 5 * nb
    assert n >= 0, "no member of %d bytes" % total
    data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    m = mm.gz_member(kind, stored_payload(data, nb), zlib.crc32(data), n)
    assert len(m) == total
    return m, data


def container_tile(members, total, rng):
    """members: [(member bytes, its contents)] -> (tile of exactly `total` bytes: the members and a pad member behind
    them, the tile's contents)"""
    blob = b"".join(m for m, _ in members)
    pad, data = pad_member(total - len(blob), rng)
    return blob + pad, b"".join(d for _, d in members) + data


# ---- tiling arithmetic: streams -------------------------------------------------------------------------------------

class StreamTile:
    """One chunk-aligned tile of input and what stream_model.encode would make of R repeats of it and a ragged rest,
    without ever holding the repeats: the tile's chunks are coded once (the twin's flush form, a chunk that appears
    several times in the tile once), the rest's last chunk once more."""

    def __init__(self, tile, level, frame, chunk):
        import hdtest
        tile = bytes(tile)
        assert len(tile) % chunk == 0 and tile
        self.tile, self.level, self.frame, self.chunk, self.kind = tile, level, frame, chunk, sm.KIND[frame]
        self._twin, self._hdtest = {}, hdtest
        parts = sm.cut(tile, chunk)
        self.coded = [self._code(p) for p in parts]
        self.checks = [sm.part_check(p, self.kind) for p in parts]
        self.stream = b"".join(self.coded)                          # the tile's share of a stream: its chunks, no header

    def _code(self, part):
        if part not in self._twin:
            r, b = self._hdtest.oracle_twin_flush(part, self.level)
            assert r == 0
            self._twin[part] = b
        return self._twin[part]

    def expected(self, nbytes):
        """the stream of the first nbytes of the endlessly repeated tile -> dict: repeats (whole tiles), rest (the coded
        bytes behind them up to the 03 00, the ragged chunk included), chunk_off (numpy uint64, nchunks + 1), tail (03 00
        and the trailer), header, summary (as stream_model.encode's), isize"""
        per, tlen = len(self.coded), len(self.tile)
        repeats, rem = divmod(nbytes, tlen)
        full, ragged = divmod(rem, self.chunk)
        rest = list(self.coded[:full]) + ([self._code(self.tile[full * self.chunk:rem])] if ragged else [])
        rest_lens = [self.chunk] * full + ([ragged] if ragged else [])
        rest_checks = self.checks[:full] + ([sm.part_check(self.tile[full * self.chunk:rem], self.kind)] if ragged else [])
        hdr = sm.HEADER[self.frame]
        sizes = np.array([len(c) for c in self.coded], dtype=np.uint64)
        inside = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes)[:-1]])      # chunk offsets inside a tile
        off = (np.arange(repeats, dtype=np.uint64)[:, None] * np.uint64(len(self.stream)) + inside[None, :]).reshape(-1)
        at = repeats * len(self.stream)
        more = []
        for c in rest:
            more.append(at)
            at += len(c)
        chunk_off = np.concatenate([off, np.array(more + [at], dtype=np.uint64)]) + np.uint64(len(hdr))
        check = sm.fold(self.checks * repeats + rest_checks, [self.chunk] * (per * repeats) + rest_lens, self.kind)
        tail = b"\x03\x00" + sm.trailer(self.frame, check, nbytes)
        nchunks = per * repeats + len(rest)
        out_bytes = len(hdr) + at + len(tail)
        return {"repeats": repeats, "rest": b"".join(rest), "chunk_off": chunk_off, "tail": tail, "header": hdr,
                "isize": nbytes % P32,
                "summary": {"out_bytes": out_bytes, "in_bytes": nbytes, "bad_chunk": nchunks, "nchunks": nchunks,
                            "check": check, "status": 0}}

    def assemble(self, nbytes):
        """the whole expected stream as bytes (small cases only)"""
        e = self.expected(nbytes)
        return e["header"] + self.stream * e["repeats"] + e["rest"] + e["tail"]


def check_stream(mem, exp, tile_stream, equal=None):
    """the checker of the stream family: mem holds header | R x tile_stream | rest | 03 00 | trailer -> [problem]"""
    hdr, n = len(exp["header"]), len(tile_stream)
    bad = []
    if to_bytes(mem[:hdr]) != exp["header"]:
        bad.append(("header",))
    bad += [("repeat", k) for k in tiles_damaged(mem, hdr, [tile_stream], [0] * exp["repeats"], equal)]
    at = hdr + exp["repeats"] * n
    if to_bytes(mem[at:at + len(exp["rest"])]) != exp["rest"]:
        bad.append(("rest",))
    at += len(exp["rest"])
    if to_bytes(mem[at:at + len(exp["tail"])]) != exp["tail"]:
        bad.append(("tail", to_bytes(mem[at:at + len(exp["tail"])]).hex(), exp["tail"].hex()))
    return bad


def gzip_isize(stream_tail):
    """the ISIZE field of the last four bytes of a gzip stream"""
    return int.from_bytes(bytes(stream_tail)[-4:], "little")


# ---- long streams: one inflate at the ends of its own 32-bit counters (families G and G2) ------------------------------

def static_code(w, sym):
    """one litlen symbol in the static code (RFC 1951 3.2.6)"""
    if sym < 144:
        w.huff(0x30 + sym, 8)
    elif sym < 256:
        w.huff(0x190 + sym - 144, 9)
    elif sym < 280:
        w.huff(sym - 256, 7)
    else:
        w.huff(0xc0 + sym - 280, 8)


def static_match(w, length, dist):
    import deflate_gen as dg
    ls, ds = dg.len_sym(length), dg.dist_sym(dist)
    static_code(w, ls)
    w.bits(length - dg.LEN_BASE[ls - 257], dg.LEN_EXTRA[ls - 257])
    w.huff(ds, 5)
    w.bits(dist - dg.DIST_BASE[ds], dg.DIST_EXTRA[ds])


def long_input_stream(nbytes, rng):
    """a stream of exactly nbytes bytes: stored blocks of 65535 noise bytes (one block, tiled), a shorter one, and a final
    static block of three literals -> (stream as numpy, the 65535-byte pattern, how often it repeats, the rest of the output)"""
    import deflate_gen as dg
    w = dg.BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for ch in b"end":
        static_code(w, ch)
    static_code(w, 256)
    last = w.value()
    pattern = rng.integers(0, 256, 65535, dtype=np.uint8)
    block = np.concatenate([np.frombuffer(b"\x00\xff\xff\x00\x00", dtype=np.uint8), pattern])
    reps, left = divmod(nbytes - len(last), len(block))
    assert 5 <= left
    part = rng.integers(0, 256, left - 5, dtype=np.uint8)
    head = np.frombuffer(b"\x00" + int(left - 5).to_bytes(2, "little") + int((left - 5) ^ 0xffff).to_bytes(2, "little"), dtype=np.uint8)
    stream = np.concatenate([np.tile(block, reps), head, part, np.frombuffer(last, dtype=np.uint8)])
    assert len(stream) == nbytes
    return stream, pattern, reps, part.tobytes() + b"end"


def long_output_stream(total):
    """a small stream of `total` bytes of output: one stored block of 32 KiB of noise, then static-Huffman matches of length
    258 at distance 32768 -- 26 bits each, so four of them are a 13-byte period of the stream, tiled -- a last match or two
    for the remainder and the end of block -> (stream as numpy, the 32 KiB pattern)"""
    import deflate_gen as dg
    pattern = np.random.default_rng(31).integers(0, 256, 32768, dtype=np.uint8)
    assert total % 32768 == 0 and total >= 32768 + 258 * 12
    n258, rem = divmod(total - 32768, 258)
    tail = []
    if 0 < rem < 3:
        n258, rem = n258 - 1, rem + 258
        tail = [rem // 2, rem - rem // 2]
    elif rem:
        tail = [rem]
    periods, extra = divmod(n258, 4)
    w = dg.BitWriter()                                   # the final block with TWO periods: head byte | period | the rest
    w.bits(1, 1)
    w.bits(1, 2)
    for length in [258] * (8 + extra) + tail:
        static_match(w, length, 32768)
    static_code(w, 256)
    sample = w.value()
    assert sample[1:14] == sample[14:27] or extra + len(tail) == 0
    head = b"\x00\x00\x80\xff\x7f" + pattern.tobytes() + sample[:1]
    stream = np.concatenate([np.frombuffer(head, dtype=np.uint8), np.tile(np.frombuffer(sample[1:14], dtype=np.uint8), periods - 1),
                             np.frombuffer(sample[14:], dtype=np.uint8)])
    return stream, pattern


def framed_long_member(frame, stream, pattern, reps, rest=b""):
    """a long stream of this file in a frame (0 raw, 4 zlib, 5 gzip: framed_gen's plain headers), its check value and ISIZE
    by construction -- the output is `pattern` reps times and `rest`, so the CRC-32 / Adler-32 is stream_model.fold of the
    parts' -> (member as numpy, check, bytes of output)"""
    import framed_gen
    kind, pat = sm.KIND[frame], pattern.tobytes()
    lens = [len(pat)] * reps + ([len(rest)] if rest else [])
    checks = [sm.part_check(pat, kind)] * reps + ([sm.part_check(rest, kind)] if rest else [])
    check, total = sm.fold(checks, lens, kind), sum(lens)
    head = {sm.FRAME_RAW: b"", sm.FRAME_ZLIB: framed_gen.zlib_header(), sm.FRAME_GZIP: framed_gen.gzip_header()}[frame]
    member = np.concatenate([np.frombuffer(head, dtype=np.uint8), stream,
                             np.frombuffer(sm.trailer(frame, check, total), dtype=np.uint8)])
    return member, check, total


LONG_OVERHEAD = {sm.FRAME_RAW: 0, sm.FRAME_ZLIB: 2 + 4, sm.FRAME_GZIP: 10 + 8}     # header + trailer of framed_long_member
