"""Carry streams from the hand-built corpus (tests/deflate_gen.py): streams of rows cut by flush points that keep the window,
each with the table the token lists give -- so the carry index and the carry decode (hd_carry.hpp: k_carry_piece,
k_carry_decode, k_carry_tails, k_carry_resolve) meet every header and token edge of DEFLATE, and the edges of their own
rings, as ROWS.  Plain Python; no product code.  tests/test_carry_rows.py pins it on the CPU, tests/test_gpu_carry_rows.py
puts it through the kernels.

  cut_every(blocks)   a new row in front of every Huffman block but the stream's first block
  cut_mid(blocks)     one cut, in front of the Huffman block whose output offset is nearest half the total
  fault_row(case)     a row of `lead` literals, then a fault stream of the corpus as row 1, with the table a caller would claim
  carry_ring(rng)     a family of its own: the 32768-symbol ring of k_carry_decode, the window and the thread layout of
                      k_carry_tails, the body of k_carry_resolve -- everything by position in the ROW
A composed stream is a `Rows`: .rows (lists of deflate_gen.Block), .stream / .plain per frame by compose(), and .table(): the
rows' (out_size, reach) counted from the token lists."""
import collections

import numpy as np

import deflate_gen as dg
from deflate_gen import Block
from stream_index_model import HEADER, trailer

W = 32768                   # DEFLATE's window = CARRY_WINDOW, the ring of k_carry_decode and of k_carry_tails


class Rows:
    __slots__ = ("name", "family", "rows", "zlib", "stats", "_body", "plain")

    def __init__(self, name, family, rows, plain=None, zlib_ok=True, stats=None):
        self.name, self.family, self.rows, self.zlib = name, family, rows, zlib_ok
        self.stats = stats or collections.Counter()
        assert rows[-1] and rows[-1][-1].final and not any(b.final for b in rows[-1][:-1]), name
        self._body = b"".join(dg.encode(r, chunk=True) for r in rows[:-1]) + dg.encode(rows[-1])
        self.plain = dg.expand([b for r in rows for b in r]) if plain is None else plain

    def compose(self, frame):
        """-> the stream in that frame"""
        return HEADER[frame] + self._body + trailer(frame, self.plain)

    def table(self):
        """(out_size, reach) by row, from the token lists: a row ends where its list ends and at every empty stored block
        inside it (the chunk form writes every block of a row but the last row's as non-final); reach = the furthest a
        match goes back over the row's first byte"""
        sizes, reach, n, r = [], [], 0, 0
        for i, row in enumerate(self.rows):
            last = i + 1 == len(self.rows)
            for b in row:
                if b.kind == "stored":
                    if not b.data and not (last and b.final):
                        sizes.append(n)
                        reach.append(r)
                        n = r = 0
                    n += len(b.data)
                    continue
                for t in b.tokens:
                    if isinstance(t, int):
                        n += 1
                    else:
                        r = max(r, t[1] - n)
                        n += t[0]
            if not last:                                     # the marker encode() puts behind the row
                sizes.append(n)
                reach.append(r)
                n = r = 0
        return sizes + [n], reach + [r]


def huffman_starts(blocks):
    """(index, output offset) of every Huffman block that is not the stream's first block"""
    out, at = 0, []
    for i, b in enumerate(blocks):
        if b.kind != "stored" and i:
            at.append((i, out))
        out += len(b.data) if b.kind == "stored" else sum(1 if isinstance(t, int) else t[0] for t in b.tokens)
    return at, out


def _split(blocks, cuts):
    rows, lo = [], 0
    for i in cuts:
        rows.append(list(blocks[lo:i]))
        lo = i
    return rows + [list(blocks[lo:])]


def cut_every(blocks):
    """-> rows, or None where there is nowhere to cut: one Huffman block in front of whatever else, or none"""
    at, _ = huffman_starts(blocks)
    return _split(blocks, [i for i, _ in at]) if at else None


def cut_mid(blocks):
    at, total = huffman_starts(blocks)
    if not at:
        return None
    i, _ = min(at, key=lambda e: (abs(2 * e[1] - total), e[0]))
    return _split(blocks, [i])


def corpus_rows(cut, family):
    """(the Rows of every valid, non-chunk corpus case that `cut` gives more than one row, the names of the cases left out)"""
    out, single = [], []
    for c in dg.cached_corpus():
        if c.chunk or c.code != dg.OK or c.blocks is None:
            continue
        rows = cut(c.blocks)
        if rows is None:
            single.append(c.name)
            continue
        out.append(Rows(c.name, family, rows, plain=c.expected, zlib_ok=c.zlib))
    return out, single


_cache = {}


def cached(key):
    """'every' | 'mid' -> corpus_rows(...) once per process; 'ring' -> carry_ring() once per process"""
    if key not in _cache:
        _cache[key] = (corpus_rows(cut_every, "cut_every") if key == "every" else corpus_rows(cut_mid, "cut_mid") if key == "mid"
                       else carry_ring(np.random.default_rng(2028)))
    return _cache[key]


# ---- a fault stream as row 1 ---------------------------------------------------------------------------------------------------

class FaultRow:
    """stream: RAW; table: the five columns a caller would claim; plain: lead + row where the row is valid there, else None"""
    __slots__ = ("name", "stream", "table", "plain")


def fault_row(case, oracle_size, lead=100):
    """oracle_size: what the oracle decodes the fault stream to in a large room, None where it refuses it.  out_size of row 1
    is the room the case states where its fault is that room (cap_over_on_*), the token lists' size where the row is valid
    behind a lead (dist_past_out_*: its one match reaches into the lead), else the oracle's size, else 1000.  reach = lead: the
    group takes the marker path, not the batch inflate."""
    f = FaultRow()
    f.name = case.name
    lits = [(7 * k + 33) & 255 for k in range(lead)]
    row0 = dg.encode([Block("static", tokens=lits)], chunk=True)
    f.stream = row0 + case.stream
    f.plain = None
    if case.name.startswith("dist_past_out_"):
        # the family builder's blocks, read back from the stream: d - 1 stored bytes, then a static block of (3, d) and 7
        d = int(case.name.rsplit("_d", 1)[1])
        blocks = [Block("stored", data=case.stream[5:4 + d]), Block("static", tokens=[(3, d), 7], final=True)]
        assert dg.encode(blocks) == case.stream
        f.plain = dg.expand([Block("static", tokens=lits)] + blocks)
        size = len(f.plain) - lead
    elif case.code == dg.INSUFFICIENT_SPACE:
        size = case.cap
    else:
        size = 1000 if oracle_size is None else oracle_size
    f.table = ([0, len(row0)], [len(row0), len(case.stream)], [lead, size], [0, lead], [0, lead])
    return f


def literal_tails():
    """a stream whose rows end in 300 literals and more behind a match that reaches back (no cut of the corpus gives such a
    row): what a table whose out_size is 100 short needs to stop the decoder in a window of literals, not at a match"""
    rng = np.random.default_rng(2029)
    rows = [[Block("stored", data=dg.rand_bytes(rng, 1000))],
            [Block("static", tokens=[(50, 900)] + dg.lits(dg.rand_bytes(rng, 400)))],
            [Block("dynamic", tokens=dg.lits(dg.rand_bytes(rng, 10)) + [(20, 500)] + dg.lits(dg.rand_bytes(rng, 350)))],
            [Block("static", tokens=[(3, 1)], final=True)]]
    return Rows("rows_end_in_300_literals", "literal_tails", rows)


# ---- carry_ring: the rings, by position in the row --------------------------------------------------------------------------------

RING_DISTS = [1, 2, 7, 8, 9, 16, 17, 64, 65, 258, 1024, 16384, 32510, 32767, 32768]
ROW_BYTES = 70001
LEAD_BYTES = 40000
ALL_MARKER_SIZES = [3, 1023, 1024, 1025, 2047, 2048, 32767, 32768, 32769, 65536, 70001]
FAR_K = [0, 1, 2, 63, 64, 65, 257]


def _phases(ln):
    return (("A", -(ln // 2)), ("B", -1), ("0", 0), ("1", 1))


def ring_items():
    """(span, other): matches as (length, distance, kind, wrap, row position of the destination).  kind d<phase>: the
    destination starts at wrap + phase, s<phase>: the source does; phase A = -length // 2, B = -1, 0, 1.  span: every
    (length, distance) with its destination across row position 32768 at both phases that span it; other: the other kinds
    at 32768 and every kind at 65536, a stride (the full matrix is 14 x 15 x 8 x 2)."""
    span = [(ln, d, "d" + p, W, W + o) for p in "AB" for d in RING_DISTS for ln in dg.MATCH_LENGTHS for q, o in _phases(ln) if q == p]
    other = [(ln, d, "d" + p, wrap, wrap + o) for wrap in (W, 2 * W) for p in ("01" if wrap == W else "AB01") for d in RING_DISTS
             for ln in dg.MATCH_LENGTHS for q, o in _phases(ln) if q == p]
    other += [(ln, d, "s" + p, wrap, wrap + o + d) for wrap in (W, 2 * W) for p in "AB01" for d in RING_DISTS if d <= 1024
              for ln in dg.MATCH_LENGTHS for q, o in _phases(ln) if q == p]
    other = [other[(i * 13) % len(other)] for i in range(260)]
    return span, other


def _item_block(rng, k, ln, d):
    """0 / 2 / 37 / 300 literals in front of the match in its own block, static or derived dynamic, three literals behind"""
    nl = (0, 2, 37, 300)[k % 4]
    return nl, Block(("static", "dynamic")[(k + k // 4) % 2], tokens=dg.lits(dg.rand_bytes(rng, nl)) + [(ln, d)] + dg.lits(dg.rand_bytes(rng, 3)))


def _count_match(st, p, ln, d):
    """what a match at row position p reaches, counted as it is written"""
    if p < W < p + ln:
        st["ring_dst_across_32768"] += 1
    if p < 2 * W < p + ln:
        st["ring_dst_across_65536"] += 1
    s = p - d
    for wrap in (W, 2 * W):
        if s < wrap < s + min(ln, d):
            st["ring_src_across_%d" % wrap] += 1
    if s < 0 < s + ln:
        st["straddle_row_start"] += 1
        st["straddle_row_start_overlap" if ln > d else "straddle_row_start_plain"] += 1
        if p <= 257:
            st["straddle_p_1_257"] += 1
        if 32511 <= p <= 32767 and d == W:
            st["straddle_p_32511_32767"] += 1
    if s + ln <= 0:
        st["all_markers_match"] += 1


def _row_stats(st, row):
    p = 0
    for b in row:
        if b.kind == "stored":
            p += len(b.data)
            continue
        for i, t in enumerate(b.tokens):
            if isinstance(t, int):
                p += 1
                continue
            _count_match(st, p, t[0], t[1])
            nxt = b.tokens[i + 1] if i + 1 < len(b.tokens) else None
            if isinstance(nxt, int) and W - t[1] in FAR_K:
                st["literal_behind_far_%d%s" % (W - t[1], "_in_ring" if p >= t[1] else "")] += 1
            p += t[0]


def _ring(name, rows, st=None):
    st = st or collections.Counter()
    rows[-1][-1].final = True
    for r in rows[1:]:
        _row_stats(st, r)
    return Rows(name, "carry_ring", rows, stats=st)


def _lead(rng, n=LEAD_BYTES):
    data = dg.rand_bytes(rng, n)
    return [Block("stored", data=data[i:i + 65535]) for i in range(0, n, 65535)]


def _size(row):
    return sum(len(b.data) if b.kind == "stored" else sum(1 if isinstance(t, int) else t[0] for t in b.tokens) for b in row)


def row_fill(rng, out, target):
    """deflate_gen.match_fill without its stored seed: one static block of (258, 300) matches and fewer than 258 random
    literals.  At a row's start the first match names 300 bytes in front of the row, so the row reaches back -- a group
    whose rows all stand alone goes through the batch inflate, not through k_carry_decode -- and what the filler copies on
    from there are markers and copies of markers."""
    gap = target - out
    assert gap >= 0
    return [Block("static", tokens=[(258, 300)] * (gap // 258) + dg.lits(dg.rand_bytes(rng, gap % 258)))] if gap else []


GROUP_BYTES = 256 << 20     # HD_CARRY_GROUP_BYTES: the default group of hipdeflate_stream_inflate_carry_dev


def marker_path_rows(sizes, reach, group_bytes=0):
    """by row: whether its group takes the marker path (k_carry_decode, k_carry_tails, k_carry_resolve).  A group is the run
    of rows whose out_off lies in one multiple of the group size (k_carry_group); it takes the marker path where its largest
    reach is > 0, else the batch inflate."""
    g = group_bytes or GROUP_BYTES
    off, t = [], 0
    for n in sizes:
        off.append(t)
        t += n
    out, r0 = [], 0
    while r0 < len(sizes):
        r1 = r0 + 1
        while r1 < len(sizes) and off[r1] // g == off[r0] // g:
            r1 += 1
        out += [max(reach[r0:r1]) > 0] * (r1 - r0)
        r0 = r1
    return out


def all_markers(size):
    """a row of `size` bytes that is nothing but markers: (258, 32768) over and over and a remainder (a match is 3 bytes
    at the least: a remainder of 1 or 2 is taken off the match in front of it).  Behind row position 32768 every symbol is
    a copy of a marker."""
    assert size >= 3
    n, r = divmod(size, 258)
    if 0 < r < 3:
        toks = [(258, W)] * (n - 1) + [(255 + r, W), (3, W)]
    else:
        toks = [(258, W)] * n + ([(r, W)] if r else [])
    assert sum(t[0] for t in toks) == size
    return toks


def carry_ring(rng):
    """-> [Rows].  Every stream starts with a row of 40,000 stored random bytes (the marker-source streams: of the length
    that puts the next row's first byte where it is wanted)."""
    out = []
    span, other = ring_items()
    at_w, at_2w = [e for e in other if e[3] == W], [e for e in other if e[3] == 2 * W]
    # ---- ring wraps: rows of about 70,000 bytes, one match at row position 32768 and one at 65536, between them a filler
    # that reaches over the row's start (row_fill): every row goes through k_carry_decode, in a group of its own too
    k, s = 0, 0
    while span or at_w or at_2w:
        rows, st = [_lead(rng)], collections.Counter()
        for _ in range(20):
            picks = [q.pop(0) for q in (span or at_w, at_2w) if q]
            if not picks:
                break
            row, p = [], 0
            for ln, d, kind, wrap, dest in picks:
                nl, blk = _item_block(rng, k, ln, d)
                row += row_fill(rng, p, dest - nl) + [blk]
                p = dest + ln + 3
                st["ring_%s_%d" % (kind, wrap)] += 1
                if kind in ("dA", "dB") and wrap == W:
                    st["ring_pair_%d_%d" % (ln, d)] += 1
                k += 1
            rows.append(row + row_fill(rng, p, max(p, ROW_BYTES)))
        out.append(_ring("ring_wrap_%d" % s, rows, st))
        s += 1
    # ---- row-start straddles: the first symbols of the match are markers, the rest the row's own bytes
    rows = [_lead(rng)]
    for p in (1, 2, 3, 37, 63, 64, 65, 255, 256, 257):
        for ln, d in ((258, p + 1), (17, p + 3), (min(258, p + 5), p + 5), (258, W)):        # overlap, overlap, none, far
            for kind in ("static", "dynamic"):
                rows.append([Block(kind, tokens=dg.lits(dg.rand_bytes(rng, p)) + [(ln, d)] + dg.lits(dg.rand_bytes(rng, 5)))])
    for p in (32511, 32512, 32600, 32766, 32767):
        rows.append(dg.match_fill(rng, 0, p) + [Block("static" if p & 1 else "dynamic", tokens=[(258, W), 1, 2, 3])])
    out.append(_ring("ring_straddle", rows))
    # ---- literals directly behind matches of distance 32768 - k: in front of row position 32768 (markers), and behind it,
    # where the slot of a literal placed ahead of its turn is one the match still has to read
    for kind in ("static", "dynamic"):
        row = []
        for base in (0, 33000):
            row += dg.match_fill(rng, _size(row), base) if base else []
            toks = []
            for kk in FAR_K:
                toks += [(258, W - kk)] + dg.lits(dg.rand_bytes(rng, 80)) + [(3, W - kk), 200 + kk % 50, (64, W - kk)] + \
                        dg.lits(dg.rand_bytes(rng, 3))
            row.append(Block(kind, tokens=toks))
        out.append(_ring("ring_far_then_literals_" + kind, [_lead(rng), row]))
    # ---- rows that are nothing but markers: behind a long row, and behind three short rows of 5, 0 and 300 bytes
    for size in ALL_MARKER_SIZES:
        short = [[Block("static", tokens=dg.lits(dg.rand_bytes(rng, 5)))], [Block("static", tokens=[])],
                 [Block("dynamic", tokens=dg.lits(dg.rand_bytes(rng, 300)))]]
        rows = [_lead(rng), [Block("dynamic" if size & 1 else "static", tokens=all_markers(size))]] + short + \
               [[Block("static" if size & 1 else "dynamic", tokens=all_markers(size))], [Block("static", tokens=[(3, 1)])]]
        out.append(_ring("ring_all_markers_%d" % size, rows, collections.Counter({"all_markers_row_%d" % size: 2})))
    # (a row of one byte cannot be a marker: it is a literal.  Behind it, a marker row that names it)
    out.append(_ring("ring_row_of_1", [_lead(rng), [Block("static", tokens=[9])], [Block("static", tokens=all_markers(1025))]],
                     collections.Counter({"row_of_1_byte": 1})))
    # ---- marker sources at the wrap of k_carry_tails' window: (row start - backdist) mod 32768 = 0, 1, 32767
    for backdist in (1, W):
        for slot in (0, 1, W - 1):
            start = 2 * W + (slot + backdist) % W
            rows = [_lead(rng, start), [Block("static", tokens=[(258, backdist), 5, 6])]]
            out.append(_ring("ring_source_slot_%d_back_%d" % (slot, backdist), rows,
                             collections.Counter({"source_slot_%d_back_%d" % (slot, backdist): 1})))
    # ... and the row's own first tail slot: with backdist 32768 that is every row shorter than the window; with backdist 1 a
    # row of 65535 bytes, whose tail starts 32767 bytes in -- the markers at its start, and copies of them in the tail
    row = [Block("static", tokens=[(258, 1)])] + dg.match_fill(rng, 258, W) + [Block("dynamic", tokens=[(258, W), 8, 9])]
    row += dg.match_fill(rng, _size(row), 65535)
    assert _size(row) == 65535
    out.append(_ring("ring_source_first_tail_slot_back_1", [_lead(rng), row], collections.Counter({"source_first_tail_slot_back_1": 1})))
    # ---- rows of 13..15-bit codewords (the shape of lat_wrap_%dbit_run): one token each through the scalar path, the matches
    # reach over the row's start -- its marker branch; a stored block of 65,535 bytes behind them, and behind that a second run
    # that reads the stored bytes from the ring.  The next row's marker matches follow: the stored block lies between two.
    pool = [int(x) for x in rng.permutation(256)[:40]]
    rows = [_lead(rng)]
    for L in (13, 14, 15):
        fixed = {256: L, 285: L, pool[0]: L, pool[1]: L}
        lit = dg.fill_lengths(fixed, pool[2:] + [257, 264, 265, 272, 280, 284], 286)
        dist = dg.auto_lengths({0: 3, 3: 2, 4: 1, 10: 1, 16: 1, 22: 1}, 30)
        dsyms = [x for x in range(30) if dist[x]]
        # four matches of the run's own codewords that name bytes in front of the row, whatever the draw below gives
        head = [pool[0], (258, 3072, 285, 22), pool[1], (258, 3000, 285, 22), (258, 2900, 285, 22), pool[0], (258, 2600, 285, 22)]
        run = head + dg.sym_tokens(rng, [285, pool[0], pool[1]], 60, LEAD_BYTES, dsyms)
        other = dg.sym_tokens(rng, [x for x in range(286) if lit[x] and x != 256], 100, LEAD_BYTES, dsyms)
        run2 = dg.sym_tokens(rng, [285, pool[0], pool[1]], 60, LEAD_BYTES, dsyms)
        row = [Block("dynamic", tokens=run + other, lit_lens=lit, dist_lens=dist), Block("stored", data=dg.rand_bytes(rng, 65535)),
               Block("dynamic", tokens=run2, lit_lens=lit, dist_lens=dist)]
        rows.append(row)
    st = collections.Counter({"long_code_row_%dbit" % L: 1 for L in (13, 14, 15)})
    c = _ring("ring_long_codes", rows, st)
    for r, L in zip(rows[1:], (13, 14, 15)):                  # the matches of the run that name bytes in front of the row
        p = 0
        for t in r[0].tokens[:67]:
            c.stats["long_code_marker_matches_%dbit" % L] += (not isinstance(t, int)) and t[1] > p
            p += 1 if isinstance(t, int) else t[0]
    out.append(c)
    return out
