"""Plain-Python model of the stream index and the decode on its table (include/hipdeflate.h, "the same decode for a stream
whose table nobody kept"):
  * the candidates: the first payload byte, and every position of the payload region with 00 00 ff ff in front of it
    (bytes.find);
  * a piece: deflate_tokens' block reader (its tables, its dynamic header, Block.sync_flush / final / end_bit) run from a
    candidate over a bounded input whose missing bits read as 0, stopped at the first flush point or final block;
  * the chain from candidate 0, the tables, the summary;
  * the verdicts of the decode on a table, in the order the header gives them, the rows through zlib.
No GPU, no product code.  tests/test_stream_index_model.py holds it to zlib."""
import zlib

from deflate_gen import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA
from deflate_tokens import Block, DeflateError, _dynamic_header, _static_tables
from framed_model import open_member

FRAME_RAW, FRAME_ZLIB, FRAME_GZIP = 0, 4, 5
TRAILER = {FRAME_RAW: 0, FRAME_ZLIB: 4, FRAME_GZIP: 8}
MIN_BYTES = {FRAME_RAW: 0, FRAME_ZLIB: 6, FRAME_GZIP: 18}
WBITS = {FRAME_RAW: -15, FRAME_ZLIB: 15, FRAME_GZIP: 31}
INFLATE_MAX_IN = 1 << 28             # include/hipdeflate_params.h HD_INFLATE_MAX_IN
MARKER = b"\x00\x00\xff\xff"
FLUSH, FINAL = 1, 2                  # the stop a piece hit
OK, BAD, CUT = 0, 1, 4               # a piece's verdict (CUT: it needed a bit at or behind the end of its input)


class _Bits:
    """deflate_tokens' reader over n bytes whose bits behind the end read as 0: nothing raises for running out; `over`
    says whether the position has passed the end"""

    def __init__(self, data):
        self.nbits = 8 * len(data)
        self.data = bytes(data) + bytes(16)
        self.pos = 0

    def get(self, n):
        p = self.pos
        v = int.from_bytes(self.data[p >> 3:(p >> 3) + 8], "little") >> (p & 7) if p < self.nbits else 0
        self.pos = p + n
        return v & ((1 << n) - 1)

    def sym(self, table, maxl):
        p = self.pos
        v = int.from_bytes(self.data[p >> 3:(p >> 3) + 8], "little") >> (p & 7) if p < self.nbits else 0
        e = table[v & ((1 << maxl) - 1)]
        if e < 0:
            raise DeflateError("bits %d: no codeword" % p)
        self.pos = p + (e & 15)
        return e >> 4

    @property
    def over(self):
        return self.pos > self.nbits


def piece(stream, p, n):
    """the piece that starts at stream[p], over n bytes of input -> (verdict, stop, in_used, out_size, blocks).  The
    verdict is CUT as soon as the position behind an element that was read lies past the input; what the rules say of
    that element no longer counts."""
    bits = _Bits(stream[p:p + n])
    nout, blocks = 0, []

    def fail(v):
        return v, 0, 0, 0, blocks

    try:
        while True:
            start = bits.pos
            final, btype = bits.get(1), bits.get(2)
            if bits.over:
                return fail(CUT)
            if btype == 3:
                return fail(BAD)
            blk = Block(("stored", "static", "dynamic")[btype], bool(final), start, nout)
            blocks.append(blk)
            if btype == 0:
                bits.pos = (bits.pos + 7) & ~7
                if bits.pos + 32 > bits.nbits:
                    return fail(CUT)
                ln, nl = bits.get(16), bits.get(16)
                if ln != (~nl & 0xffff):
                    return fail(BAD)
                if (bits.pos >> 3) + ln > n:
                    return fail(CUT)
                bits.pos += 8 * ln
                nout += ln
                blk.stored_len = ln
            else:
                if btype == 1:
                    (lt, lm), (dt, dm) = _static_tables()
                else:
                    try:
                        (lt, lm), (dt, dm) = _dynamic_header(bits, blk, oracle=True)
                    except DeflateError:
                        return fail(CUT if bits.over else BAD)
                    if bits.over:
                        return fail(CUT)
                while True:
                    s = bits.sym(lt, lm)
                    if bits.over:
                        return fail(CUT)
                    if s < 256:
                        nout += 1
                        continue
                    if s == 256:
                        break
                    k = s - 257                              # (286, 287: length 258, as the oracle has them)
                    length = LEN_BASE[k] + bits.get(LEN_EXTRA[k])
                    ds = bits.sym(dt, dm)                    # (the empty code: symbol 0; 30, 31: 24577 + 13 bits)
                    d = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                    if bits.over:
                        return fail(CUT)
                    if d > nout:
                        return fail(BAD)
                    nout += length
            blk.end_bit, blk.out_end = bits.pos, nout
            if blk.final or blk.sync_flush:
                return OK, FINAL if blk.final else FLUSH, (blk.end_bit + 7) >> 3, nout, blocks
    except DeflateError:
        return fail(CUT if bits.over else BAD)


def header(stream, frame):
    """-> (hdr_bytes, verdict): 0, 1 the header is refused, 2 the stream is below the frame's header and trailer"""
    if len(stream) < MIN_BYTES[frame]:
        return 0, 2
    h = open_member(bytes(stream[:INFLATE_MAX_IN - 1]), frame)
    return (0, 1) if h is None else (h, 0)


def candidates(stream, frame, hdr):
    """the first payload byte, then every position in front of nbytes - trailer with the marker, inside the payload
    region, in front of it"""
    end = len(stream) - TRAILER[frame]
    out, q = [hdr], stream.find(MARKER, hdr, end - 1)
    while q >= 0:
        out.append(q + 4)
        q = stream.find(MARKER, q + 1, end - 1)
    return out


def index(stream, frame, max_chunks=None, max_chunk_in=0):
    """what hipdeflate_stream_index_dev answers -> (summary as a dict, in_off, in_len, out_size, out_off): the tables
    hold min(nchunks, max_chunks) rows (max_chunks None: as many as the stream has)"""
    stream = bytes(stream)
    max_in = max_chunk_in or INFLATE_MAX_IN - 1
    s = {"nchunks": 0, "out_bytes": 0, "end_offset": 0, "ncandidates": 0, "hdr_bytes": 0, "status": 0}
    hdr, refused = header(stream, frame)
    if refused:
        s["status"] = refused
        return s, [], [], [], []
    end = len(stream) - TRAILER[frame]
    s["hdr_bytes"] = s["end_offset"] = hdr
    s["ncandidates"] = 1
    if end == hdr:
        s["status"] = 2
        return s, [], [], [], []
    cand = candidates(stream, frame, hdr)
    s["ncandidates"] = len(cand)
    on_list = set(cand)
    rows, c = [], hdr
    while True:
        v, stop, used, size, _ = piece(stream, c, min(max_in, end - c))
        if v != OK:
            s["end_offset"] = c
            s["status"] = 2 if v == CUT and end - c <= max_in else 1
            break
        rows.append((c, used, size))
        if stop == FINAL:
            s["end_offset"] = c + used + TRAILER[frame]
            break
        c += used
        if c == end:                                   # a flush point is the last payload byte
            s["end_offset"], s["status"] = c, 2
            break
        assert c in on_list, c                         # the byte behind a flush point is a candidate by construction
    s["nchunks"] = len(rows)
    if max_chunks is not None and len(rows) > max_chunks:
        s["status"] = 3
        rows = rows[:max_chunks]
    out_off, t = [], 0
    for _, _, size in rows:
        out_off.append(t)
        t += size
    s["out_bytes"] = t
    return s, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], out_off


def inflate_row(data):
    """one row by the flush rule: a raw stream that may end on a byte boundary behind a non-final block -> bytes or None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(data)
    except zlib.error:
        return None
    if d.unused_data or d.unconsumed_tail:
        return None
    return out


def decode(stream, frame, in_off, in_len, out_size, out_off, out_cap=None):
    """what hipdeflate_stream_inflate_table_dev answers -> (summary as a dict, output or None).  summary["check"] is None
    where the header leaves it unspecified (a bad row) or nothing was inflated."""
    stream, n = bytes(stream), len(in_off)
    trl = TRAILER[frame]

    def verdict(status, bad, out_bytes=0, in_bytes=0, check=None):
        return {"out_bytes": out_bytes, "in_bytes": in_bytes, "bad_chunk": bad, "nchunks": n, "check": check, "status": status}

    if n == 0:
        return verdict(1, n), None
    hdr, refused = header(stream, frame)
    if refused:
        return verdict(1, n), None
    end = len(stream) - trl
    for i in range(n):
        o, ln = in_off[i], in_len[i]
        fault = ln >= INFLATE_MAX_IN or o < hdr or o > end or ln > end - o or (i == 0 and out_off[0] != 0)
        if i + 1 < n:
            fault = fault or in_off[i + 1] < o + ln or out_off[i + 1] != out_off[i] + out_size[i]
        if fault:
            return verdict(1, i), None
    total = out_off[-1] + out_size[-1]
    if out_cap is not None and out_cap < total:
        return verdict(3, n, total), None
    used = in_off[-1] + in_len[-1] + trl
    outs = []
    for i in range(n):
        b = inflate_row(stream[in_off[i]:in_off[i] + in_len[i]])
        if b is None or len(b) != out_size[i]:
            return verdict(2, i, total, used), None
        outs.append(b)
    out = b"".join(outs)
    t = stream[used - trl:used]
    ok = True
    if frame == FRAME_ZLIB:
        check = zlib.adler32(out)
        ok = t == check.to_bytes(4, "big")
    else:
        check = zlib.crc32(out)
        if frame == FRAME_GZIP:
            ok = t == check.to_bytes(4, "little") + (total & 0xffffffff).to_bytes(4, "little")
    return verdict(0 if ok else 2, n, total, used, check), out


HEADER = {FRAME_RAW: b"", FRAME_ZLIB: bytes.fromhex("789c"), FRAME_GZIP: bytes.fromhex("1f8b08000000000000ff")}


def trailer(frame, plain):
    if frame == FRAME_ZLIB:
        return zlib.adler32(plain).to_bytes(4, "big")
    if frame == FRAME_GZIP:
        return zlib.crc32(plain).to_bytes(4, "little") + (len(plain) & 0xffffffff).to_bytes(4, "little")
    return b""


def writer(pieces, frame, level=6):
    """a stream of another writer: ONE zlib object, Z_FULL_FLUSH behind every piece but the last, Z_FINISH with the last
    piece still to code -> (stream, the offsets the writer recorded: where every piece starts)"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[frame])
    stream, off = b"", []
    for i, p in enumerate(pieces):
        off.append(max(len(stream), len(HEADER[frame])))          # (the header comes out with the first bytes)
        stream += c.compress(p)
        if i + 1 < len(pieces):
            stream += c.flush(zlib.Z_FULL_FLUSH)
    return stream + c.flush(), off


def compose(pieces, frame, header=None, raw_pieces=False):
    """the same from pieces coded one by one -- pieces behind a full flush share nothing, so they concatenate: (bytes, level)
    in the place of bytes codes that piece at its own level, and with raw_pieces the pieces are raw DEFLATE already (every
    one but the last in flush form) given as (coded, plain) -> (stream, the offsets where the pieces start, the plain bytes)"""
    hdr = HEADER[frame] if header is None else header
    body, off, plain = b"", [], b""
    for i, p in enumerate(pieces):
        off.append(len(hdr) + len(body))
        if raw_pieces:
            body += p[0]
            plain += p[1]
            continue
        data, level = p if isinstance(p, tuple) else (p, 6)
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body += c.compress(data) + (c.flush(zlib.Z_FULL_FLUSH) if i + 1 < len(pieces) else c.flush())
        plain += data
    return hdr + body + trailer(frame, plain), off, plain
