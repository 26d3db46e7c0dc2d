"""Plain-Python model of the carry index and the carry decode (include/hipdeflate.h, "a stream whose flushes CARRY the
window"): stream_index_model with the window carried across the flush points.
  * piece(): stream_index_model.piece without its `d > nout` refusal, and with the furthest distance over the piece's first
    byte kept as its reach;
  * index_carry(): the chain, the five tables, the reach rule and its clause for a table that is too small;
  * decode_carry(): the verdicts in the header's order; the bytes through ONE zlib.decompressobj over the stream (the
    caller's own where zlib refuses the form);
  * two writers of such streams, and a composer for hand-built rows with chosen (length, distance) tokens.
No GPU, no product code.  tests/test_stream_carry_model.py holds it to zlib."""
import zlib

import deflate_gen as dg
from deflate_gen import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA
from deflate_tokens import Block, DeflateError, _dynamic_header, _static_tables
from stream_index_model import (BAD, CUT, FINAL, FLUSH, FRAME_GZIP, FRAME_RAW, FRAME_ZLIB, HEADER, INFLATE_MAX_IN, OK, TRAILER, WBITS,
                                _Bits, candidates, header, trailer)

WINDOW = 32768


def piece(stream, p, n):
    """the piece that starts at stream[p], over n bytes of input -> (verdict, stop, in_used, out_size, reach).  A distance
    past the bytes the piece has put out is no fault: reach is the furthest one, counted from the piece's first byte."""
    bits = _Bits(stream[p:p + n])
    nout, reach = 0, 0

    def fail(v):
        return v, 0, 0, 0, 0

    try:
        while True:
            start = bits.pos
            final, btype = bits.get(1), bits.get(2)
            if bits.over:
                return fail(CUT)
            if btype == 3:
                return fail(BAD)
            blk = Block(("stored", "static", "dynamic")[btype], bool(final), start, nout)
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
                        reach = max(reach, d - nout)
                    nout += length
            blk.end_bit, blk.out_end = bits.pos, nout
            if blk.final or blk.sync_flush:
                return OK, FINAL if blk.final else FLUSH, (blk.end_bit + 7) >> 3, nout, reach
    except DeflateError:
        return fail(CUT if bits.over else BAD)


def index_carry(stream, frame, max_chunks=None, max_chunk_in=0):
    """what hipdeflate_stream_index_carry_dev answers -> (summary as a dict, in_off, in_len, out_size, out_off, reach): the
    tables hold the rows in front of where the chain ended, max_chunks at the most"""
    stream = bytes(stream)
    max_in = max_chunk_in or INFLATE_MAX_IN - 1
    s = {"nchunks": 0, "out_bytes": 0, "end_offset": 0, "ncandidates": 0, "hdr_bytes": 0, "status": 0}
    hdr, refused = header(stream, frame)
    if refused:
        s["status"] = refused
        return s, [], [], [], [], []
    end = len(stream) - TRAILER[frame]
    s["hdr_bytes"] = s["end_offset"] = hdr
    s["ncandidates"] = 1
    if end == hdr:
        s["status"] = 2
        return s, [], [], [], [], []
    cand = candidates(stream, frame, hdr)
    s["ncandidates"] = len(cand)
    on_list = set(cand)
    rows, c = [], hdr
    while True:
        v, stop, used, size, reach = piece(stream, c, min(max_in, end - c))
        if v != OK:
            s["end_offset"] = c
            s["status"] = 2 if v == CUT and end - c <= max_in else 1
            break
        rows.append((c, used, size, reach))
        if stop == FINAL:
            s["end_offset"] = c + used + TRAILER[frame]
            break
        c += used
        if c == end:                                   # a flush point is the last payload byte
            s["end_offset"], s["status"] = c, 2
            break
        assert c in on_list, c
    s["nchunks"] = len(rows)
    if max_chunks is not None and len(rows) > max_chunks:
        s["status"] = 3                                # ... unless a row of the table breaks the reach rule
        rows = rows[:max_chunks]
    out_off, t = [], 0
    for _, _, size, _ in rows:
        out_off.append(t)
        t += size
    s["out_bytes"] = t
    # the reach rule, on the rows in the table: the first row that reaches back over the start of the stream ends the chain
    for i, r in enumerate(rows):
        if r[3] > out_off[i]:
            s.update(status=1, end_offset=r[0], nchunks=i, out_bytes=out_off[i])
            rows, out_off = rows[:i], out_off[:i]
            break
    return s, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], out_off, [r[3] for r in rows]


def row(stream, p, n):
    """one row by the flush rule: pieces from stream[p] until a final block, or until the n bytes are used exactly
    -> (out_size, reach) or None"""
    used, nout, reach = 0, 0, 0
    while True:
        v, stop, u, size, r = piece(stream, p + used, n - used)
        if v != OK:
            return None
        if r > nout:
            reach = max(reach, r - nout)
        used, nout = used + u, nout + size
        if stop == FINAL or used == n:
            return nout, reach


def decode_carry(stream, frame, in_off, in_len, out_size, out_off, reach, out_cap=None, plain=None):
    """what hipdeflate_stream_inflate_carry_dev answers -> (summary as a dict, output or None).  summary["check"] is None
    where the header leaves it unspecified (a bad row) or nothing was decoded.  plain: the bytes of the rows by the
    caller's own reference (deflate_gen.expand of the token lists), taken where zlib refuses a row -- the forms only
    libdeflate decodes -- and held to zlib's where it does not."""
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
        fault = fault or reach[i] > WINDOW or reach[i] > out_off[i]
        if fault:
            return verdict(1, i), None
    total = out_off[-1] + out_size[-1]
    if out_cap is not None and out_cap < total:
        return verdict(3, n, total), None
    used = in_off[-1] + in_len[-1] + trl
    for i in range(n):
        r = row(stream, in_off[i], in_len[i])
        if r is None or r[0] != out_size[i] or r[1] > reach[i]:
            return verdict(2, i, total, used), None
    # every row decodes to its size within its reach, and no reach goes over the start of the stream: the rows' bytes are
    # those of one inflate over them
    try:
        d = zlib.decompressobj(-15)
        out = b"".join(d.decompress(stream[in_off[i]:in_off[i] + in_len[i]]) for i in range(n))
        assert plain is None or out == bytes(plain[:total])
    except zlib.error:
        assert plain is not None, "rows zlib refuses: the caller states their bytes"
        out = bytes(plain[:total])
    assert len(out) == total
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


# ---- writers ----------------------------------------------------------------------------------------------------------------

def sync_writer(pieces, frame, level=6):
    """ONE zlib object, Z_SYNC_FLUSH behind every piece but the last, Z_FINISH behind the last -> stream"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[frame])
    stream = b""
    for i, p in enumerate(pieces):
        stream += c.compress(p)
        if i + 1 < len(pieces):
            stream += c.flush(zlib.Z_SYNC_FLUSH)
    return stream + c.flush()


def pigz_writer(pieces, frame, level=6):
    """pigz's default form: every piece by a fresh raw compressor primed with the 32768 bytes in front of it, Z_SYNC_FLUSH
    behind every piece but the last, Z_FINISH behind the last -> stream"""
    body, plain = b"", b""
    for i, p in enumerate(pieces):
        prime = plain[-WINDOW:]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=prime) if prime else zlib.compressobj(level, zlib.DEFLATED, -15)
        body += c.compress(p) + (c.flush(zlib.Z_SYNC_FLUSH) if i + 1 < len(pieces) else c.flush())
        plain += p
    return HEADER[frame] + body + trailer(frame, plain)


def compose_rows(rows, frame):
    """hand-built rows: rows[i] a list of deflate_gen.Block whose tokens may name distances over the row's first byte; every
    row but the last ends in a flush point, the last in its final block -> (stream, plain)"""
    body, blocks = b"", []
    for i, r in enumerate(rows):
        last = i + 1 == len(rows)
        assert (bool(r) and r[-1].final) == last and not any(b.final for b in r[:-1]), i
        body += dg.encode(r, chunk=not last)
        blocks += r
    plain = dg.expand(blocks)
    return HEADER[frame] + body + trailer(frame, plain), plain


def cut(data, sizes):
    """data in pieces of the sizes given, the last repeated to the end"""
    out, o, i = [], 0, 0
    while o < len(data):
        k = sizes[min(i, len(sizes) - 1)]
        out.append(data[o:o + k])
        o, i = o + k, i + 1
    return out


def words(rng, n):
    """n bytes of word text: matches at every distance a window holds"""
    vocab = [bytes(rng.integers(97, 123, int(rng.integers(2, 10))).astype("uint8")) for _ in range(600)]
    out = bytearray()
    while len(out) < n:
        out += vocab[int(rng.integers(0, len(vocab)))] + b" "
    return bytes(out[:n])
