"""Plain-Python model of the block index and the block decode (include/hipdeflate.h, "a PLAIN stream, which has no flush
point at all"): stream_carry_model with bit positions and a header rule in the place of byte positions and the marker.
  * header_rule(): the filter at one bit position; candidates(): the first payload bit and every later position of the
    payload region that passes it (numpy over all positions at once; brute_candidates() is the loop it is held to);
  * piece(): stream_carry_model.piece started on a bit, stopped behind a final block or in front of BFINAL 0 / BTYPE 2, its
    input counted in bits;
  * index_blocks(): the chain from candidate 0, the merge into rows, the reach rule and the long-row rule, the summary;
  * decode_blocks(): the verdicts of the decode on a table, in the header's order; the bytes of a row through zlib on the
    row's bits shifted to a byte boundary, with the 32 KiB in front of it as the dictionary.
No GPU, no product code.  tests/test_stream_blocks_model.py holds it to zlib."""
import zlib

import numpy as np

from deflate_gen import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, PRECODE_ORDER
from deflate_tokens import Block, DeflateError, _dynamic_header, _static_tables
from stream_index_model import (BAD, CUT, FINAL, FRAME_GZIP, FRAME_RAW, FRAME_ZLIB, HEADER, INFLATE_MAX_IN, OK, TRAILER, WBITS, _Bits,
                                header, trailer)

WINDOW = 32768
NEXT = 3                             # the stop of a piece in front of a non-final dynamic header (hd_inflate_size.hpp PIECE_NEXT)
ROW_BYTES = 128 << 10                # include/hipdeflate_params.h HD_BLOCK_ROW_BYTES
NO, YES, SHORT = 0, 1, 2             # the header rule's verdicts (hipdeflate_test_block_headers_dev)
PASS_RATE = 5.13e-4                  # of random positions, as the header states it


def header_rule(stream, p, end):
    """the rule at bit p of stream[:end] -> NO | YES | SHORT (the header does not fit in front of bit 8 * end)"""
    left = 8 * end - p
    if left < 3:
        return SHORT
    v = int.from_bytes(stream[p >> 3:min((p >> 3) + 12, end)], "little") >> (p & 7)
    if v & 7 != 4:                                      # BFINAL 0, BTYPE 2
        return NO
    if left < 17:
        return SHORT
    npre = 4 + ((v >> 13) & 15)
    if left < 17 + 3 * npre:
        return SHORT
    lens = [(v >> (17 + 3 * i)) & 7 for i in range(npre)]
    k = sum(128 >> l for l in lens if l)
    return YES if k in (0, 128) or [l for l in lens if l] == [1] else NO


def brute_candidates(stream, hdr, end):
    return [8 * hdr] + [p for p in range(8 * hdr + 1, 8 * end) if header_rule(stream, p, end) == YES]


def candidates(stream, hdr, end):
    """the first payload bit, then every bit position behind it, in front of 8 * end, that passes the rule"""
    bits = np.unpackbits(np.frombuffer(bytes(stream[:end]) + bytes(16), dtype=np.uint8), bitorder="little")
    nb = 8 * end
    p = np.flatnonzero((bits[:nb] == 0) & (bits[1:nb + 1] == 0) & (bits[2:nb + 2] == 1))
    p = p[(p > 8 * hdr) & (p + 17 <= nb)]
    npre = 4 + bits[p + 13] + 2 * bits[p + 14] + 4 * bits[p + 15] + 8 * bits[p + 16].astype(np.int64)
    keep = p + 17 + 3 * npre <= nb
    p, npre = p[keep], npre[keep]
    at = p[:, None] + 17 + 3 * np.arange(19)[None, :]
    lens = (bits[at] + 2 * bits[at + 1] + 4 * bits[at + 2]).astype(np.int64)
    lens[np.arange(19)[None, :] >= npre[:, None]] = 0
    k = np.where(lens > 0, 128 >> lens, 0).sum(axis=1)
    nz = (lens > 0).sum(axis=1)
    ok = (k == 128) | (k == 0) | ((k == 64) & (nz == 1))
    return [8 * hdr] + [int(v) for v in p[ok]]


def pass_rate():
    """the share of random bit strings the rule passes, exactly: P(BFINAL 0, BTYPE 2) = 1 / 8, HCLEN uniform, and the
    distribution of K = sum 2^(7 - len) over n uniform 3-bit lengths by dynamic programming -> a Fraction"""
    from fractions import Fraction
    total = Fraction(0)
    for npre in range(4, 20):
        dist = {(0, 0): Fraction(1)}                    # (K capped at 129, non-zero lengths capped at 2) -> probability
        for _ in range(npre):
            nxt = {}
            for (k, nz), pr in dist.items():
                for l in range(8):
                    key = (min(k + (128 >> l if l else 0), 129), min(nz + (l != 0), 2))
                    nxt[key] = nxt.get(key, 0) + pr / 8
            dist = nxt
        total += sum(pr for (k, nz), pr in dist.items() if k in (0, 128) or (k == 64 and nz == 1)) / 16
    return total / 8


def piece(stream, p, n):
    """the piece that starts at BIT p, over the n bytes from the byte that bit lies in -> (verdict, stop, in_used in BITS from
    p, out_size, reach).  It ends behind a final block, or behind a non-final block whose following three bits, all inside
    the input, read BFINAL 0 / BTYPE 2; a flush point is no stop."""
    o = p >> 3
    bits = _Bits(stream[o:o + n])
    bits.pos = p & 7
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
                    k = s - 257
                    length = LEN_BASE[k] + bits.get(LEN_EXTRA[k])
                    ds = bits.sym(dt, dm)
                    d = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                    if bits.over:
                        return fail(CUT)
                    if d > nout:
                        reach = max(reach, d - nout)
                    nout += length
            if nout > 0xffffffff:
                return fail(3)                          # (HD_INSUFFICIENT_SPACE: no test stream is that long)
            if final:
                return OK, FINAL, bits.pos - (p & 7), nout, reach
            at = bits.pos
            if at + 3 <= bits.nbits and bits.get(3) == 4:
                return OK, NEXT, at - (p & 7), nout, reach
            bits.pos = at
    except DeflateError:
        return fail(CUT if bits.over else BAD)


def chain(stream, frame, max_chunk_in=0):
    """-> (hdr, refused, cand, pieces as (bit, used bits, out_size, reach), end_bit, status 0 | 1 | 2)"""
    stream = bytes(stream)
    max_in = max_chunk_in or INFLATE_MAX_IN - 1
    hdr, refused = header(stream, frame)
    if refused:
        return 0, refused, [], [], 0, refused
    end = len(stream) - TRAILER[frame]
    if end == hdr:
        return hdr, 0, [8 * hdr], [], 8 * hdr, 2
    cand = candidates(stream, hdr, end)
    on_list = set(cand)
    pieces, c = [], 8 * hdr
    while True:
        left = end - (c >> 3)
        v, stop, used, size, reach = piece(stream, c, min(max_in, left))
        if v != OK:
            return hdr, 0, cand, pieces, c, 2 if v == CUT and left <= max_in else 1
        pieces.append((c, used, size, reach))
        c += used
        if stop == FINAL:
            return hdr, 0, cand, pieces, c, 0
        if c not in on_list:                           # the filter refuses what stands there, or it does not fit
            return hdr, 0, cand, pieces, c, 2 if header_rule(stream, c, end) == SHORT else 1


def merge(pieces, row_bytes):
    """-> rows as [in_off, in_len, out_size, out_off, reach]: the runs of pieces whose out_off lies in one multiple of row_bytes"""
    rows, off = [], 0
    for c, used, size, reach in pieces:
        if not rows or off // row_bytes != (off - prev_size) // row_bytes:
            rows.append([c, 0, 0, off, 0])
        r = rows[-1]
        r[4] = max(r[4], reach - (off - r[3]))
        r[1] += used
        r[2] += size
        off, prev_size = off + size, size
    return rows


def index_blocks(stream, frame, max_rows=None, max_chunk_in=0, row_bytes=0):
    """what hipdeflate_stream_index_blocks_dev answers -> (summary as a dict, in_off, in_len, out_size, out_off, reach): the
    tables hold the rows in front of where the chain ended, max_rows at the most"""
    stream = bytes(stream)
    max_in = max_chunk_in or INFLATE_MAX_IN - 1
    s = {"nrows": 0, "npieces": 0, "out_bytes": 0, "end_offset": 0, "end_bit": 0, "ncandidates": 0, "hdr_bytes": 0, "status": 0}
    hdr, refused, cand, pieces, end_bit, status = chain(stream, frame, max_chunk_in)
    if refused:
        s["status"] = refused
        return s, [], [], [], [], []
    rows = merge(pieces, row_bytes or ROW_BYTES)
    s.update(hdr_bytes=hdr, ncandidates=len(cand), npieces=len(pieces), nrows=len(rows), end_bit=end_bit, status=status)
    if max_rows is not None and len(rows) > max_rows:
        s["status"] = 3
        rows = rows[:max_rows]
    s["out_bytes"] = sum(r[2] for r in rows)
    for i, r in enumerate(rows):                       # the reach rule and the long-row rule, on the rows in the table
        if r[4] > r[3] or r[1] > 8 * max_in:
            s.update(status=1, end_bit=r[0], nrows=i, out_bytes=r[3])
            rows = rows[:i]
            break
    s["end_offset"] = ((s["end_bit"] + 7) >> 3) + TRAILER[frame] if s["status"] == 0 else s["end_bit"] >> 3
    return (s,) + tuple([r[k] for r in rows] for k in range(5))


def shifted(stream, bit, end):
    """the bits of stream[:end] from `bit` on, moved to a byte boundary"""
    return (int.from_bytes(stream[bit >> 3:end], "little") >> (bit & 7)).to_bytes(end - (bit >> 3), "little")


def row_bits(stream, bit, nbits, end):
    """the nbits bits of stream[:end] from `bit` on, moved to a byte boundary, zeros behind them in the last byte: zlib given
    these never looks at what stands behind the row"""
    v = (int.from_bytes(stream[bit >> 3:min(end, (bit + nbits + 15) >> 3)], "little") >> (bit & 7)) & ((1 << nbits) - 1)
    return v.to_bytes((nbits + 7) >> 3, "little")


def row(stream, p, nbits, end):
    """one row by the rule of bit rows: pieces from bit p until a final block whose end lies at or in front of p + nbits, or
    until a block ends on bit p + nbits exactly -> (out_size, reach) or None"""
    o = p >> 3
    data = stream[o:o + ((p & 7) + nbits + 7 >> 3)]
    bits = _Bits(data)
    bits.pos = p & 7
    stop_at = (p & 7) + nbits
    nout, reach = 0, 0
    try:
        while True:
            final, btype = bits.get(1), bits.get(2)
            if btype == 3 or bits.pos > stop_at:
                return None
            if btype == 0:
                bits.pos = (bits.pos + 7) & ~7
                if bits.pos + 32 > bits.nbits:
                    return None
                ln, nl = bits.get(16), bits.get(16)
                if ln != (~nl & 0xffff) or (bits.pos >> 3) + ln > len(data):
                    return None
                bits.pos += 8 * ln
                nout += ln
            else:
                if btype == 1:
                    (lt, lm), (dt, dm) = _static_tables()
                else:
                    (lt, lm), (dt, dm) = _dynamic_header(bits, Block("dynamic", bool(final), 0, 0), oracle=True)
                while True:
                    s = bits.sym(lt, lm)
                    if bits.pos > stop_at:
                        return None
                    if s < 256:
                        nout += 1
                        continue
                    if s == 256:
                        break
                    k = s - 257
                    length = LEN_BASE[k] + bits.get(LEN_EXTRA[k])
                    ds = bits.sym(dt, dm)
                    d = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                    if d > nout:
                        reach = max(reach, d - nout)
                    nout += length
            if bits.pos > stop_at:
                return None
            if final or bits.pos == stop_at:
                return nout, reach
    except DeflateError:
        return None


def decode_blocks(stream, frame, in_off, in_len, out_size, out_off, reach, out_cap=None, plain=None):
    """what hipdeflate_stream_inflate_blocks_dev answers -> (summary as a dict, output or None).  summary["check"] is None
    where the header leaves it unspecified (a bad row) or nothing was decoded.  plain: the bytes of the rows by the caller's
    own reference, taken where zlib refuses a row (the forms only libdeflate decodes)."""
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
        fault = ln >= 1 << 31 or o < 8 * hdr or o > 8 * end or ln > 8 * end - o or (i == 0 and out_off[0] != 0)
        if i + 1 < n:
            fault = fault or in_off[i + 1] < o + ln or out_off[i + 1] != out_off[i] + out_size[i]
        fault = fault or reach[i] > WINDOW or reach[i] > out_off[i]
        if fault:
            return verdict(1, i), None
    total = out_off[-1] + out_size[-1]
    if out_cap is not None and out_cap < total:
        return verdict(3, n, total), None
    used = ((in_off[-1] + in_len[-1] + 7) >> 3) + trl
    for i in range(n):
        r = row(stream, in_off[i], in_len[i], end)
        if r is None or r[0] != out_size[i] or r[1] > reach[i]:
            return verdict(2, i, total, used), None
    out = b""
    for i in range(n):
        try:
            d = zlib.decompressobj(-15, zdict=out[max(0, out_off[i] - WINDOW):out_off[i]])
            b = d.decompress(row_bits(stream, in_off[i], in_len[i], end), out_size[i]) if out_size[i] else b""
            assert len(b) == out_size[i] and (plain is None or b == bytes(plain[out_off[i]:out_off[i] + out_size[i]]))
        except zlib.error:
            assert plain is not None, "rows zlib refuses: the caller states their bytes"
            b = bytes(plain[out_off[i]:out_off[i] + out_size[i]])
        out += b
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

def plain_writer(data, frame, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    """ONE zlib object and no flush: what gzip, zlib.compress and a PNG writer put out"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[frame], mem_level, strategy)
    return c.compress(data) + c.flush()


def decoy_stream(frame, rng):
    """a stored block whose payload holds a complete non-final dynamic block at each of the eight bit shifts, then a final
    dynamic block -> (stream, plain, the eight bit positions of the decoys in the stream)"""
    import deflate_gen as dg
    inner = dg.encode([dg.Block("dynamic", [int(v) for v in rng.integers(97, 123, 60)] + [(20, 7)]), dg.Block("stored", final=True)])
    inner = inner[:-4]                                 # (without the LEN / NLEN of the closing stored block)
    payload, at = b"", []
    for k in range(8):
        v = int.from_bytes(inner, "little") << k
        at.append(8 * len(payload) + k)
        payload += v.to_bytes(len(inner) + 1, "little") + bytes([0xff] * 3)
    blocks = [dg.Block("stored", data=payload), dg.Block("dynamic", [int(v) for v in rng.integers(97, 123, 200)] + [(30, 11)], final=True)]
    body, plain = dg.encode(blocks), dg.expand(blocks)
    base = 8 * (len(HEADER[frame]) + 5)                # the stored block's header: three bits, padding, LEN, NLEN
    return HEADER[frame] + body + trailer(frame, plain), plain, [base + a for a in at]
