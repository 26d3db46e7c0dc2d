"""What include/hipdeflate.h promises about hipdeflate_index_members_any_dev, restated in plain Python: the serial walk over
a file of gzip members that may state no length -- from first_offset on, member after member, until the end -- and the
summary of how it stopped.  Nothing here is taken from hd_index.hpp: the header fields are those of
tests/framed_model.py (RFC 1952 as libdeflate_gzip_decompress_ex reads it), a stated length is
tests/member_index_model.member_len, and where a stream ends is what zlib.decompressobj(-15) says.

A candidate is a position p >= first_offset with 1f 8b 08 and FLG & 0xe0 == 0, all four bytes in front of nbytes.  The
member at a candidate is read from its window W = blob[p : min(nbytes, p + cap)]:
  rule A  FEXTRA is set and the extra field is one of the five known kinds (by XLEN and tag): member_len, cap unbounded;
  rule B  everything else: the header fields in stream order, the stream to the end of its final block, eight trailer bytes,
          ISIZE == the decoded length < 2^32; cap = max_member_in (0: MAX_IN - 1).
The first event in stream order decides: BAD for a byte that rules a member out, and for a needed byte at or behind the end
of W: CUT where W ends at nbytes, TOO_LONG where the cap ended it."""
import struct
import zlib

import framed_model
import member_index_model as mim

OK, BAD, CUT, TOO_SMALL, TOO_LONG = 0, 1, 2, 3, 4
MAX_IN = framed_model.MAX_IN
KNOWN = ((6, b"BC\x02\x00"), (8, b"MZ\x04\x00"), (20, b"IG\x10\x00"), (8, b"IG\x04\x00"))


def is_candidate(blob, p, nbytes):
    return p + 4 <= nbytes and blob[p:p + 3] == b"\x1f\x8b\x08" and not (blob[p + 3] & framed_model.FRESERVED)


def candidates(blob, first_offset=0, nbytes=None):
    """every candidate at or behind first_offset, ascending"""
    blob = bytes(blob)
    nbytes = len(blob) if nbytes is None else nbytes
    out, p = [], blob.find(b"\x1f\x8b\x08", first_offset, nbytes)
    while p >= 0:
        if is_candidate(blob, p, nbytes):
            out.append(p)
        p = blob.find(b"\x1f\x8b\x08", p + 1, nbytes)
    return out


def states_length(blob, p, nbytes):
    """rule A applies to the candidate at p: FEXTRA, and an extra field of one of the five kinds that lies in front of nbytes"""
    avail = nbytes - p
    if not (blob[p + 3] & framed_model.FEXTRA) or avail < 12:
        return False
    xlen = blob[p + 10] | blob[p + 11] << 8
    if avail < 12 + xlen:
        return False
    x = bytes(blob[p + 12:p + 12 + xlen])
    return (xlen, x[:4]) in KNOWN or (xlen == 4 and x[3] == 0x7d)


def header_len(w, flg):
    """the header fields of a rule-B member in stream order inside the window w -> the header's length, or None where a
    needed byte lies at or behind the end of w"""
    n, pos = len(w), 10
    if flg & framed_model.FEXTRA:
        if n < 12:
            return None
        pos = 12 + (w[10] | w[11] << 8)
    for bit in (framed_model.FNAME, framed_model.FCOMMENT):
        if flg & bit:
            z = w.find(b"\0", pos)
            if z < 0:
                return None
            pos = z + 1
    if flg & framed_model.FHCRC:
        pos += 2
    return pos if pos <= n else None


def sized_member(w):
    """rule B on the window w -> (OK, hdr, total, out_size) | (BAD, ...) | (None, ...) where the window ran out"""
    hdr = header_len(w, w[3]) if len(w) >= 4 else None
    if hdr is None:
        return None, 0, 0, 0
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(w[hdr:])
    except zlib.error:
        return BAD, 0, 0, 0
    if not d.eof:
        return None, 0, 0, 0
    rest = d.unused_data
    if len(rest) < 8:
        return None, 0, 0, 0
    if len(out) >= 1 << 32 or struct.unpack("<I", rest[4:8])[0] != len(out):
        return BAD, 0, 0, 0
    return OK, hdr, len(w) - len(rest) + 8, len(out)


def member(blob, p, nbytes, max_member_in=0):
    """the candidate at p -> (cls, hdr, total, out_size): cls OK | BAD | CUT | TOO_LONG; OK implies p + total <= nbytes"""
    if states_length(blob, p, nbytes):
        cls, hdr, total = mim.member_len(blob, p, nbytes)
        return cls, hdr, total, struct.unpack("<I", blob[p + total - 4:p + total])[0] if cls == OK else 0
    cap = max_member_in or MAX_IN - 1
    end = min(nbytes, p + cap)
    cls, hdr, total, size = sized_member(blob[p:end])
    if cls is None:
        cls = CUT if end == nbytes else TOO_LONG
    return cls, hdr, total, size


def walk(blob, first_offset=0, max_member_in=0, nbytes=None):
    """-> (rows, status, end_offset): rows = [(in_off, in_len, out_size, out_off, crc_want)] of the members in front of
    end_offset; status OK with end_offset == nbytes, or what sits at end_offset"""
    blob = bytes(blob)
    nbytes = len(blob) if nbytes is None else nbytes
    assert first_offset <= nbytes
    rows, p, out = [], first_offset, 0
    while p < nbytes:
        if not is_candidate(blob, p, nbytes):
            left = blob[p:nbytes]
            fits = len(left) < 4 and left == b"\x1f\x8b\x08"[:len(left)]
            return rows, CUT if fits else BAD, p
        cls, hdr, total, size = member(blob, p, nbytes, max_member_in)
        if cls != OK:
            return rows, cls, p
        crc = struct.unpack("<I", blob[p + total - 8:p + total - 4])[0]
        rows.append((p + hdr, total - hdr, size, out, crc))
        out += size
        p += total
    return rows, OK, p


def summary(blob, max_members, first_offset=0, max_member_in=0, nbytes=None):
    """what hipdeflate_member_any_summary holds and the rows the table holds -> (rows, dict of the six fields).  A table too
    small answers TOO_SMALL whatever else is wrong, as the member index does."""
    blob = bytes(blob)
    n_all = len(blob) if nbytes is None else nbytes
    rows, status, end = walk(blob, first_offset, max_member_in, n_all)
    n = len(rows)
    if n > max_members:
        rows, status = rows[:max_members], TOO_SMALL
    cand = candidates(blob, first_offset, n_all)
    return rows, {"nmembers": n, "out_bytes": sum(r[2] for r in rows), "end_offset": end, "ncandidates": len(cand),
                  "nsized": sum(1 for p in cand if not states_length(blob, p, n_all)), "status": status}


def plain_member(payload, level=6, flg=0, extra=b"", fname=b"", fcomment=b"", strategy=zlib.Z_DEFAULT_STRATEGY, crc=None, isize=None):
    """one gzip member without a known length field; the optional fields follow flg (extra: the bytes behind XLEN)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    stream = c.compress(payload) + c.flush()
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if flg & framed_model.FEXTRA:
        head += struct.pack("<H", len(extra)) + extra
    if flg & framed_model.FNAME:
        head += fname + b"\0"
    if flg & framed_model.FCOMMENT:
        head += fcomment + b"\0"
    if flg & framed_model.FHCRC:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + stream + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)
