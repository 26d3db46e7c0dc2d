"""What include/hipdeflate.h promises about hipdeflate_index_members_dev, restated in plain Python: the serial walk over
a stream of gzip members -- member_len() of 7bgzf_amd/csrc/hd_bgzf_host.c applied at byte 0, then behind every member,
until the end -- and the summary of how it stopped.  Nothing here is taken from hd_index.hpp;
tests/test_member_index_model.py holds it to the oracle's _read_gz_header, to bgzf_scan and to the corrupt files of
tests/test_host_cli.py, tests/test_gpu_member_index.py holds the device index to it, bit for bit.

member_len() answers 0 both for "these bytes are not a member" and for "the bytes ran out"; the summary tells them apart:
  BAD (status 1)  the bytes that are there rule a member out: magic / CM / FLG (FEXTRA missing, a reserved bit set), an
                  extra field of no known kind, a length below header + trailer or above 0xfffffff0;
  CUT (status 2)  they run out first: fewer than 12 bytes (their magic fitting as far as it goes), fewer than 12 + XLEN,
                  a FNAME / FCOMMENT without its NUL, no room for FHCRC, or a member reaching past the end.
The checks come in member_len()'s order, so a header that is both (XLEN past the end AND of no known kind) is CUT."""
import struct

OK, BAD, CUT, TOO_SMALL = 0, 1, 2, 3


def member_len(blob, p, nbytes=None):
    """-> (OK, hdr, total) | (BAD, 0, 0) | (CUT, 0, 0) for the member at p < nbytes; OK implies p + total <= nbytes"""
    n_all = len(blob) if nbytes is None else nbytes
    avail = n_all - p
    assert avail > 0
    b = blob[p:p + 4]
    if b[0] != 0x1f or (avail > 1 and b[1] != 0x8b) or (avail > 2 and b[2] != 8) or \
            (avail > 3 and ((b[3] & 0xe0) or not (b[3] & 4))):
        return BAD, 0, 0
    if avail < 12:
        return CUT, 0, 0
    flg = blob[p + 3]
    xlen = blob[p + 10] | blob[p + 11] << 8
    if avail < 12 + xlen:
        return CUT, 0, 0
    n = 12 + xlen
    for bit in (0x08, 0x10):
        if flg & bit:
            z = blob.find(b"\0", p + n, n_all)
            if z < 0:
                return CUT, 0, 0
            n = z - p + 1
    if flg & 0x02:
        n += 2
    if n > avail:
        return CUT, 0, 0
    x = bytes(blob[p + 12:p + 12 + xlen])
    if xlen == 6 and x[:4] == b"BC\x02\x00":
        t = struct.unpack("<H", x[4:6])[0] + 1
    elif xlen == 8 and x[:4] == b"MZ\x04\x00":
        t = struct.unpack("<I", x[4:8])[0] + n + 8
    elif xlen == 20 and x[:4] == b"IG\x10\x00":
        t = struct.unpack("<Q", x[4:12])[0]
    elif xlen == 8 and x[:4] == b"IG\x04\x00":
        t = struct.unpack("<I", x[4:8])[0]
    elif xlen == 4 and x[3] == 0x7d:
        t = struct.unpack("<I", x)[0] & 0xffffff
    else:
        return BAD, 0, 0
    if t < n + 8 or t > 0xfffffff0:
        return BAD, 0, 0
    if t > avail:
        return CUT, 0, 0
    return OK, n, t


def walk(blob, nbytes=None):
    """-> (rows, status, end_offset): rows = [(in_off, in_len, out_size, out_off, crc_want)] of the members in front of
    end_offset; status OK with end_offset == nbytes, or BAD / CUT for what sits at end_offset"""
    blob = bytes(blob)
    nbytes = len(blob) if nbytes is None else nbytes
    rows, p, out = [], 0, 0
    while p < nbytes:
        cls, hdr, total = member_len(blob, p, nbytes)
        if cls != OK:
            return rows, cls, p
        crc, isize = struct.unpack("<II", blob[p + total - 8:p + total])
        rows.append((p + hdr, total - hdr, isize, out, crc))
        out += isize
        p += total
    return rows, OK, p


def summary(blob, max_members, nbytes=None):
    """what hipdeflate_member_summary holds and the rows the table holds: -> (rows, nmembers, out_bytes, end_offset, status).
    A table too small answers TOO_SMALL whatever else is wrong: nmembers is the count the stream has, the rows are the
    first max_members and out_bytes is theirs."""
    rows, status, end = walk(blob, nbytes)
    n = len(rows)
    if n > max_members:
        rows, status = rows[:max_members], TOO_SMALL
    return rows, n, sum(r[2] for r in rows), end, status


def gz_member(kind, payload, crc, isize, fname=b"", fcomment=b"", fhcrc=False):
    """one gzip member whose extra field carries the member length in each of the five ways _read_gz_header
    (applet/7bgzf.c:111-129) understands: BC, MZ, IG1, IG2, MG (tests/test_host_cli.py::_gz_member, with FCOMMENT and
    FHCRC added)"""
    flg = 4 | (8 if fname else 0) | (16 if fcomment else 0) | (2 if fhcrc else 0)
    tail = (fname + b"\0" if fname else b"") + (fcomment + b"\0" if fcomment else b"") + (b"\x12\x34" if fhcrc else b"")
    xlen = {"BC": 6, "MZ": 8, "IG1": 20, "IG2": 8, "MG": 4}[kind]
    total = 12 + xlen + len(tail) + len(payload) + 8
    if kind == "BC":
        extra = b"BC\x02\x00" + struct.pack("<H", total - 1)
    elif kind == "MZ":
        extra = b"MZ\x04\x00" + struct.pack("<I", len(payload))
    elif kind == "IG1":
        extra = b"IG\x10\x00" + struct.pack("<QQ", total, isize)
    elif kind == "IG2":
        extra = b"IG\x04\x00" + struct.pack("<I", total)
    else:
        extra = struct.pack("<I", total)[:3] + b"\x7d"
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra + tail
    return head + payload + struct.pack("<II", crc, isize)
