"""What include/hipdeflate.h promises about hipdeflate_read_ranges_dev, restated in plain Python on the rows of
member_index_model.walk(): which ranges are accepted, how long each is, where its bytes go, and which members must be
decoded for them.  Nothing here is taken from hd_range.hpp: no scan, no difference array, no binary search -- every
query is held against every member (numpy does that comparison for all members at once, to keep 2049 x 2049 quick).
tests/test_range_read_model.py holds it to data[begin:end] of the zlib-decoded file, tests/test_gpu_range_read.py holds
the device to it, bit for bit.

A row is (in_off, in_len, out_size, out_off, crc_want); in_len counts the 8-byte trailer, so member i starts where member
i - 1 ends: at in_off[i-1] + in_len[i-1], and member 0 at 0 -- whatever kind of header the members carry."""
import numpy as np

BYTES, VOFFSET = 0, 1
OK, REFUSED, TOO_LONG = 0, 1, 2


def voffset(coffset, uoffset):
    return (coffset << 16) | (uoffset & 0xffff)


def total_of(rows):
    return rows[-1][3] + rows[-1][2] if rows else 0


def member_starts(rows):
    """-> ([start of member i], end of the file)"""
    starts, p = [], 0
    for r in rows:
        starts.append(p)
        p = r[0] + r[1]
    return starts, p


def position(rows, v):
    """U(v): the decoded position a virtual offset names, None if it names none"""
    starts, end = member_starts(rows)
    c, u = v >> 16, v & 0xffff
    for m, s in enumerate(starts):
        if s == c:
            return rows[m][3] + u if u <= rows[m][2] else None
    if c == end and u == 0:
        return total_of(rows)
    return None


def resolve(rows, kind, begin, end):
    """-> (status, first byte, one past the last byte) in the decoded file; the span is empty unless status is OK"""
    total = total_of(rows)
    if kind == VOFFSET:
        b, e = position(rows, begin), position(rows, end)
        if b is None or e is None or b > e:
            return REFUSED, 0, 0
    else:
        if begin > end:
            return REFUSED, 0, 0
        b, e = min(begin, total), min(end, total)
    if e - b >= 1 << 32:
        return TOO_LONG, 0, 0
    return OK, b, e


def plan(rows, kind, begins, ends):
    """-> dict: q_len, q_status, dst_off (lists), spans [(b, e)], selected (sorted member indices), out_bytes, nselected,
    sel_bytes, nrefused"""
    q_len, q_status, dst_off, spans, at = [], [], [], [], 0
    first = np.array([r[3] for r in rows], dtype=np.int64)             # a member's bytes: [first, behind)
    behind = first + np.array([r[2] for r in rows], dtype=np.int64)
    taken = np.zeros(len(rows), dtype=bool)
    for begin, end in zip(begins, ends):
        status, b, e = resolve(rows, kind, begin, end)
        q_status.append(status)
        q_len.append(e - b)
        dst_off.append(at)
        spans.append((b, e))
        at += e - b
        taken |= np.maximum(first, b) < np.minimum(behind, e)       # a member is selected if the query takes a byte of it
    selected = [int(m) for m in np.flatnonzero(taken)]
    return {"q_len": q_len, "q_status": q_status, "dst_off": dst_off, "spans": spans, "selected": selected,
            "out_bytes": at, "nselected": len(selected), "sel_bytes": sum(rows[m][2] for m in selected),
            "nrefused": sum(1 for s in q_status if s)}
