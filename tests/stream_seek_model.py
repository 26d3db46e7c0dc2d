"""Plain-Python model of the seek index (include/hipdeflate.h, "a SEEK INDEX on either table"): what
hipdeflate_stream_windows_dev and hipdeflate_stream_read_ranges_dev answer, every field and the bytes.
  * windows(): the table check of the output-side columns, win_off, the window bytes and the rows' CRC-32 from the plain bytes;
  * read(): the verdicts in the header's order -- the table by the rules of its unit's decode call and the window offsets, the
    queries by range_read_model.resolve / plan, the selected rows by the `row` functions of stream_carry_model /
    stream_blocks_model (size and reach, by the unit's end rule) -- and the bytes of a row through ONE zlib.decompressobj
    whose dictionary is the row's window alone, the reach[i] bytes the index keeps: nothing in front of them exists for it.
A table is the five columns (in_off, in_len, out_size, out_off, reach) as lists.  No GPU, no product code.
tests/test_stream_seek_model.py holds it to zlib."""
import bisect
import zlib

import range_read_model as rr
import stream_blocks_model as bm
import stream_carry_model as cm
from stream_index_model import INFLATE_MAX_IN, TRAILER, header

WINDOW = 32768
BYTES, BITS = 0, 1                   # HD_ROWS_BYTES, HD_ROWS_BITS
_rows = {}                           # (stream, unit, in_off, in_len) -> (out_size, reach) or None: a row's verdict, decoded once


def windows(table, plain, win_cap=None):
    """what hipdeflate_stream_windows_dev answers for the decoded stream `plain` -> (summary as a dict, win_off or None, win or
    None, row_check or None).  win_cap None: room enough."""
    _, _, out_size, out_off, reach = table
    n = len(out_size)

    def verdict(status, bad, win_bytes=0):
        return {"win_bytes": win_bytes, "bad_row": bad, "status": status}

    if n == 0:
        return verdict(1, 0), None, None, None
    for i in range(n):
        nxt = out_off[i + 1] if i + 1 < n else len(plain)
        if (i == 0 and out_off[0] != 0) or nxt - out_off[i] != out_size[i] or reach[i] > WINDOW or reach[i] > out_off[i]:
            return verdict(1, i), None, None, None
    win_off, t = [], 0
    for r in reach:
        win_off.append(t)
        t += r
    win_off.append(t)
    if win_cap is not None and win_cap < t:
        return verdict(3, n, t), win_off, None, None
    win = b"".join(bytes(plain[out_off[i] - reach[i]:out_off[i]]) for i in range(n))
    row_check = [zlib.crc32(bytes(plain[out_off[i]:out_off[i] + out_size[i]])) for i in range(n)]
    return verdict(0, n, t), win_off, win, row_check


def table_fault(table, unit, stream, frame, win_off, win_bytes):
    """the lowest row that breaks a rule of status 1, len(rows) for the header, None where the table stands"""
    in_off, in_len, out_size, out_off, reach = table
    n = len(in_off)
    hdr, refused = header(stream, frame)
    if refused:
        return n
    k = 8 if unit == BITS else 1
    lo, end = k * hdr, k * (len(stream) - TRAILER[frame])
    for i in range(n):
        o, ln = in_off[i], in_len[i]
        fault = ln >= (1 << 31 if unit == BITS else INFLATE_MAX_IN) or o < lo or o > end or ln > end - o or (i == 0 and out_off[0] != 0)
        if i + 1 < n:
            fault = fault or in_off[i + 1] < o + ln or out_off[i + 1] != out_off[i] + out_size[i]
        fault = fault or reach[i] > WINDOW or reach[i] > out_off[i]
        fault = fault or (i == 0 and win_off[0] != 0) or win_off[i + 1] - win_off[i] != reach[i] or win_off[i + 1] > win_bytes
        if fault:
            return i
    return None


def row_verdict(stream, unit, o, ln, end):
    """(out_size, reach) of the row at o, ln by its unit's end rule, None where it does not decode"""
    key = (stream, unit, o, ln)
    if key not in _rows:
        _rows[key] = bm.row(stream, o, ln, end) if unit == BITS else cm.row(stream, o, ln)
    return _rows[key]


def row_bytes(stream, unit, o, ln, end, size, window):
    """the row's bytes by zlib, which is given the row's bits and its window and nothing else; None where zlib refuses them"""
    data = bm.row_bits(stream, o, ln, end) if unit == BITS else stream[o:o + ln]
    try:
        d = zlib.decompressobj(-15, zdict=bytes(window)) if window else zlib.decompressobj(-15)
        out = d.decompress(data, size) if size else b""
    except zlib.error:
        return None
    return out if len(out) == size else None


def read(table, unit, stream, frame, wins, row_check, begins, ends, dst_cap=None, win_bytes=None, plain=None):
    """what hipdeflate_stream_read_ranges_dev answers -> dict: summary (out_bytes, nselected, sel_bytes, nrefused, bad_member,
    status), q_len, q_status, dst_off (None with status 1: not written), dst (bytes; None where nothing is decoded), exact
    (by query: its bytes are specified), selected.  wins = (win_off, win); win_bytes None: len(win); dst_cap None: room
    enough.  plain: the stream's bytes by the caller's own reference, taken for a row zlib refuses (the forms only libdeflate
    decodes) -- such a row's window must be the untampered one."""
    stream = bytes(stream)
    in_off, in_len, out_size, out_off, reach = table
    win_off, win = wins
    n, nq = len(in_off), len(begins)
    win_bytes = len(win) if win_bytes is None else win_bytes
    s = {"out_bytes": 0, "nselected": 0, "sel_bytes": 0, "nrefused": 0, "bad_member": n, "status": 0}
    res = {"summary": s, "q_len": None, "q_status": None, "dst_off": None, "dst": None, "exact": [True] * nq, "selected": []}
    if n == 0 or nq == 0:
        return res
    bad = table_fault(table, unit, stream, frame, win_off, win_bytes)
    if bad is not None:
        s.update(status=1, bad_member=bad)
        return res
    rows = [(in_off[i], in_len[i], out_size[i], out_off[i], 0) for i in range(n)]
    p = rr.plan(rows, rr.BYTES, begins, ends)
    s.update(out_bytes=p["out_bytes"], nselected=p["nselected"], sel_bytes=p["sel_bytes"], nrefused=p["nrefused"])
    res.update(q_len=p["q_len"], q_status=p["q_status"], dst_off=p["dst_off"], selected=p["selected"])
    if dst_cap is not None and p["out_bytes"] > dst_cap:
        s["status"] = 3
        return res
    end = len(stream) - TRAILER[frame]
    got, failed = {}, []
    for i in p["selected"]:
        v = row_verdict(stream, unit, in_off[i], in_len[i], end)
        if v is None or v[0] != out_size[i] or v[1] > reach[i]:
            failed.append(i)
            continue
        b = row_bytes(stream, unit, in_off[i], in_len[i], end, out_size[i], win[win_off[i]:win_off[i] + reach[i]])
        if b is None:
            assert plain is not None, "a row zlib refuses: the caller states its bytes"
            b = bytes(plain[out_off[i]:out_off[i] + out_size[i]])
        if row_check is not None and zlib.crc32(b) != row_check[i]:
            failed.append(i)
        got[i] = b
    if failed:
        s.update(status=2, bad_member=failed[0])
    dst = bytearray(p["out_bytes"])
    sel_off = [out_off[i] for i in p["selected"]]
    for q, (b, e) in enumerate(p["spans"]):
        at = p["dst_off"][q]
        for k in range(max(bisect.bisect_right(sel_off, b) - 1, 0), len(sel_off)):
            i = p["selected"][k]
            if out_off[i] >= e:
                break
            lo, hi = max(b, out_off[i]), min(e, out_off[i] + out_size[i])
            if lo >= hi:
                continue
            if i in got and i not in failed:
                dst[at + lo - b:at + hi - b] = got[i][lo - out_off[i]:hi - out_off[i]]
            else:
                res["exact"][q] = False
    res["dst"] = bytes(dst)
    return res
