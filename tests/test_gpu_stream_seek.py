"""The seek index -- hipdeflate_stream_windows_dev, hipdeflate_stream_read_ranges_dev and device.SeekIndex -- against the
plain-Python model of tests/stream_seek_model.py.  Bit-exact: every field of both summaries, win_off, the window bytes, the
rows' checks, dst_off / q_len / q_status, the bytes of every query the contract specifies; 64 sentinel bytes around every dst
and every win; hipdeflate_stall_count() stays 0.  No case provokes a fault: every refusal is a verdict the contract of
include/hipdeflate.h defines, each runs once, and none reads or writes outside its buffers.  Every case decodes 600,000 bytes
at the most (the carry_ring streams: 1.5 MB).

Where the cases land (hd_seek.hpp):
  * k_seek_resolve's fast path (eight symbols, no marker, one row) and its symbol-by-symbol path: rows of 1 byte (row_bytes 1:
    every lane straddles a row edge), rows whose every symbol is a marker (carry_ring's all_markers rows, reach exactly 32768),
    a reach of 1 (ring_source_slot_*_back_1), a group base that is no multiple of 8 (every group but a read's first),
    pieces with one row and with many (the uniform search and the per-lane one);
  * groups of 4096 / 65536 / the default, counted in SELECTED output; ranges across a row edge and across a group edge;
  * rows of size 0 between selected rows (a writer's two flushes in a row: never selected, never decoded);
  * a full-flush stream: all reach 0, win_bytes 0, no window memory at all.
carry_rows.marker_path_rows is a predicate, not a family of streams: it is used here to state that the carry_ring tables read
below are ones whose every row would take the marker path in the full decode too.
The 2^32-byte query (q_status 2) is not crossed on the device in this change: the model test holds the rule, and
k_range_resolve, which applies it, is the member call's kernel, held to it there."""
import importlib
import os

import numpy as np
import pytest

import blocks_dev as bd
import carry_rows as cr
import deflate_gen as dg
import hdtest
import stream_blocks_model as bm
import stream_carry_model as cm
import stream_index_model as m
import stream_seek_model as sm
from carry_dev import GUARD, GZIP, RAW, SENT, ZLIB, fields, to_dev, u32, u64
from stream_seek_model import BITS, BYTES

pytestmark = pytest.mark.gpu
W_FIELDS = ("win_bytes", "bad_row", "status")
R_FIELDS = ("out_bytes", "nselected", "sel_bytes", "nrefused", "bad_member", "status")
_cache = {}


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def dev():
    return importlib.import_module("7bgzf_amd.device")


@pytest.fixture(autouse=True)
def no_stalls(pkg):
    yield
    pkg.lib().hipdeflate_test_carry_group(0)
    assert pkg.lib().hipdeflate_stall_count() == 0


# ---- one index on the device, held to the model ---------------------------------------------------------------------------------

class Index:
    """the device's tables, windows and checks of one stream -- made by the full decode and the windows call, and held to the
    model's while they are made"""

    def __init__(self, torch, dev, stream, frame, unit, table, plain):
        self.stream, self.frame, self.unit, self.table, self.plain = bytes(stream), frame, unit, [list(c) for c in table], bytes(plain)
        n = self.n = len(table[0])
        self.d_stream = to_dev(torch, stream)
        self.cols = [u64(torch, table[0]), u32(torch, table[1]), u32(torch, table[2]), u64(torch, table[3]), u32(torch, table[4])]
        out = torch.full((len(plain) + 1,), SENT, dtype=torch.uint8, device="cuda")[1:]          # (no alignment is asked of out)
        decode = dev.inflate_stream_blocks_call if unit == BITS else dev.inflate_stream_carry_call
        s = decode(self.d_stream, frame, *self.cols, n, out, len(plain))
        assert s.status == 0 and bytes(out.cpu().numpy()) == self.plain
        self.full = out
        want, self.win_off, self.win, self.row_check = sm.windows(table, plain)
        assert want["status"] == 0
        # the sizing call, one byte short, then the call: sentinels either side of win, a sentinel entry either side of the columns
        d_off = torch.full((n + 3,), -2, dtype=torch.int64, device="cuda")
        d_chk = torch.full((n + 2,), -2, dtype=torch.int32, device="cuda")
        w = dev.stream_windows_call(out, self.cols[2], self.cols[3], self.cols[4], n, d_off[1:], None, 0, d_chk[1:])
        short = {"win_bytes": want["win_bytes"], "bad_row": n, "status": 3} if want["win_bytes"] else want
        assert fields(w, W_FIELDS) == short and d_off.cpu().tolist() == [-2] + self.win_off + [-2]
        if want["win_bytes"]:
            assert d_chk.cpu().tolist() == [-2] * (n + 2)
        room = want["win_bytes"]
        buf = torch.full((GUARD + 1 + room + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        if room:
            w = dev.stream_windows_call(out, self.cols[2], self.cols[3], self.cols[4], n, d_off[1:], buf[GUARD + 1:], room - 1, d_chk[1:])
            assert fields(w, W_FIELDS) == short and bytes(buf.cpu().numpy()) == bytes([SENT]) * (2 * GUARD + 1 + room)
        w = dev.stream_windows_call(out, self.cols[2], self.cols[3], self.cols[4], n, d_off[1:], buf[GUARD + 1:], room, d_chk[1:])
        assert fields(w, W_FIELDS) == want
        b = bytes(buf.cpu().numpy())
        assert b[:GUARD + 1] == bytes([SENT]) * (GUARD + 1) and b[GUARD + 1 + room:] == bytes([SENT]) * GUARD
        assert b[GUARD + 1:GUARD + 1 + room] == self.win
        assert d_off.cpu().tolist() == [-2] + self.win_off + [-2]
        assert [v & 0xffffffff for v in d_chk.cpu().tolist()[1:-1]] == self.row_check and d_chk[0] == -2 and d_chk[-1] == -2
        self.d_win_off, self.d_win, self.d_check = d_off[1:n + 2], buf[GUARD + 1:GUARD + 1 + room], d_chk[1:n + 1]


def read_check(torch, dev, x, begins, ends, table=None, win_off=None, win=None, win_bytes=None, check=True, stream=None, cap=None,
               plain=None):
    """one hipdeflate_stream_read_ranges_dev held to the model.  table / win_off / win / stream: tampered ones in the place of
    the index's; check False: row_check NULL; cap: dst_cap (None: what the queries need) -> (the model's answer, dst)"""
    t = x.table if table is None else table
    wo = x.win_off if win_off is None else win_off
    wn = x.win if win is None else bytes(win)
    strm = x.stream if stream is None else bytes(stream)
    want = sm.read(t, x.unit, strm, x.frame, (wo, wn), x.row_check if check else None, begins, ends, cap, win_bytes, plain=plain)
    cols = x.cols if table is None else [u64(torch, t[0]), u32(torch, t[1]), u32(torch, t[2]), u64(torch, t[3]), u32(torch, t[4])]
    d_wo = x.d_win_off if win_off is None else u64(torch, wo)
    d_wn = x.d_win if win is None else to_dev(torch, wn)
    d_strm = x.d_stream if stream is None else to_dev(torch, strm)
    room = want["summary"]["out_bytes"] if cap is None else cap
    buf = torch.full((GUARD + 1 + room + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    dst_off, q_len, q_status, s = dev.stream_read_ranges_call(
        d_strm, x.frame, x.unit, *cols, d_wo, d_wn if len(wn) else None, len(wn) if win_bytes is None else win_bytes,
        x.d_check if check else None, len(t[0]), u64(torch, begins), u64(torch, ends), buf[GUARD + 1:] if room else None, room)
    assert fields(s, R_FIELDS) == want["summary"]
    b = bytes(buf.cpu().numpy())
    assert b[:GUARD + 1] == bytes([SENT]) * (GUARD + 1) and b[GUARD + 1 + room:] == bytes([SENT]) * GUARD
    dst = b[GUARD + 1:GUARD + 1 + room]
    status = want["summary"]["status"]
    if status != 1 and len(t[0]) and len(begins):
        assert dst_off.cpu().tolist() == want["dst_off"]
        assert [v & 0xffffffff for v in q_len.cpu().tolist()] == want["q_len"] and q_status.cpu().tolist() == want["q_status"]
    if status in (1, 3):                                                          # nothing is decoded
        assert dst == bytes([SENT]) * room
    else:
        for q in range(len(begins)):
            if want["exact"][q]:
                at, ln = want["dst_off"][q], want["q_len"][q]
                assert dst[at:at + ln] == want["dst"][at:at + ln], q
    return want, dst


def blocks_index(torch, dev, name, frame, row_bytes):
    key = ("blocks", name, frame, row_bytes)
    if key not in _cache:
        stream, plain = bd.stream(name, frame)
        x, *t = bd.model(stream, frame, row_bytes=row_bytes)
        assert x["status"] == 0
        _cache[key] = Index(torch, dev, stream, frame, BITS, t, plain)
    return _cache[key]


def small_index(torch, dev, row_bytes=4096):
    key = ("small", row_bytes)
    if key not in _cache:
        stream, plain = bd.small()
        x, *t = bm.index_blocks(stream, GZIP, row_bytes=row_bytes)
        _cache[key] = Index(torch, dev, stream, GZIP, BITS, t, plain)
    return _cache[key]


def carry_index(torch, dev, writer, kind, frame):
    key = ("carry", writer.__name__, kind, frame)
    if key not in _cache:
        plain = bd.data(kind, 300000)
        stream = writer(cm.cut(plain, [70000, 1, 333, 0, 0, 20000, 2, 50000]), frame)
        x, *t = cm.index_carry(stream, frame)
        assert x["status"] == 0 and 1 in t[2] and 70000 in t[2]
        _cache[key] = Index(torch, dev, stream, frame, BYTES, t, plain)
    return _cache[key]


def queries(t, rng, nrandom=40, edges=(4096, 65536)):
    """the shapes the issue names -> (begins, ends)"""
    total, n = t[3][-1] + t[2][-1], len(t[0])
    b, e = [0, 0], [total, 0]                                                    # the whole stream; nothing
    for k in sorted(set([0, 1, n // 3, n // 2, n - 2, n - 1]) & set(range(n))):
        if t[2][k]:
            o, z = t[3][k], t[2][k]
            b += [o, o + z - 1, max(o - 3, 0), o + 1]                            # its first byte, its last, across its edge, inside its first 8
            e += [o + 1, o + z, o + 3, o + min(z, 7)]
    for g in edges:
        if g + 3 < total:
            b += [g - 3]
            e += [g + 3]
    b += [5, 5, 100, 200, total // 2, 7, total - 1, total, total + 5, 10]         # duplicates, nested, unsorted; begin > end; end past
    e += [9, 9, 50000, 300, total // 2 + 70000, 3, total + 9, total + 9, total + 9, (1 << 63) + 5]      # the total; begin at and past it
    rb = rng.integers(0, total, nrandom)
    return b + [int(v) for v in rb], e + [int(v + l) for v, l in zip(rb, rng.integers(0, 20000, nrandom))]


def whole_and_ranges(torch, dev, x, nrandom=40):
    total = len(x.plain)
    want, dst = read_check(torch, dev, x, [0], [total])
    assert want["summary"]["status"] == 0 and dst == x.plain == bytes(x.full.cpu().numpy())     # the bytes of the full decode
    b, e = queries(x.table, np.random.default_rng(31), nrandom)
    want, dst = read_check(torch, dev, x, b, e)
    assert want["summary"]["status"] == 0 and want["summary"]["nrefused"] == 1
    for q in range(len(b)):                                                      # ... and every query a slice of it
        at, ln = want["dst_off"][q], want["q_len"][q]
        assert dst[at:at + ln] == (x.plain[min(b[q], total):min(e[q], total)] if b[q] <= e[q] else b""), q
    return want


# ---- the streams ------------------------------------------------------------------------------------------------------------------

BLOCK_CASES = (("text-6-m1", GZIP, 1), ("text-6-m1", ZLIB, 4096), ("text-6-m1", RAW, 65536), ("text-6-m1", GZIP, 0),
               ("fastq-1-m1", RAW, 4096), ("fastq-1-m1", ZLIB, 1), ("text-6", ZLIB, 65536), ("text-6", RAW, 0), ("fastq-9", GZIP, 65536),
               ("fastq-9", ZLIB, 0))


@pytest.mark.parametrize("name, frame, row_bytes", BLOCK_CASES)
def test_flushless_streams_through_the_block_table(torch, dev, name, frame, row_bytes):
    x = blocks_index(torch, dev, name, frame, row_bytes)
    whole_and_ranges(torch, dev, x)
    assert any(x.table[4])


@pytest.mark.parametrize("frame", (RAW, ZLIB, GZIP))
@pytest.mark.parametrize("writer, kind", ((cm.sync_writer, "text"), (cm.pigz_writer, "fastq")))
def test_flushed_streams_through_the_carry_table(torch, dev, writer, kind, frame):
    x = carry_index(torch, dev, writer, kind, frame)
    whole_and_ranges(torch, dev, x)
    if writer is cm.pigz_writer:                                                 # (zlib writes no second marker for a flush without input)
        # rows of size 0 between selected rows: never selected
        k = x.table[2].index(0, 1)
        assert x.table[2][k + 1] == 0
        want, _ = read_check(torch, dev, x, [x.table[3][k] - 2], [x.table[3][k] + 2])
        assert k not in want["selected"] and len(want["selected"]) == 2


def test_a_full_flush_stream_has_no_windows(torch, dev):
    plain = bd.data("text", 150000)
    stream = m.writer(cm.cut(plain, [20000, 333, 50000]), GZIP)[0]
    x, *t = cm.index_carry(stream, GZIP)
    assert x["status"] == 0 and not any(t[4])
    ix = Index(torch, dev, stream, GZIP, BYTES, t, plain)
    assert ix.win == b"" and ix.win_off == [0] * (len(t[0]) + 1)
    whole_and_ranges(torch, dev, ix)


@pytest.mark.parametrize("group", (4096, 65536))
def test_groups(pkg, torch, dev, group):
    x = blocks_index(torch, dev, "text-6-m1", ZLIB, 4096)
    pkg.lib().hipdeflate_test_carry_group(group)
    whole_and_ranges(torch, dev, x)
    # a read that starts in the middle: the groups are counted in selected output, so its first edge lies `group` bytes behind its start
    k = next(i for i in range(len(x.table[0]) // 2, len(x.table[0])) if x.table[3][i] & 7)
    o = x.table[3][k]
    want, dst = read_check(torch, dev, x, [o + 1, o + group - 5], [o + 3 * group, o + group + 5])
    assert want["summary"]["status"] == 0 and want["selected"][0] == k


def test_3000_random_ranges_in_one_call(torch, dev):
    x = blocks_index(torch, dev, "text-6-m1", ZLIB, 4096)
    total = len(x.plain)
    rng = np.random.default_rng(77)
    b = [int(v) for v in rng.integers(0, total, 3000)]
    e = [v + int(l) for v, l in zip(b, rng.integers(0, 3000, 3000))]
    want, dst = read_check(torch, dev, x, b, e)
    assert want["summary"]["status"] == 0 and want["summary"]["out_bytes"] == len(dst) > 3000000
    # ... and a few that leave most rows alone
    want, dst = read_check(torch, dev, x, b[:5], e[:5])
    assert 0 < want["summary"]["nselected"] <= 10


@pytest.mark.parametrize("k", range(4))
def test_carry_ring(torch, dev, k):
    """rows whose every symbol is a marker, a reach of exactly 32768, a reach of 1; matches across the ring's wraps"""
    ring = cr.cached("ring")
    picks = [c for c in ring if not c.name.startswith("ring_wrap_")] + [c for c in ring if c.name.startswith("ring_wrap_")][:4]
    seen = set()
    for c in picks[k::4]:
        frame = RAW if k & 1 else GZIP
        stream = c.compose(frame)
        x, *t = cm.index_carry(stream, frame)
        assert x["status"] == 0 and all(cr.marker_path_rows(t[2], t[4])[1:]), c.name
        ix = Index(torch, dev, stream, frame, BYTES, t, c.plain)
        b, e = queries(t, np.random.default_rng(k), 10)
        for i in range(1, len(t[0])):                                            # inside the first 8 bytes of every row that reaches back
            if t[4][i] and t[2][i] >= 3:
                b += [t[3][i] + 1, t[3][i]]
                e += [t[3][i] + min(t[2][i], 7), t[3][i] + min(t[2][i], 12)]
        want, dst = read_check(torch, dev, ix, [0] + b, [len(c.plain)] + e, plain=c.plain)
        assert want["summary"]["status"] == 0 and dst[:len(c.plain)] == c.plain, c.name
        seen |= set(t[4])
    assert {1, cr.W} <= seen, (k, sorted(seen)[:5])


# ---- only touched rows decode -----------------------------------------------------------------------------------------------------

def test_only_touched_rows_decode(torch, dev):
    x = small_index(torch, dev)
    t, total = x.table, len(x.plain)
    k = len(t[0]) // 2
    bit = t[0][k] + t[1][k] // 2
    s = bytearray(x.stream)
    s[bit >> 3] ^= 1 << (bit & 7)
    assert (t[0][k] + 7) >> 3 < bit >> 3 < (t[0][k + 1] >> 3)                    # (no bit of another row is in that byte)
    want, dst = read_check(torch, dev, x, [0, t[3][k + 1]], [t[3][k], total], stream=s)
    assert want["summary"]["status"] == 0 and want["summary"]["nselected"] == len(t[0]) - 1 and k not in want["selected"]
    assert dst == x.plain[:t[3][k]] + x.plain[t[3][k + 1]:]
    want, dst = read_check(torch, dev, x, [0, t[3][k + 1] - 1], [t[3][k], total], stream=s)
    assert (want["summary"]["status"], want["summary"]["bad_member"]) == (2, k) and want["exact"] == [True, False]
    assert dst[:t[3][k]] == x.plain[:t[3][k]]
    want, dst = read_check(torch, dev, x, [t[3][k]], [t[3][k] + 1], stream=s, check=False)
    assert want["summary"]["status"] in (0, 2) and want["summary"]["nselected"] == 1      # (without its check a flipped literal passes)


# ---- a tampered window ------------------------------------------------------------------------------------------------------------

def test_a_tampered_window(torch, dev):
    rng = np.random.default_rng(9)
    rows = [[dg.Block("stored", data=dg.rand_bytes(rng, 1000))],
            [dg.Block("static", tokens=[(5, 700)] + dg.lits(dg.rand_bytes(rng, 50)), final=True)]]
    stream, plain = cm.compose_rows(rows, RAW)
    x, *t = cm.index_carry(stream, RAW)
    assert x["status"] == 0 and t[2] == [1000, 55] and t[4] == [0, 700]
    ix = Index(torch, dev, stream, RAW, BYTES, t, plain)
    assert ix.win == plain[300:1000]
    w = bytearray(ix.win)
    w[0] ^= 0x40                                                                 # the byte 700 back from row 1: its first token's first byte
    want, dst = read_check(torch, dev, ix, [0], [1055], win=w)
    assert (want["summary"]["status"], want["summary"]["bad_member"]) == (2, 1)
    want, dst = read_check(torch, dev, ix, [0], [1055], win=w, check=False)
    assert want["summary"]["status"] == 0
    assert [i for i in range(1055) if dst[i] != plain[i]] == [1000] and dst[1000] == plain[1000] ^ 0x40
    want, dst = read_check(torch, dev, ix, [0], [1000], win=w)                    # row 1 is not touched
    assert want["summary"]["status"] == 0 and dst == plain[:1000]


# ---- tampered tables, room, arguments -----------------------------------------------------------------------------------------------

def test_tampered_tables(torch, dev):
    x = small_index(torch, dev)
    t, n, total = x.table, x.n, len(x.plain)
    assert n >= 6 and all(t[4][1:])

    def refused(at, **kw):
        want, _ = read_check(torch, dev, x, [0, 5], [total, 9], **kw)
        assert (want["summary"]["status"], want["summary"]["bad_member"]) == (1, at), kw

    def bump(col, row, by):
        u = [list(c) for c in t]
        u[col][row] += by
        return u
    refused(1, table=bump(0, 2, -1))                                             # overlaps its predecessor
    refused(0, table=bump(0, 0, -1))                                             # starts in front of the header
    refused(n - 1, table=bump(1, n - 1, 72))                                     # ends behind the payload
    refused(3, table=bump(1, 3, 1 << 31))                                        # 2^31 bits
    refused(4, table=bump(2, 4, 1))                                              # out_off is not the prefix sum of out_size
    refused(0, table=bump(3, 0, 1))
    refused(2, table=bump(4, 2, 40000))                                          # reach > 32768
    refused(1, table=bump(4, 1, t[3][1] + 1 - t[4][1]))                          # reach > out_off
    u = list(x.win_off)
    u[0] = 1
    refused(0, win_off=u)
    u = list(x.win_off)
    u[3] += 1
    refused(2, win_off=u)                                                        # win_off[i+1] - win_off[i] != reach[i]
    refused(n - 1, win_bytes=len(x.win) - 1)                                     # win_off[nrows] > win_bytes
    refused(n, stream=b"\x1f\x8c" + x.stream[2:])                                # the stream's header
    # ... and the windows call's own rules
    for tab, nbytes, at in ((bump(3, 4, 1), total, 3), (bump(2, n - 1, 1), total, n - 1), (t, total + 1, n - 1), (bump(4, 2, 40000), total, 2),
                            (bump(4, 1, t[3][1] + 1 - t[4][1]), total, 1), (bump(3, 0, 1), total, 0)):
        d_off = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
        d_chk = torch.full((n,), -2, dtype=torch.int32, device="cuda")
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        w = dev.stream_windows_call(out, u32(torch, tab[2]), u64(torch, tab[3]), u32(torch, tab[4]), n, d_off, None, 0, d_chk)
        assert fields(w, W_FIELDS) == sm.windows(tab, bytes(nbytes))[0] == {"win_bytes": 0, "bad_row": at, "status": 1}
        assert d_off.cpu().tolist() == [-2] * (n + 1) and d_chk.cpu().tolist() == [-2] * n       # nothing is written
    w = dev.stream_windows_call(torch.zeros(0, dtype=torch.uint8, device="cuda"), None, None, None, 0, None, None, 0, None)
    assert fields(w, W_FIELDS) == {"win_bytes": 0, "bad_row": 0, "status": 1}


def test_room_one_short_and_the_sizing_call(torch, dev):
    x = small_index(torch, dev)
    total = len(x.plain)
    b, e = [100, 0, 7], [20000, total, 3]
    need = 19900 + total
    want, dst = read_check(torch, dev, x, b, e, cap=need - 1)
    assert want["summary"]["status"] == 3 and want["summary"]["out_bytes"] == need and want["summary"]["nrefused"] == 1
    want, dst = read_check(torch, dev, x, b, e, cap=0)                            # dst NULL, dst_cap 0
    assert want["summary"]["status"] == 3 and want["summary"]["nselected"] == x.n
    want, dst = read_check(torch, dev, x, b, e, cap=need)
    assert want["summary"]["status"] == 0
    want, dst = read_check(torch, dev, x, [], [])                                # no queries: a zero summary
    assert want["summary"] == {"out_bytes": 0, "nselected": 0, "sel_bytes": 0, "nrefused": 0, "bad_member": x.n, "status": 0}
    want, dst = read_check(torch, dev, x, [total, 9], [total + 5, 9])             # queries, and none takes a byte
    assert want["summary"]["status"] == 0 and want["summary"]["nselected"] == 0


def test_arguments(pkg, torch, dev):
    x = small_index(torch, dev)
    args = [x.d_stream, GZIP, BITS, *x.cols, x.d_win_off, x.d_win, len(x.win), x.d_check, x.n, u64(torch, [0]), u64(torch, [10]), None, 0]
    for i, v in ((2, 2), (1, pkg.FRAME_BGZF), (0, x.d_stream[1:]), (3, None), (8, None), (14, None)):
        a = list(args)
        a[i] = v
        with pytest.raises(pkg.HipDeflateError, match="failed with 101"):
            dev.stream_read_ranges_call(*a)
    a = list(args)
    a[16] = 5                                                                    # dst NULL with dst_cap != 0
    with pytest.raises(pkg.HipDeflateError, match="failed with 101"):
        dev.stream_read_ranges_call(*a)
    assert dev.stream_read_ranges_call(*args)[3].status == 3


# ---- the layer above ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("blocks", "carry"))
def test_seek_index_class(pkg, torch, dev, kind, tmp_path):
    plain = bd.data("text", 200000)
    if kind == "blocks":
        stream = bm.plain_writer(plain, GZIP, 6, 1)
        x = dev.SeekIndex.build(to_dev(torch, stream), GZIP, kind, row_bytes=4096)
        assert x.unit == pkg.ROWS_BITS and x.nrows == bm.index_blocks(stream, GZIP, row_bytes=4096)[0]["nrows"]
    else:
        stream = cm.pigz_writer(cm.cut(plain, [30000]), GZIP)
        x = dev.SeekIndex.build(to_dev(torch, stream), GZIP, kind)
        assert x.unit == pkg.ROWS_BYTES and x.nrows >= 7
    assert x.total == len(plain) and x.win.numel() == int(x.columns["win_off"][-1]) > 0
    assert bytes(x.read(0, len(plain)).cpu().numpy()) == plain
    assert bytes(x.read(123456, 123999).cpu().numpy()) == plain[123456:123999]
    out, dst_off, q_len, q_status, s = x.read_ranges([5, 190000, 9], [10, 300000, 3])
    assert bytes(out.cpu().numpy()) == plain[5:10] + plain[190000:] and q_status.cpu().tolist() == [0, 0, 1] and s.nrefused == 1
    path = str(tmp_path / "index.npz")
    x.save(path)
    y = dev.SeekIndex.load(path, to_dev(torch, stream))
    assert (y.frame, y.unit, y.nbytes, y.nrows) == (x.frame, x.unit, len(stream), x.nrows)
    assert bytes(y.read(70000, 70100).cpu().numpy()) == plain[70000:70100]
    with pytest.raises(pkg.HipDeflateError):
        dev.SeekIndex.load(path, to_dev(torch, stream + b"x"))
    with pytest.raises(ValueError):
        x.read(9, 3)
