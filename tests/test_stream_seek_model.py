"""tests/stream_seek_model.py held to zlib, which knows nothing of rows, windows or markers: every row of every test stream is
inflated by a fresh zlib object whose dictionary is the row's window ALONE -- the reach[i] bytes the index keeps, nothing in
front of them -- and must give the row's exact bytes; every query the model answers is a slice of zlib.decompress of the whole
stream.  Then the model's own verdicts, each rule of the header once, and SeekIndex.save / load on a fake table (plain Python:
nothing touches a device).  No GPU."""
import importlib
import zlib

import numpy as np
import pytest

import blocks_dev as bd
import stream_blocks_model as bm
import stream_carry_model as cm
import stream_index_model as m
import stream_seek_model as sm
from stream_seek_model import BITS, BYTES

GZIP, ZLIB, RAW = m.FRAME_GZIP, m.FRAME_ZLIB, m.FRAME_RAW
_cache = {}


def block_case(mem, row_bytes, frame=ZLIB, n=200000):
    """a plain zlib stream of n bytes of word-shaped text -> (stream, plain, table)"""
    key = ("blocks", mem, row_bytes, frame, n)
    if key not in _cache:
        plain = bd.data("text", n)
        stream = bm.plain_writer(plain, frame, 6, mem)
        x, *t = bm.index_blocks(stream, frame, row_bytes=row_bytes)
        assert x["status"] == 0 and x["out_bytes"] == n
        _cache[key] = (stream, plain, t)
    return _cache[key]


def carry_case(writer, frame=GZIP, n=120000):
    key = ("carry", writer.__name__, frame, n)
    if key not in _cache:
        plain = bd.data("fastq", n)
        stream = writer(cm.cut(plain, [20000, 1, 333, 0, 50000]), frame)
        x, *t = cm.index_carry(stream, frame)
        assert x["status"] == 0 and x["out_bytes"] == n
        _cache[key] = (stream, plain, t)
    return _cache[key]


CASES = [("m1-4096", lambda: block_case(1, 4096), BITS, ZLIB), ("m1-1", lambda: block_case(1, 1), BITS, ZLIB),
         ("m8-65536", lambda: block_case(8, 65536), BITS, ZLIB), ("m1-4096-gzip", lambda: block_case(1, 4096, GZIP), BITS, GZIP),
         ("sync", lambda: carry_case(cm.sync_writer), BYTES, GZIP), ("pigz", lambda: carry_case(cm.pigz_writer, RAW), BYTES, RAW)]


@pytest.mark.parametrize("name, make, unit, frame", CASES, ids=[c[0] for c in CASES])
def test_every_row_inflates_from_its_window_alone(name, make, unit, frame):
    stream, plain, t = make()
    assert zlib.decompress(stream, m.WBITS[frame]) == plain
    w, win_off, win, row_check = sm.windows(t, plain)
    assert w == {"win_bytes": sum(t[4]), "bad_row": len(t[0]), "status": 0} and len(win) == w["win_bytes"] == win_off[-1]
    end = len(stream) - m.TRAILER[frame]
    for i in range(len(t[0])):
        W = win[win_off[i]:win_off[i + 1]]
        assert len(W) == t[4][i] <= min(sm.WINDOW, t[3][i]) and W == plain[t[3][i] - t[4][i]:t[3][i]]
        data = bm.row_bits(stream, t[0][i], t[1][i], end) if unit == BITS else stream[t[0][i]:t[0][i] + t[1][i]]
        d = zlib.decompressobj(-15, zdict=W) if W else zlib.decompressobj(-15)
        assert d.decompress(data) == plain[t[3][i]:t[3][i] + t[2][i]], (name, i)
        assert row_check[i] == zlib.crc32(plain[t[3][i]:t[3][i] + t[2][i]])
        if t[4][i] > 1:                                          # ... and from no less: a byte short, zlib refuses the row
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15, zdict=W[1:]).decompress(data)


def test_what_the_windows_cost():
    """32 KiB a row at the most: row_bytes decides"""
    for mem, row_bytes, lo, hi in ((1, 4096, 4.0, 8.0), (8, 65536, 0.0, 0.5), (1, 0, 0.0, 0.25)):
        stream, plain, t = block_case(mem, row_bytes)
        ratio = sum(t[4]) / len(plain)
        assert max(t[4]) <= sm.WINDOW and lo <= ratio <= hi, (mem, row_bytes, ratio)


def queries(t, rng, nrandom=200):
    total, n = t[3][-1] + t[2][-1], len(t[0])
    k = n // 2
    b = [0, 0, t[3][k], t[3][k] + t[2][k] - 1, max(t[3][k] - 3, 0), 5, 5, 100, total - 1, total, 7, total + 5, 10]
    e = [total, 0, t[3][k] + 1, t[3][k] + t[2][k], t[3][k] + 3, 9, 9, 50000, total + 9, total + 9, 3, total + 9, (1 << 63) + 5]
    rb = rng.integers(0, total, nrandom)
    return b + [int(v) for v in rb], e + [int(v + l) for v, l in zip(rb, rng.integers(0, 9000, nrandom))]


@pytest.mark.parametrize("name, make, unit, frame", CASES, ids=[c[0] for c in CASES])
def test_every_query_is_a_slice_of_the_whole(name, make, unit, frame):
    stream, plain, t = make()
    _, win_off, win, row_check = sm.windows(t, plain)
    b, e = queries(t, np.random.default_rng(5))
    r = sm.read(t, unit, stream, frame, (win_off, win), row_check, b, e)
    s = r["summary"]
    assert s["status"] == 0 and s["bad_member"] == len(t[0]) and s["nrefused"] == 1 and r["q_status"][10] == 1
    at = 0
    for q in range(len(b)):
        lo, hi = min(b[q], len(plain)), min(e[q], len(plain))
        want = plain[lo:hi] if b[q] <= e[q] else b""
        assert r["dst_off"][q] == at and r["q_len"][q] == len(want) and r["dst"][at:at + len(want)] == want, (name, q)
        at += len(want)
    assert s["out_bytes"] == at == len(r["dst"])
    touched = [i for i in range(len(t[0])) if t[2][i] and any(max(b[q], t[3][i]) < min(e[q], t[3][i] + t[2][i]) for q in range(len(b)) if b[q] <= e[q])]
    assert r["selected"] == touched and s["nselected"] == len(touched) and s["sel_bytes"] == sum(t[2][i] for i in touched)
    # one byte of one row: that row alone
    k = min(3, len(t[0]) - 1)
    one = sm.read(t, unit, stream, frame, (win_off, win), row_check, [t[3][k]], [t[3][k] + 1])
    assert one["selected"] == [k if t[2][k] else k + 1] and one["dst"] == plain[t[3][k]:t[3][k] + 1]


def test_verdicts_in_the_headers_order():
    stream, plain, t = block_case(1, 4096, GZIP)
    n, total = len(t[0]), len(plain)
    _, win_off, win, row_check = sm.windows(t, plain)

    def status(table=t, wo=win_off, rc=row_check, b=(0,), e=(total,), strm=stream, **kw):
        r = sm.read(table, BITS, strm, GZIP, (wo, win), rc, list(b), list(e), **kw)
        return r["summary"]["status"], r["summary"]["bad_member"]

    def bump(col, row, by):
        u = [list(c) for c in t]
        u[col][row] += by
        return u
    assert status() == (0, n)
    assert status(bump(0, 2, -1)) == (1, 1) and status(bump(0, 0, -1)) == (1, 0)        # overlaps its predecessor's end; in front of the header
    assert status(bump(1, n - 1, 8 * 9)) == (1, n - 1)                                   # ends behind the payload
    assert status(bump(2, 5, 1)) == (1, 5) and status(bump(3, 0, 1))[0] == 1             # the prefix sum
    assert status(bump(4, 0, 1)) == (1, 0) and status(bump(4, 7, 40000)) == (1, 7)       # the reach rule
    assert status(strm=b"\x1f\x8c" + stream[2:]) == (1, n)                               # the header
    u = list(win_off)
    u[0] = 1
    assert status(wo=u) == (1, 0)
    u = list(win_off)
    u[4] += 1
    assert status(wo=u) == (1, 3)
    assert status(win_bytes=len(win) - 1) == (1, n - 1) and status(win_bytes=win_off[6] - 1) == (1, 5)
    # status 3 in front of status 2; the sizing call
    bad = list(row_check)
    bad[2] ^= 1
    assert status(rc=bad, dst_cap=total - 1) == (3, n) and status(dst_cap=0) == (3, n)
    assert status(rc=bad) == (2, 2) and status(rc=bad, b=(t[3][3],), e=(total,)) == (0, n)
    # a window byte: with the rows' checks a verdict, without them a wrong byte
    k = next(i for i in range(1, n) if t[4][i] > 0)
    w2 = bytearray(win)
    w2[win_off[k]] ^= 0x55                                    # the furthest byte the row names: one it does name
    r = sm.read(t, BITS, stream, GZIP, (win_off, bytes(w2)), row_check, [0], [total])
    assert (r["summary"]["status"], r["summary"]["bad_member"]) == (2, k) and r["exact"] == [False]
    r = sm.read(t, BITS, stream, GZIP, (win_off, bytes(w2)), row_check, [0, t[3][k + 1]], [t[3][k], total])
    assert r["summary"]["status"] == 0 and r["dst"] == plain[:t[3][k]] + plain[t[3][k + 1]:]
    # a flipped stream bit inside row 6: only a query that touches the row sees it
    s2 = bytearray(stream)
    s2[(t[0][6] + 40) >> 3] ^= 1 << ((t[0][6] + 40) & 7)
    assert status(strm=bytes(s2), b=(0,), e=(t[3][6],)) == (0, n)
    assert status(strm=bytes(s2), b=(t[3][6] + t[2][6] - 1,), e=(total,)) == (2, 6)
    assert status(table=[[], [], [], [], []], wo=[0], rc=[]) == (0, 0) and status(b=(), e=()) == (0, n)
    # the windows call's own refusals
    assert sm.windows(t, plain + b"x")[0] == {"win_bytes": 0, "bad_row": n - 1, "status": 1}
    assert sm.windows(bump(3, 4, 1), plain)[0]["bad_row"] == 3 and sm.windows(bump(4, 9, 40000), plain)[0]["bad_row"] == 9
    assert sm.windows([[], [], [], [], []], b"")[0] == {"win_bytes": 0, "bad_row": 0, "status": 1}
    w3 = sm.windows(t, plain, win_cap=len(win) - 1)
    assert w3[0] == {"win_bytes": len(win), "bad_row": n, "status": 3} and w3[1] == win_off and w3[2] is None and w3[3] is None


def test_seek_index_save_and_load(tmp_path):
    dev = importlib.import_module("7bgzf_amd.device")
    pkg = importlib.import_module("7bgzf_amd")
    n = 5
    cols = {"in_off": np.array([80, 900, 5000, 5000, 70000], dtype=np.uint64).view(np.int64),
            "in_len": np.array([820, 4100, 0, 65000, 0xfffffff0], dtype=np.uint32).view(np.int32),
            "out_size": np.array([100, 300, 0, 70000, 1], dtype=np.int32), "out_off": np.array([0, 100, 400, 400, 70400], dtype=np.int64),
            "reach": np.array([0, 100, 0, 400, 32768], dtype=np.int32), "win_off": np.array([0, 0, 100, 100, 500, 33268], dtype=np.int64),
            "row_check": np.array([1, 0xffffffff, 0, 0x80000000, 5], dtype=np.uint32).view(np.int32)}
    win = np.random.default_rng(1).integers(0, 256, 33268, dtype=np.uint8)
    stream = bytes(12345)
    x = dev.SeekIndex(None, pkg.FRAME_ZLIB, pkg.ROWS_BITS, len(stream), cols, win)
    assert x.nrows == n and x.total == 70401
    path = str(tmp_path / "x.seek.npz")
    x.save(path)
    y = dev.SeekIndex.load(path, stream)
    assert (y.frame, y.unit, y.nbytes, y.nrows, y.stream) == (pkg.FRAME_ZLIB, pkg.ROWS_BITS, 12345, n, None)
    for c in dev.SeekIndex.COLUMNS:
        assert y.columns[c].dtype == cols[c].dtype and np.array_equal(y.columns[c], cols[c]), c
    assert y.win.dtype == np.uint8 and np.array_equal(y.win, win)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(("version", "frame", "unit", "nbytes", "win") + dev.SeekIndex.COLUMNS) and int(z["version"]) == 1
    with pytest.raises(pkg.HipDeflateError, match="12345 bytes"):
        dev.SeekIndex.load(path, stream + b"x")
    with pytest.raises(pkg.HipDeflateError, match="loaded without its stream"):
        y.read(0, 1)
    with np.load(path) as z:
        parts = {k: z[k] for k in z.files}
    parts["version"] = np.int64(2)
    other = str(tmp_path / "v2.npz")
    with open(other, "wb") as f:
        np.savez(f, **parts)
    with pytest.raises(pkg.HipDeflateError, match="version 2"):
        dev.SeekIndex.load(other, stream)
    with pytest.raises(ValueError):
        dev.SeekIndex(None, pkg.FRAME_ZLIB, pkg.ROWS_BITS, 1, dict(cols, reach=cols["reach"][:4]), win)
