#!/usr/bin/env python3
"""What the seek index costs and buys: hipdeflate_stream_windows_dev and hipdeflate_stream_read_ranges_dev on one gzip stream
resident in HBM, beside the full decode on the same table -- hipdeflate_stream_inflate_blocks_dev /
hipdeflate_stream_inflate_carry_dev, unchanged code, in the same run: the yardstick.

Data: the bench's two kinds (7bgzf_amd/synth.py), 16 MiB of each repeated to --mib.  Streams in a gzip frame: zlib level 6,
one compressor, no flush (the block table at its default rows), and pigz's form at 128 KiB pieces (the carry table).

Per stream:
  (a) the windows call, and win_bytes / out_bytes;
  (b) a read of [0, total) against the full decode, the two calls ALTERNATED, the best of --reps of each behind a warm-up;
  (c) reads of 1, 64 and 4,096 random 64 KiB ranges: time, nselected, the ratio to (b);
  (d) a read that touches one row: one byte in the middle of a row.
Times are a host clock around calls that end in a synchronise of the stream.  Never run under a counter collection.
Writes --out (default profiles/stream_seek_timing.txt)."""
import argparse
import concurrent.futures
import importlib
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from stream_carry_bench import best, piecewise          # noqa: E402


def alternated(reps, f, g):
    """the best of reps calls of each, f and g taking turns behind one warm-up of both -> (ms of f, ms of g, f's answer, g's)"""
    rf, rg = f(), g()
    tf, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rf = f()
        t1 = time.perf_counter()
        rg = g()
        t2 = time.perf_counter()
        tf.append(t1 - t0)
        tg.append(t2 - t1)
    return min(tf) * 1e3, min(tg) * 1e3, rf, rg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_seek_timing.txt"))
    a = ap.parse_args()
    torch = importlib.import_module("torch")
    import numpy as np
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    assert pkg.available(), "no usable MI355X"
    lines = ["stream_seek_bench: %d MiB per stream, gzip frame, best of %d behind a warm-up, ms (GB/s of the bytes read)" % (a.mib, a.reps), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def to_dev(blob):
        return torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]

    def rate(ms, n):
        return "%9.3f (%6.2f)" % (ms, n / ms / 1e6)

    G = pkg.FRAME_GZIP
    rng = np.random.default_rng(2031)
    pool = concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1))
    for kind, gen in (("text", synth.text_like), ("fastq", synth.fastq_like)):
        tile = bytes(gen(16 << 20))
        data = (tile * ((a.mib + 15) // 16))[:a.mib << 20]
        n = len(data)
        crc = zlib.crc32(data)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        for form in ("plain", "pigz"):
            if form == "plain":
                c = zlib.compressobj(6, zlib.DEFLATED, 31)
                stream = c.compress(data) + c.flush()
                d = to_dev(stream)
                in_off, in_len, out_size, out_off, reach, x = dev.index_stream_blocks(d, G, max_chunk_in=pkg.BLOCK_PIECE_IN)
                nrows, unit, decode, what = x.nrows, pkg.ROWS_BITS, dev.inflate_stream_blocks_call, "zlib level 6, no flush: the block table, default rows"
            else:
                stream = piecewise(pool, data, 128 << 10, 6, zlib.Z_SYNC_FLUSH)
                d = to_dev(stream)
                in_off, in_len, out_size, out_off, reach, x = dev.index_stream_carry(d, G)
                nrows, unit, decode, what = x.nchunks, pkg.ROWS_BYTES, dev.inflate_stream_carry_call, "pigz form, 128 KiB pieces, level 6: the carry table"
            assert x.status == 0 and x.out_bytes == n, (x.status, x.out_bytes)
            cols = [t[:nrows].contiguous() for t in (in_off, in_len, out_size, out_off, reach)]
            full = lambda: decode(d, G, *cols, nrows, out, n)
            s = full()
            assert s.status == 0 and s.check == crc
            say("%s, %s: %d bytes of stream, %d rows" % (kind, what, len(stream), nrows))
            # (a) the windows
            win_off = torch.zeros(nrows + 1, dtype=torch.int64, device="cuda")
            row_check = torch.zeros(nrows, dtype=torch.int32, device="cuda")
            w = dev.stream_windows_call(out, cols[2], cols[3], cols[4], nrows, win_off, None, 0, row_check)
            assert w.status in (0, 3)
            win = torch.empty(w.win_bytes, dtype=torch.uint8, device="cuda")
            t_win, w = best(a.reps, lambda: dev.stream_windows_call(out, cols[2], cols[3], cols[4], nrows, win_off, win, win.numel(), row_check))
            assert w.status == 0
            say("  (a) windows call %s   win_bytes %d = %.4f of out_bytes" % (rate(t_win, n), w.win_bytes, w.win_bytes / n))

            def read(begins, ends, dst, check=True):
                return dev.stream_read_ranges_call(d, G, unit, *cols, win_off, win, win.numel(), row_check if check else None, nrows, begins,
                                                   ends, dst, dst.numel())

            # (b) the whole stream, against the yardstick, alternated
            dst = torch.empty(n, dtype=torch.uint8, device="cuda")
            b0, e0 = dev._u64_tensor([0], "cuda"), dev._u64_tensor([n], "cuda")
            t_full, t_read, s, r = alternated(a.reps, full, lambda: read(b0, e0, dst))
            assert s.status == 0 and r[3].status == 0 and r[3].out_bytes == n and torch.equal(dst, out)
            t_full2, t_nock, _, r = alternated(a.reps, full, lambda: read(b0, e0, dst, check=False))
            assert r[3].status == 0
            say("  (b) full decode (the yardstick) %s   read of [0, total) %s   ratio %.3f   without row_check %s   ratio %.3f"
                % (rate(t_full, n), rate(t_read, n), t_read / t_full, rate(t_nock, n), t_nock / t_full2))
            # (c) random 64 KiB ranges
            for nq in (1, 64, 4096):
                b = rng.integers(0, n - (64 << 10), nq)
                begins, ends = dev._u64_tensor([int(v) for v in b], "cuda"), dev._u64_tensor([int(v) + (64 << 10) for v in b], "cuda")
                dq = torch.empty(nq * (64 << 10), dtype=torch.uint8, device="cuda")
                t_q, r = best(a.reps, lambda: read(begins, ends, dq))
                assert r[3].status == 0 and r[3].out_bytes == dq.numel()
                k = int(b[0])
                assert torch.equal(dq[:64 << 10], out[k:k + (64 << 10)])
                say("  (c) %4d random 64 KiB ranges %s   nselected %d (%d bytes decoded)   %.4f of (b)"
                    % (nq, rate(t_q, dq.numel()), r[3].nselected, r[3].sel_bytes, t_q / t_read))
            # (d) one row: one byte in the middle of the stream's middle row
            k = nrows // 2
            at = int(cols[3][k]) + (int(cols[2][k]) & 0xffffffff) // 2
            d1 = torch.empty(1, dtype=torch.uint8, device="cuda")
            b1, e1 = dev._u64_tensor([at], "cuda"), dev._u64_tensor([at + 1], "cuda")
            torch.cuda.synchronize()
            t_1, r = best(max(a.reps, 10), lambda: read(b1, e1, d1))
            assert r[3].status == 0 and r[3].nselected == 1 and int(d1[0]) == data[at]
            say("  (d) one byte, one row of %d bytes (row_bytes %s) %9.3f ms"
                % (r[3].sel_bytes, "the default, 128 KiB" if form == "plain" else "the writer's 128 KiB", t_1))
            del d, win, dst
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
