#!/usr/bin/env python3
"""What the carry decode costs: hipdeflate_stream_index_carry_dev and hipdeflate_stream_inflate_carry_dev on streams whose
flushes carry the window, beside the full-flush decode of the same data and pieces (hipdeflate_stream_inflate_table_dev,
the yardstick) and one zlib.decompress on the CPU.

Data: the bench's two kinds (7bgzf_amd/synth.py), 16 MiB of each repeated to --mib (the period is 512 windows: no match
sees it).  Streams, raw DEFLATE in a gzip frame: pigz's form (every piece by a fresh compressor primed with the 32 KiB in
front of it, Z_SYNC_FLUSH; a pool of at most 16 threads, zlib releases the GIL), one compressor with Z_SYNC_FLUSH, and --
independent pieces -- Z_FULL_FLUSH.  Pieces of 128 KiB and 16 KiB, levels 1 and 6.

Per stream: the carry index, the marker path's passes by events (hipdeflate_test_carry_times: decode, tails, resolve,
check + fold), the whole carry decode; on the full-flush stream the table decode and the carry decode (its fast path).
Times are the best of --reps calls behind one warm-up.  Writes --out (default profiles/stream_carry_timing.txt)."""
import argparse
import concurrent.futures
import ctypes
import importlib
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 32768
GZ_HEADER = bytes.fromhex("1f8b08000000000000ff")


def gz_trailer(plain):
    return zlib.crc32(plain).to_bytes(4, "little") + (len(plain) & 0xffffffff).to_bytes(4, "little")


def code_piece(args):
    data, lo, hi, level, last, flush = args
    prime = data[max(0, lo - WINDOW):lo] if flush == zlib.Z_SYNC_FLUSH else b""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=prime) if prime else zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data[lo:hi]) + (c.flush() if last else c.flush(flush))


def piecewise(pool, data, piece, level, flush):
    """pigz's form (flush = Z_SYNC_FLUSH: primed pieces) or independent pieces (Z_FULL_FLUSH), coded side by side"""
    cuts = list(range(0, len(data), piece))
    jobs = [(data, lo, min(lo + piece, len(data)), level, lo == cuts[-1], flush) for lo in cuts]
    return GZ_HEADER + b"".join(pool.map(code_piece, jobs)) + gz_trailer(data)


def one_compressor(data, piece, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    out = []
    for lo in range(0, len(data), piece):
        out.append(c.compress(data[lo:lo + piece]))
        out.append(c.flush(zlib.Z_SYNC_FLUSH) if lo + piece < len(data) else c.flush())
    return b"".join(out)


def best(reps, f):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        t.append(time.perf_counter() - t0)
    return min(t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_carry_timing.txt"))
    a = ap.parse_args()
    torch = importlib.import_module("torch")
    import numpy as np
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    assert pkg.available(), "no usable MI355X"
    lib = pkg.lib()
    lines = ["stream_carry_bench: %d MiB per stream, best of %d, ms (GB/s of output)" % (a.mib, a.reps), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def to_dev(blob):
        return torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]

    def rate(ms, n):
        return "%9.2f (%6.2f)" % (ms, n / ms / 1e6)

    pool = concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
    ms4 = (ctypes.c_double * 4)()
    for kind, gen in (("text", synth.text_like), ("fastq", synth.fastq_like)):
        tile = bytes(gen(16 << 20))
        data = (tile * ((a.mib + 15) // 16))[:a.mib << 20]
        n = len(data)
        for piece in (128 << 10, 16 << 10):
            for level in (1, 6):
                full = piecewise(pool, data, piece, level, zlib.Z_FULL_FLUSH)
                streams = (("pigz", piecewise(pool, data, piece, level, zlib.Z_SYNC_FLUSH)), ("sync", one_compressor(data, piece, level)))
                say("%s, pieces of %d KiB, level %d: full-flush stream %d bytes" % (kind, piece >> 10, level, len(full)))
                d_full = to_dev(full)
                t_idx, r = best(a.reps, lambda: dev.index_stream(d_full, pkg.FRAME_GZIP))
                in_off, in_len, out_size, out_off, x = r
                assert x.status == 0 and x.out_bytes == n
                out = torch.empty(n, dtype=torch.uint8, device="cuda")
                t_tab, s = best(a.reps, lambda: dev.inflate_stream_table_call(d_full, pkg.FRAME_GZIP, in_off, in_len, out_size, out_off,
                                                                                x.nchunks, out, n))
                assert s.status == 0
                zero = torch.zeros(x.nchunks, dtype=torch.int32, device="cuda")
                t_fast, s = best(a.reps, lambda: dev.inflate_stream_carry_call(d_full, pkg.FRAME_GZIP, in_off, in_len, out_size, out_off,
                                                                                 zero, x.nchunks, out, n))
                assert s.status == 0
                say("  full-flush   index %s   table decode (yardstick) %s   carry decode, fast path %s"
                    % (rate(t_idx, n), rate(t_tab, n), rate(t_fast, n)))
                del d_full
                for name, stream in streams:
                    t0 = time.perf_counter()
                    assert zlib.decompress(stream, 31) == data
                    t_cpu = (time.perf_counter() - t0) * 1e3
                    d = to_dev(stream)
                    t_idx, r = best(a.reps, lambda: dev.index_stream_carry(d, pkg.FRAME_GZIP))
                    in_off, in_len, out_size, out_off, reach, x = r
                    assert x.status == 0 and x.out_bytes == n, (x.status, x.out_bytes)
                    call = lambda: dev.inflate_stream_carry_call(d, pkg.FRAME_GZIP, in_off, in_len, out_size, out_off, reach, x.nchunks,
                                                                 out, n)
                    t_all, s = best(a.reps, call)
                    assert s.status == 0 and s.check == zlib.crc32(data)
                    lib.hipdeflate_test_carry_times(ms4)          # on
                    call()
                    lib.hipdeflate_test_carry_times(ms4)
                    lib.hipdeflate_test_carry_times(None)         # off
                    say("  %-4s %9d bytes, %6d rows   carry index %s   decode %8.2f  tails %8.2f  resolve %8.2f  check %8.2f   whole call %s"
                        "   zlib on the CPU %s" % (name, len(stream), x.nchunks, rate(t_idx, n), ms4[0], ms4[1], ms4[2], ms4[3],
                                                   rate(t_all, n), rate(t_cpu, n)))
                    del d
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
