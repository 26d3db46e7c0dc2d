#!/usr/bin/env python3
"""What the block index and the block decode cost: hipdeflate_stream_index_blocks_dev and hipdeflate_stream_inflate_blocks_dev
on plain streams, which have no flush point, beside (a) the path such a stream took before -- hipdeflate_stream_index_dev and
hipdeflate_stream_inflate_table_dev, one row, one wavefront -- (b) hipdeflate_stream_inflate_carry_dev on the sync-flush stream
of the same data at 128 KiB pieces, the yardstick this path cannot beat, and (c) one zlib.decompress on the CPU.

Data: the bench's two kinds (7bgzf_amd/synth.py), 16 MiB of each repeated to --mib.  Streams: zlib levels 1 and 6, one
compressor, no flush, gzip frame.

Per stream: candidates per GiB of stream, the share of them whose piece gets past its own first block header and the share
whose piece decodes to its stop (hipdeflate_test_blocks_counts), the pieces of the chain; the index's passes by events
(hipdeflate_test_blocks_times: candidates, pieces, chain, merge) with max_chunk_in 0 and with HD_BLOCK_PIECE_IN, which is what
the convenience calls index with first; the decode's four (hipdeflate_test_carry_times); the whole calls.  Times are the best
of --reps calls behind one warm-up.  Writes --out (default profiles/stream_blocks_timing.txt)."""
import argparse
import ctypes
import importlib
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from stream_carry_bench import best, one_compressor          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-one-row", action="store_true", help="leave (a) out: one wavefront over the whole stream takes seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_blocks_timing.txt"))
    a = ap.parse_args()
    torch = importlib.import_module("torch")
    import numpy as np
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    assert pkg.available(), "no usable MI355X"
    lib = pkg.lib()
    lines = ["stream_blocks_bench: %d MiB per stream, best of %d, ms (GB/s of output)" % (a.mib, a.reps), ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def to_dev(blob):
        return torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()[:len(blob)]

    def rate(ms, n):
        return "%9.2f (%6.2f)" % (ms, n / ms / 1e6)

    G = pkg.FRAME_GZIP
    ms4, ix4 = (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
    for kind, gen in (("text", synth.text_like), ("fastq", synth.fastq_like)):
        tile = bytes(gen(16 << 20))
        data = (tile * ((a.mib + 15) // 16))[:a.mib << 20]
        n = len(data)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        for level in (1, 6):
            c = zlib.compressobj(level, zlib.DEFLATED, 31)
            stream = c.compress(data) + c.flush()
            t0 = time.perf_counter()
            assert zlib.decompress(stream, 31) == data
            t_cpu = (time.perf_counter() - t0) * 1e3
            d = to_dev(stream)
            say("%s, level %d: plain stream %d bytes   (c) zlib on the CPU %s" % (kind, level, len(stream), rate(t_cpu, n)))
            B = pkg.BLOCK_PIECE_IN
            t_idx, r = best(a.reps, lambda: dev.index_stream_blocks(d, G, max_chunk_in=B))
            in_off, in_len, out_size, out_off, reach, x = r
            assert x.status == 0 and x.out_bytes == n, (x.status, x.out_bytes)
            t_idx0, r0 = best(1, lambda: dev.index_stream_blocks(d, G))
            assert r0[5].status == 0 and r0[5].nrows == x.nrows
            call = lambda: dev.inflate_stream_blocks_call(d, G, in_off, in_len, out_size, out_off, reach, x.nrows, out, n)
            t_dec, s = best(a.reps, call)
            assert s.status == 0 and s.check == zlib.crc32(data)
            ix0, cnt = (ctypes.c_double * 4)(), (ctypes.c_uint64 * 2)()
            lib.hipdeflate_test_blocks_times(ix4)             # on
            dev.index_stream_blocks_call(d, G, x.nrows, 0, 0, in_off, in_len, out_size, out_off, reach)
            lib.hipdeflate_test_blocks_times(ix0)
            lib.hipdeflate_test_blocks_counts(cnt)
            dev.index_stream_blocks_call(d, G, x.nrows, B, 0, in_off, in_len, out_size, out_off, reach)
            lib.hipdeflate_test_blocks_times(ix4)
            lib.hipdeflate_test_blocks_times(None)            # off
            lib.hipdeflate_test_carry_times(ms4)
            call()
            lib.hipdeflate_test_carry_times(ms4)
            lib.hipdeflate_test_carry_times(None)
            say("  blocks  %d candidates (%.2f M per GiB of stream), %d (%.2f %%) past their first header, %d (%.2f %%) decode to their stop; "
                "%d pieces, %d rows" % (x.ncandidates, x.ncandidates / len(stream) * 1024, cnt[0], 100.0 * cnt[0] / x.ncandidates, cnt[1],
                                        100.0 * cnt[1] / x.ncandidates, x.npieces, x.nrows))
            say("          index, max_chunk_in 0      %s   candidates %8.2f  pieces %8.2f  chain %8.2f  merge %8.2f"
                % (rate(t_idx0, n), ix0[0], ix0[1], ix0[2], ix0[3]))
            say("          index, max_chunk_in %d %s   candidates %8.2f  pieces %8.2f  chain %8.2f  merge %8.2f"
                % (B, rate(t_idx, n), ix4[0], ix4[1], ix4[2], ix4[3]))
            say("          decode %s   decode %8.2f  tails %8.2f  resolve %8.2f  check %8.2f   index + decode %s"
                % (rate(t_dec, n), ms4[0], ms4[1], ms4[2], ms4[3], rate(t_idx + t_dec, n)))
            if not a.skip_one_row:
                t_i1, r1 = best(1, lambda: dev.index_stream(d, G))
                assert r1[4].status == 0 and r1[4].nchunks == 1
                t_d1, s1 = best(1, lambda: dev.inflate_stream_table_call(d, G, r1[0], r1[1], r1[2], r1[3], 1, out, n))
                assert s1.status == 0
                say("  (a) one row   index %s   table decode %s   both %s" % (rate(t_i1, n), rate(t_d1, n), rate(t_i1 + t_d1, n)))
            del d
            sync = to_dev(one_compressor(data, 128 << 10, level))
            t_ci, rc = best(a.reps, lambda: dev.index_stream_carry(sync, G))
            assert rc[5].status == 0
            t_cd, sc = best(a.reps, lambda: dev.inflate_stream_carry_call(sync, G, rc[0], rc[1], rc[2], rc[3], rc[4], rc[5].nchunks, out, n))
            assert sc.status == 0
            say("  (b) sync-flush stream, 128 KiB pieces   carry index %s   carry decode %s   both %s"
                % (rate(t_ci, n), rate(t_cd, n), rate(t_ci + t_cd, n)))
            del sync
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
