#!/usr/bin/env python3
"""Time of decoding ONE gzip stream in parallel without its chunk table, next to the decode that has the table.

--gib GiB of the text set and of the FASTQ-like set (a seeded 64 MiB tile replicated; no chunk sees the repetition) are
coded by hipdeflate_stream_deflate_dev, HD_FRAME_GZIP, at level 1 and level 6 in chunks of 64 KiB and 1 MiB; the stream
stays in HBM.  After a warm-up, --reps repetitions of
    (a) hipdeflate_stream_index_dev                               the scan, one piece decode per candidate, the chain, the tables
    (b) (a), then hipdeflate_stream_inflate_table_dev on its table    what a caller without a table pays
    (c) hipdeflate_stream_inflate_dev with the encoder's own table    unchanged code: the yardstick
are timed with device events; the medians and (b)/(c) are reported, with (a)'s candidates, and how many of them are false, per
GiB of stream.  The index's table is held to the encoder's and (b)'s output to the input before anything is timed.  One
process; every GPU step runs under its own time limit (the process exits when one runs out) and the first failure ends the
run.  The figures go to --out (profiles/stream_index_timing.txt) and, as one JSON line, to stdout.  No bar is set: the size
pass costs 0.51-0.59 of an inflate (profiles/framed_inflate_timing.txt), so (b)/(c) is expected near 1.5-1.6.

    python tools/stream_index_bench.py [--gib 1] [--reps 3] [--out profiles/stream_index_timing.txt]
"""
import argparse
import faulthandler
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Step:
    """a GPU step under its own time limit: the watchdog thread ends the process if the step has not returned"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        print("step: %s (limit %d s)" % (self.name, self.seconds), file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def measure(gib=1.0, reps=3, tile_mib=64):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    L = pkg.lib()
    tile_bytes = tile_mib << 20
    frame = pkg.FRAME_GZIP

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def median(v):
        return sorted(v)[len(v) // 2]

    rows = []
    tiles = {"text": lambda: synth.text_like(tile_bytes, seed=4321), "fastq": lambda: synth.fastq_like(tile_bytes, seed=1234)}
    for name, make in tiles.items():
        with Step("%s: input" % name, 300):
            tile = torch.from_numpy(make()).cuda()
            data = tile.repeat(max(1, int(gib * (1 << 30)) // tile_bytes))
            total = data.numel()
            torch.cuda.synchronize()
        for level in (1, 6):
            for chunk in (64 << 10, 1 << 20):
                nchunks = (total + chunk - 1) // chunk
                with Step("%s level %d chunk %d: encode" % (name, level, chunk), 300):
                    bound = int(L.hipdeflate_stream_bound(total, chunk, level, frame))
                    dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
                    tab = torch.zeros(nchunks + 1, dtype=torch.int64, device="cuda")
                    s = dev.deflate_stream_call(data, level, frame, chunk, dst, bound, tab)
                    assert (s.status, s.in_bytes, s.nchunks) == (0, total, nchunks), (s.status, s.in_bytes, s.nchunks)
                    stream = dst[:s.out_bytes]
                back = torch.empty(total, dtype=torch.uint8, device="cuda")
                with Step("%s level %d chunk %d: index" % (name, level, chunk), 300):
                    # (the sizing pass, the warm-up and the check.  A row is a piece between two flush points: a chunk, or --
                    # levels 1..2, chunks longer than HD_SEG_LIMIT -- one of the full-flush segments the encoder codes it in)
                    in_off, in_len, out_size, out_off, x = dev.index_stream(stream, frame)
                    n = int(x.nchunks)
                    assert (x.status, x.out_bytes, x.end_offset) == (0, total, s.out_bytes), (x.status, x.nchunks, x.out_bytes, x.end_offset)
                    assert n >= nchunks + 1 and bool(torch.isin(tab, in_off[:n]).all())
                    in_off, in_len, out_size, out_off = in_off[:n].clone(), in_len[:n].clone(), out_size[:n].clone(), out_off[:n].clone()

                def index():
                    return dev.index_stream_call(stream, frame, n, 0, in_off, in_len, out_size, out_off)

                def index_and_decode():
                    x = index()
                    return dev.inflate_stream_table_call(stream, frame, in_off, in_len, out_size, out_off, x.nchunks, back, total)

                def with_table():
                    return dev.inflate_stream_call(stream, frame, tab, nchunks, chunk, total, back, total)

                with Step("%s level %d chunk %d: index, timed" % (name, level, chunk), 300):
                    a_ms = [timed(index)[0] for _ in range(reps)]
                with Step("%s level %d chunk %d: index and decode" % (name, level, chunk), 300):
                    back.zero_()
                    d = index_and_decode()
                    assert (d.status, d.check, d.out_bytes) == (0, s.check, total), (d.status, d.bad_chunk)
                    assert torch.equal(back, data)
                    b_ms = [timed(index_and_decode)[0] for _ in range(reps)]
                with Step("%s level %d chunk %d: decode with the encoder's table" % (name, level, chunk), 300):
                    back.zero_()
                    d = with_table()
                    assert (d.status, d.check) == (0, s.check), (d.status, d.bad_chunk)
                    assert torch.equal(back, data)
                    c_ms = [timed(with_table)[0] for _ in range(reps)]
                a, b, c = median(a_ms), median(b_ms), median(c_ms)
                per_gib = (1 << 30) / s.out_bytes
                rows.append({
                    "set": name, "level": level, "chunk": chunk, "bytes": total, "stream_bytes": int(s.out_bytes), "chunks": nchunks, "nchunks": n,
                    "ncandidates": int(x.ncandidates), "false_candidates": int(x.ncandidates) - n,
                    "candidates_per_GiB_of_stream": round(x.ncandidates * per_gib, 1),
                    "false_candidates_per_GiB_of_stream": round((x.ncandidates - n) * per_gib, 2),
                    "index_ms": [round(v, 3) for v in a_ms], "index_decode_ms": [round(v, 3) for v in b_ms],
                    "table_decode_ms": [round(v, 3) for v in c_ms],
                    "index_GBps": round(total / a / 1e6, 2), "index_decode_GBps": round(total / b / 1e6, 2),
                    "table_decode_GBps": round(total / c / 1e6, 2),
                    "index_over_table_decode": round(a / c, 4), "index_decode_over_table_decode": round(b / c, 4),
                })
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                del dst, tab, stream, back, in_off, in_len, out_size, out_off
                torch.cuda.empty_cache()
        del data, tile
        torch.cuda.empty_cache()
    assert L.hipdeflate_stall_count() == 0
    ratios = [r["index_decode_over_table_decode"] for r in rows]
    return {"rows": rows, "ratio_min": min(ratios), "ratio_max": max(ratios)}


def report(res):
    lines = ["stream index timing -- tools/stream_index_bench.py",
             "(a) hipdeflate_stream_index_dev | (b) (a) + hipdeflate_stream_inflate_table_dev | (c) hipdeflate_stream_inflate_dev with",
             "the encoder's own table (unchanged code: the yardstick).  HD_FRAME_GZIP; medians of the repetitions; GB/s of decoded bytes.", ""]
    for r in res["rows"]:
        lines.append("%-5s level %d chunk %7d  %d bytes, stream %d bytes, %d chunks, %d rows" % (
            r["set"], r["level"], r["chunk"], r["bytes"], r["stream_bytes"], r["chunks"], r["nchunks"]))
        lines.append("    (a) ms %s -> %.2f GB/s   candidates %d (%d false): %.1f (%.2f false) per GiB of stream" % (
            " ".join("%.3f" % v for v in r["index_ms"]), r["index_GBps"], r["ncandidates"], r["false_candidates"],
            r["candidates_per_GiB_of_stream"], r["false_candidates_per_GiB_of_stream"]))
        lines.append("    (b) ms %s -> %.2f GB/s   (c) ms %s -> %.2f GB/s   (a)/(c) %.4f   (b)/(c) %.4f" % (
            " ".join("%.3f" % v for v in r["index_decode_ms"]), r["index_decode_GBps"],
            " ".join("%.3f" % v for v in r["table_decode_ms"]), r["table_decode_GBps"], r["index_over_table_decode"],
            r["index_decode_over_table_decode"]))
    lines += ["", "(b)/(c) over the rows: %.4f .. %.4f (expected near 1.5-1.6 from the size pass's 0.51-0.59 of an inflate; no bar)" % (
        res["ratio_min"], res["ratio_max"])]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_index_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.reps, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
