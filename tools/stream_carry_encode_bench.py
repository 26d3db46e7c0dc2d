#!/usr/bin/env python3
"""What priming every chunk with the 32 KiB in front of it costs the stream encoder, and what it gains.

--gib GiB of the text set and of the FASTQ-like set (a seeded 64 MiB tile replicated) stay in HBM.  For levels 3 and 6 and
chunks of 16 KiB, 64 KiB and 1 MiB, after a warm-up of both, --reps pairs of
    (i) hipdeflate_stream_deflate_dev, HD_FRAME_GZIP         chunks that know nothing of each other
    (p) hipdeflate_stream_deflate_carry_dev, HD_FRAME_GZIP   every chunk parsed with min(32768, its offset) & ~1023 bytes of history
are timed with device events, ALTERNATED in one run; medians.  (p)'s check value is held to the input's CRC-32, and the
first --verify-mib MiB of its stream are inflated by zlib on the host and compared.
The supposition this file confirms or refutes (hd_deflate_wg.hpp: a replayed piece is an eighth of a piece's work):
    (p) / (i) in time  ~  1 + prime / (8 * chunk_bytes),   prime = 32768
--bench-ab FILE: lines "<build> <run-label>\\t<bench.py's JSON line>", builds `parent` and `new` alternated by whoever made the
file (the two unchanged paths the stream encoder's change could touch); they are tabulated under the timing.
--results FILE: the JSON line an earlier run of this tool printed; the report is written from it and nothing is measured (the
bench.py lines may be taken after the timing).
One process; every GPU step runs under its own time limit and the first failure ends the run.

    python tools/stream_carry_encode_bench.py [--gib 1] [--reps 3] [--bench-ab FILE] [--results FILE]
                                              [--out profiles/stream_encode_carry_timing.txt]
"""
import argparse
import faulthandler
import importlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW = 32768


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


def measure(gib=1.0, reps=3, tile_mib=64, verify_mib=8, levels=(3, 6), chunks=(16 << 10, 64 << 10, 1 << 20)):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sm = importlib.import_module("stream_model")         # the host's fold: the CRC-32 of a tile repeated from the tile's own
    L = pkg.lib()
    tile_bytes = tile_mib << 20

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
            crc_tile = zlib.crc32(memoryview(tile.cpu().numpy()))
            crc_data = sm.crc_fold([crc_tile] * (total // tile_bytes), [tile_bytes] * (total // tile_bytes))
            head = bytes(tile[:min(verify_mib << 20, tile_bytes)].cpu().numpy())
        for level in levels:
            for chunk in chunks:
                nchunks = (total + chunk - 1) // chunk
                bound = int(L.hipdeflate_stream_bound(total, chunk, level, pkg.FRAME_GZIP))
                dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
                tab = torch.zeros(nchunks + 1, dtype=torch.int64, device="cuda")

                def plain():
                    return dev.deflate_stream_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab)

                def primed():
                    return dev.deflate_stream_carry_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab)
                with Step("%s level %d chunk %d" % (name, level, chunk), 300):
                    si = plain()                                                          # warm-up of both
                    assert (si.status, si.in_bytes, si.nchunks, si.check) == (0, total, nchunks, crc_data), (si.status, hex(si.check))
                    sp = primed()
                    assert (sp.status, sp.in_bytes, sp.nchunks, sp.check) == (0, total, nchunks, crc_data), (sp.status, hex(sp.check))
                    # the primed stream is one stream to zlib: its first bytes inflated on the host
                    take = bytes(dst[:min(sp.out_bytes, len(head))].cpu().numpy())
                    d = zlib.decompressobj(31)
                    got = d.decompress(take, len(head))
                    assert len(got) >= len(head) // 4 and got == head[:len(got)]
                    i_ms, p_ms = [], []
                    for _ in range(reps):                                                 # alternated
                        i_ms.append(timed(plain)[0])
                        p_ms.append(timed(primed)[0])
                i, p = median(i_ms), median(p_ms)
                rows.append({
                    "set": name, "level": level, "chunk": chunk, "bytes": total, "nchunks": nchunks,
                    "independent_ms": [round(x, 3) for x in i_ms], "primed_ms": [round(x, 3) for x in p_ms],
                    "independent_GBps": round(total / i / 1e6, 2), "primed_GBps": round(total / p / 1e6, 2),
                    "independent_bytes": int(si.out_bytes), "primed_bytes": int(sp.out_bytes),
                    "independent_ratio": round(si.out_bytes / total, 5), "primed_ratio": round(sp.out_bytes / total, 5),
                    "primed_over_independent_time": round(p / i, 4),
                    "supposed_time": round(1 + WINDOW / (8.0 * chunk), 4),
                })
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                del dst, tab
                torch.cuda.empty_cache()
        del data, tile
        torch.cuda.empty_cache()
    assert L.hipdeflate_stall_count() == 0
    return {"rows": rows}


def read_bench_ab(path):
    """-> { run label: { build: [GB/s, ...] } } in file order"""
    runs = {}
    for line in open(path):
        if "\t" not in line:
            continue
        head, js = line.rstrip("\n").split("\t", 1)
        build, label = head.split(" ", 1)
        try:
            value = json.loads(js)["value"]
        except (ValueError, KeyError):
            continue
        runs.setdefault(label, {}).setdefault(build, []).append(value)
    return runs


def report(res, bench_ab=None):
    lines = ["stream encoder, chunks that carry the window -- tools/stream_carry_encode_bench.py",
             "(i) hipdeflate_stream_deflate_dev | (p) hipdeflate_stream_deflate_carry_dev; HD_FRAME_GZIP, device events, alternated, medians",
             "ratio = stream bytes / input bytes; supposed (p)/(i) = 1 + 32768 / (8 * chunk_bytes)", ""]
    for r in res["rows"]:
        lines.append("%-5s level %d chunk %7d  %d bytes in %d chunks" % (r["set"], r["level"], r["chunk"], r["bytes"], r["nchunks"]))
        lines.append("    (i) ms %s -> %.2f GB/s  ratio %.5f" % (" ".join("%.3f" % x for x in r["independent_ms"]), r["independent_GBps"],
                                                               r["independent_ratio"]))
        lines.append("    (p) ms %s -> %.2f GB/s  ratio %.5f" % (" ".join("%.3f" % x for x in r["primed_ms"]), r["primed_GBps"],
                                                               r["primed_ratio"]))
        lines.append("    (p)/(i) time %.4f (supposed %.4f)   (p)/(i) bytes %.4f" % (
            r["primed_over_independent_time"], r["supposed_time"], r["primed_bytes"] / r["independent_bytes"]))
    over = [r for r in res["rows"] if r["primed_over_independent_time"] > 1.05 * r["supposed_time"]]
    lines += ["", "the supposition (p)/(i) = 1 + 32768 / (8 * chunk_bytes) holds within 5 %% on %d of %d rows%s" % (
        len(res["rows"]) - len(over), len(res["rows"]), "" if not over else "; (p) takes longer than supposed on: " + ", ".join(
            "%s %d %d KiB (%.2f against %.2f)" % (r["set"], r["level"], r["chunk"] >> 10, r["primed_over_independent_time"],
                                                   r["supposed_time"]) for r in over))]
    lines.append("")
    if bench_ab:
        lines.append("unchanged paths, parent build against this one, alternated in one run on one device (bench.py, GB/s per run):")
        for label, builds in bench_ab.items():
            lines.append(("  python bench.py %s" % label).rstrip())
            for build in ("parent", "new"):
                v = builds.get(build, [])
                lines.append("    %-6s %s%s" % (build, " ".join("%.3f" % x for x in v), "   (slowest %.3f)" % min(v) if v else " not measured"))
            if builds.get("parent") and builds.get("new"):
                lines.append("    the new build's slowest run is %s the parent's slowest" % (
                    "not below" if min(builds["new"]) >= min(builds["parent"]) else "BELOW"))
    else:
        lines.append("unchanged paths against the parent build: not measured")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--verify-mib", type=int, default=8)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_encode_carry_timing.txt"))
    ap.add_argument("--results", default=None, help="this tool's JSON line of an earlier run: write the report from it, measure nothing")
    args = ap.parse_args()
    if args.results:
        res = json.loads(open(args.results).read().strip().splitlines()[-1])
    else:
        res = measure(args.gib, args.reps, args.tile_mib, args.verify_mib)
    ab = read_bench_ab(args.bench_ab) if args.bench_ab else None
    with open(args.out, "w") as f:
        f.write(report(res, ab))
    res["bench_ab"] = ab
    print(json.dumps(res))


if __name__ == "__main__":
    main()
