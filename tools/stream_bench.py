#!/usr/bin/env python3
"""Time of ONE gzip stream coded in parallel chunks next to what a caller had before and next to the ceiling.

--gib GiB of the text set and of the FASTQ-like set (a seeded 64 MiB tile replicated; no chunk sees the repetition) stay
in HBM.  For level 6 and level 1, chunks of 64 KiB and 1 MiB, after a warm-up, --reps repetitions of
    (a) hipdeflate_stream_deflate_dev, HD_FRAME_GZIP         the whole call: table, encode, scan, fold, gather, ends
    (c) the same chunks as HD_FRAME_MIGZ members             hipdeflate_batch_deflate_dev + scan + compact: the ceiling
are timed with device events, and once
    (b) 64 MiB of the same bytes as ONE block, HD_FRAME_GZIP  what hipdeflate_batch_deflate_dev gave a one-stream caller
    (d) hipdeflate_stream_inflate_dev on (a)'s output, compared with the input
    (a1) the call of (a) with every chunk in one window (hipdeflate_test_stream_window): what the window seams cost
Then one run of (a) over --big-gib GiB (default 5: ISIZE wraps, offsets pass 2^32), decoded back on the device and
compared.  One process; every GPU step runs under its own time limit (the process exits when one runs out) and the
first failure ends the run.  The figures go to --out (profiles/stream_timing.txt) and, as one JSON line, to stdout.
The bar: (a) within 5 % of (c).

    python tools/stream_bench.py [--gib 1] [--big-gib 5] [--reps 3] [--out profiles/stream_timing.txt]
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

ONE_BLOCK = 64 << 20


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


def measure(gib=1.0, big_gib=5.0, reps=3, tile_mib=64):
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
        for level in (6, 1):
            # (b) one block of 64 MiB: the single-stream caller of before
            with Step("%s level %d: one block" % (name, level), 300):
                one = dev.DeviceDeflate(1, slot=int(L.hipdeflate_bound(ONE_BLOCK, level)))
                off1, len1 = dev.block_table(ONE_BLOCK, ONE_BLOCK)
                one.run(data, off1, len1, level=level, frame=pkg.FRAME_GZIP)          # warm-up
                torch.cuda.synchronize()
                one_ms = timed(lambda: one.run(data, off1, len1, level=level, frame=pkg.FRAME_GZIP))[0]
                assert int(one.status[0]) == 0
                one_bytes = int(dev.to_numpy_u32(one.out_len)[0])
                del one
            for chunk in (64 << 10, 1 << 20):
                nchunks = (total + chunk - 1) // chunk
                bound = int(L.hipdeflate_stream_bound(total, chunk, level, pkg.FRAME_GZIP))
                dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
                tab = torch.zeros(nchunks + 1, dtype=torch.int64, device="cuda")
                with Step("%s level %d chunk %d: stream" % (name, level, chunk), 300):
                    s = dev.deflate_stream_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab)     # warm-up
                    assert (s.status, s.in_bytes, s.nchunks) == (0, total, nchunks), (s.status, s.in_bytes, s.nchunks)
                    a_ms = [timed(lambda: dev.deflate_stream_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab))[0]
                            for _ in range(reps)]
                    assert s.check == crc_data, (hex(s.check), hex(crc_data))
                    # (a1) the same call with every chunk in ONE window (the test entry; more scratch than the contract allows):
                    # what the seams between windows cost
                    try:
                        L.hipdeflate_test_stream_window(nchunks)
                        s1 = dev.deflate_stream_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab)
                        assert (s1.status, s1.out_bytes, s1.check) == (0, s.out_bytes, s.check)
                        a1_ms = [timed(lambda: dev.deflate_stream_call(data, level, pkg.FRAME_GZIP, chunk, dst, bound, tab))[0]
                                 for _ in range(reps)]
                    finally:
                        L.hipdeflate_test_stream_window(0)
                with Step("%s level %d chunk %d: stream decode" % (name, level, chunk), 300):
                    back = torch.empty(total, dtype=torch.uint8, device="cuda")
                    stream = dst[:s.out_bytes]
                    ds = dev.inflate_stream_call(stream, pkg.FRAME_GZIP, tab, nchunks, chunk, total, back, total)
                    assert (ds.status, ds.check) == (0, s.check), (ds.status, ds.bad_chunk)
                    assert torch.equal(back, data)
                    d_ms = [timed(lambda: dev.inflate_stream_call(stream, pkg.FRAME_GZIP, tab, nchunks, chunk, total, back, total))[0]
                            for _ in range(reps)]
                    del back
                with Step("%s level %d chunk %d: members" % (name, level, chunk), 300):
                    enc = dev.DeviceDeflate(nchunks, slot=int(L.hipdeflate_bound(chunk, level)))
                    in_off, in_len = dev.block_table(total, chunk)

                    def members():
                        enc.run(data, in_off, in_len, level=level, frame=pkg.FRAME_MIGZ)
                        enc.scan()
                        enc.compact(dst)
                    members()                                                                            # warm-up
                    torch.cuda.synchronize()
                    assert int(enc.status.abs().sum()) == 0
                    c_bytes = int(enc.total[0])
                    c_ms = [timed(members)[0] for _ in range(reps)]
                    del enc, in_off, in_len
                a, c, d, a1 = median(a_ms), median(c_ms), median(d_ms), median(a1_ms)
                rows.append({
                    "set": name, "level": level, "chunk": chunk, "bytes": total, "nchunks": nchunks,
                    "stream_ms": [round(x, 3) for x in a_ms], "members_ms": [round(x, 3) for x in c_ms],
                    "stream_inflate_ms": [round(x, 3) for x in d_ms], "one_window_ms": [round(x, 3) for x in a1_ms],
                    "one_window_over_members": round(a1 / c, 4),
                    "stream_GBps": round(total / a / 1e6, 2), "members_GBps": round(total / c / 1e6, 2),
                    "stream_inflate_GBps": round(total / d / 1e6, 2),
                    "stream_over_members": round(a / c, 4), "within_5_percent": bool(a <= 1.05 * c),
                    "one_block_GBps": round(ONE_BLOCK / one_ms / 1e6, 3),
                    "stream_over_one_block": round((total / a) / (ONE_BLOCK / one_ms), 1),
                    "stream_bytes": int(s.out_bytes), "members_bytes": c_bytes,
                    "stream_ratio": round(s.out_bytes / total, 5), "one_block_ratio": round(one_bytes / ONE_BLOCK, 5),
                    "windows": -(-nchunks // max(1, pkg.STREAM_WINDOW_BYTES // int(L.hipdeflate_bound(chunk, level)))),
                })
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                del dst, tab
                torch.cuda.empty_cache()
        # the 64-bit paths: one stream of big_gib GiB, decoded back and compared
        if name == "fastq" and big_gib > 0:
            with Step("big run", 600):
                level, chunk = 1, 1 << 20
                big = tile.repeat(int(big_gib * (1 << 30)) // tile_bytes)
                n = big.numel()
                nchunks = (n + chunk - 1) // chunk
                bound = int(L.hipdeflate_stream_bound(n, chunk, level, pkg.FRAME_GZIP))
                dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
                tab = torch.zeros(nchunks + 1, dtype=torch.int64, device="cuda")
                ms, s = timed(lambda: dev.deflate_stream_call(big, level, pkg.FRAME_GZIP, chunk, dst, bound, tab))
                assert (s.status, s.in_bytes) == (0, n)
                crc = sm.crc_fold([crc_tile] * (n // tile_bytes), [tile_bytes] * (n // tile_bytes))
                assert s.check == crc, (hex(s.check), hex(crc))
                isize = int.from_bytes(bytes(dst[s.out_bytes - 4:s.out_bytes].cpu().numpy()), "little")
                assert isize == n % (1 << 32)
                back = torch.empty(n, dtype=torch.uint8, device="cuda")
                dms, ds = timed(lambda: dev.inflate_stream_call(dst[:s.out_bytes], pkg.FRAME_GZIP, tab, nchunks, chunk, n, back, n))
                assert (ds.status, ds.check, ds.out_bytes) == (0, crc, n), (ds.status, ds.bad_chunk)
                assert torch.equal(back, big)
                big_row = {"bytes": n, "level": level, "chunk": chunk, "stream_bytes": int(s.out_bytes), "stream_ms": round(ms, 3),
                           "stream_GBps": round(n / ms / 1e6, 2), "inflate_ms": round(dms, 3), "crc32": "%08x" % crc,
                           "isize": isize, "round_trip": "equal"}
                del big, dst, tab, back
        del data, tile
        torch.cuda.empty_cache()
    assert L.hipdeflate_stall_count() == 0
    return {"rows": rows, "big": big_row if big_gib > 0 else None, "all_within_5_percent": all(r["within_5_percent"] for r in rows)}


def report(res):
    lines = ["stream timing -- tools/stream_bench.py",
             "(a) hipdeflate_stream_deflate_dev, GZIP | (c) the same chunks as MiGz members: batch + scan + compact | "
             "(b) 64 MiB as one block, GZIP | (d) hipdeflate_stream_inflate_dev on (a)'s stream", ""]
    for r in res["rows"]:
        lines.append("%-5s level %d chunk %7d  %d bytes in %d chunks, %d window(s)" % (
            r["set"], r["level"], r["chunk"], r["bytes"], r["nchunks"], r["windows"]))
        lines.append("    (a) ms %s -> %.2f GB/s   (c) ms %s -> %.2f GB/s   (a)/(c) %.4f  %s" % (
            " ".join("%.3f" % x for x in r["stream_ms"]), r["stream_GBps"], " ".join("%.3f" % x for x in r["members_ms"]),
            r["members_GBps"], r["stream_over_members"], "within 5 %" if r["within_5_percent"] else "NOT within 5 %"))
        lines.append("    (b) %.3f GB/s: (a) is %.1f x   sizes: (a) %d bytes = %.5f of the input, (b) %.5f of its 64 MiB, (c) %d bytes" % (
            r["one_block_GBps"], r["stream_over_one_block"], r["stream_bytes"], r["stream_ratio"], r["one_block_ratio"],
            r["members_bytes"]))
        lines.append("    (a1) one window: ms %s   (a1)/(c) %.4f" % (" ".join("%.3f" % x for x in r["one_window_ms"]),
                                                                    r["one_window_over_members"]))
        lines.append("    (d) ms %s -> %.2f GB/s" % (" ".join("%.3f" % x for x in r["stream_inflate_ms"]), r["stream_inflate_GBps"]))
    if res["big"]:
        b = res["big"]
        lines += ["", "one stream of %d bytes (level %d, chunk %d): %d bytes out in %.3f ms (%.2f GB/s), CRC-32 %s, ISIZE %d; "
                  "inflated back on the device in %.3f ms, %s" % (b["bytes"], b["level"], b["chunk"], b["stream_bytes"], b["stream_ms"],
                                                                    b["stream_GBps"], b["crc32"], b["isize"], b["inflate_ms"], b["round_trip"])]
    lines += ["", "bar: (a) within 5 %% of (c) on every row: %s" % ("met" if res["all_within_5_percent"] else "NOT met"),
              "what (a) adds to (c): the chunk table, the fold (one scan, one pass of a lane per chunk), header and trailer, and one",
              "wait for the stream per window (the windows column).  (a1) is the same call with every chunk in one window -- more",
              "scratch than HD_STREAM_WINDOW_BYTES allows, through the test entry: (a) - (a1) is what the seam between windows costs",
              "(the encode kernel's tail runs once per window with the chip partly empty, the gather of a window does not overlap the",
              "next window's encode, and the host round trip in between), (a1) - (c) what the call's own passes cost."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--big-gib", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.big_gib, args.reps, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
