#!/usr/bin/env python3
"""Time of the size pass and of the framed inflate next to the plain batch inflate of the same payloads.

--gib GiB of the text set and of the FASTQ-like set (a seeded 64 MiB tile replicated) are coded by this encoder at
levels 1 and 6 as 64 KiB zlib members and as 64 KiB gzip members, and stay in HBM.  After a warm-up, --reps rounds in which
the variants take turns, each timed with device events:
    (p0) hipdeflate_batch_inflate_dev on the payloads, tables made by the caller, no CRC-32      the plain inflate
    (pc) the same with the CRC-32 of every output                                                 ... as a gzip reader needs it
    (s)  hipdeflate_batch_inflate_size_dev on the zlib members                                    the size pass
    (fg) hipdeflate_batch_inflate_framed_dev on the gzip members                                  open + inflate + close
    (fz) ... on the zlib members                                                                  ... + the Adler-32 pass
Bars: (s) / (p0) below 1.0 by more than the spread of the rounds; (fg) within 5 % of (pc).  (fz) - (p0) is what the
Adler-32 pass, open and close add for zlib.  One process; every GPU step runs under its own time limit and the first
failure ends the run.  The figures go to --out (profiles/framed_inflate_timing.txt) and, as one JSON line, to stdout.

    python tools/framed_inflate_bench.py [--gib 1] [--reps 3] [--out profiles/framed_inflate_timing.txt]
"""
import argparse
import importlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from stream_bench import Step          # noqa: E402  (a GPU step under its own time limit)

BLOCK = 64 << 10


def kernel_resources(name="k_inflate_size"):
    """registers, LDS and wavefronts per CU of a kernel from the build's resource report, {} where there is none"""
    log = os.path.join(ROOT, "7bgzf_amd", "csrc", "hd_api.resources.log")
    if not os.path.exists(log):
        return {}
    cur, out = None, {}
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur and name + "E" in cur:
            out[m.group(1).strip()] = int(m.group(2))
    if out:
        units = -(-out["LDS Size"] // 1280)
        out["LDS units"] = units
        out["waves per CU"] = min(4 * out["Occupancy"], 128 // units)
    return out


def measure(gib=1.0, reps=3, tile_mib=64):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    L = pkg.lib()
    tile_bytes = tile_mib << 20

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(v):
        return sorted(v)[len(v) // 2]

    rows = []
    tiles = {"text": lambda: synth.text_like(tile_bytes, seed=4321), "fastq": lambda: synth.fastq_like(tile_bytes, seed=1234)}
    for name, make in tiles.items():
        with Step("%s: input" % name, 300):
            tile = torch.from_numpy(make()).cuda()
            data = tile.repeat(max(1, int(gib * (1 << 30)) // tile_bytes))
            total = data.numel()
            n = total // BLOCK
            in_off, in_len = dev.block_table(total, BLOCK)
            torch.cuda.synchronize()
        for level in (1, 6):
            with Step("%s level %d: encode" % (name, level), 300):
                slot = int(L.hipdeflate_bound(BLOCK, level))
                enc = {}
                for frame in (pkg.FRAME_ZLIB, pkg.FRAME_GZIP):
                    e = dev.DeviceDeflate(n, slot=slot)
                    e.run(data, in_off, in_len, level=level, frame=frame)
                    torch.cuda.synchronize()
                    assert int(e.status.abs().sum()) == 0
                    enc[frame] = e
                m_off = torch.arange(n, dtype=torch.int64, device="cuda") * slot
                zl, gz = enc[pkg.FRAME_ZLIB], enc[pkg.FRAME_GZIP]
                # the caller-made tables of the plain inflate: the payloads of the zlib members (2 bytes of header, 4 of trailer)
                p_off, p_len = m_off + 2, zl.out_len - 6
                out = torch.empty(total, dtype=torch.uint8, device="cuda")
                out_off = in_off
                cap = in_len
                out_len, crc, status, osz, used, chk = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(6))
            variants = {
                "p0": lambda: dev.device_inflate(zl.slots, p_off, p_len, out, out_off, cap, out_len, None, status),
                "pc": lambda: dev.device_inflate(zl.slots, p_off, p_len, out, out_off, cap, out_len, crc, status),
                "s": lambda: dev.inflate_size_call(zl.slots, m_off, zl.out_len, pkg.FRAME_ZLIB, osz, used, status),
                "fg": lambda: dev.inflate_framed_call(gz.slots, m_off, gz.out_len, pkg.FRAME_GZIP, out, out_off, cap, out_len, chk, used, status),
                "fz": lambda: dev.inflate_framed_call(zl.slots, m_off, zl.out_len, pkg.FRAME_ZLIB, out, out_off, cap, out_len, chk, used, status),
            }
            ms = {k: [] for k in variants}
            with Step("%s level %d: inflate" % (name, level), 300):
                for k, fn in variants.items():              # warm-up, and every variant's answer held to the input once
                    out.zero_()
                    fn()
                    torch.cuda.synchronize()
                    assert int(status.abs().sum()) == 0, k
                    if k == "s":
                        assert bool((osz == in_len).all()) and bool((used == zl.out_len).all())
                    else:
                        assert torch.equal(out, data) and bool((out_len == in_len).all()), k
                    if k in ("fg", "fz"):
                        assert bool((used == (gz if k == "fg" else zl).out_len).all())
                for _ in range(reps):
                    for k, fn in variants.items():
                        ms[k].append(timed(fn))
            med = {k: median(v) for k, v in ms.items()}
            spread = max((max(v) - min(v)) / median(v) for v in (ms["s"], ms["p0"]))
            rows.append({
                "set": name, "level": level, "bytes": total, "members": n, "zlib_bytes": int(zl.out_len.sum()),
                "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                "GBps_out": {k: round(total / med[k] / 1e6, 2) for k in med},
                "size_over_plain": round(med["s"] / med["p0"], 4), "spread_of_the_rounds": round(spread, 4),
                "size_below_plain_by_more_than_the_spread": bool(med["s"] / med["p0"] < 1.0 - spread),
                "gzip_framed_over_plain_with_crc": round(med["fg"] / med["pc"], 4),
                "gzip_framed_over_plain_without_crc": round(med["fg"] / med["p0"], 4),
                "gzip_within_5_percent": bool(med["fg"] <= 1.05 * med["pc"]),
                "zlib_framed_over_plain_without_crc": round(med["fz"] / med["p0"], 4),
                "zlib_adler_open_close_ms": round(med["fz"] - med["p0"], 3),
            })
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del enc, zl, gz, out, variants
            torch.cuda.empty_cache()
        del data, tile
        torch.cuda.empty_cache()
    assert L.hipdeflate_stall_count() == 0
    return {"rows": rows, "k_inflate_size": kernel_resources("k_inflate_size"), "k_inflate": kernel_resources("k_inflate"),
            "k_inflate_framed": kernel_resources("k_inflate_framed"),
            "size_bar_met": all(r["size_below_plain_by_more_than_the_spread"] for r in rows),
            "gzip_bar_met": all(r["gzip_within_5_percent"] for r in rows)}


def report(res):
    lines = ["framed inflate timing -- tools/framed_inflate_bench.py",
             "(p0) plain batch inflate of the payloads, no CRC | (pc) with CRC | (s) size pass, zlib members | (fg) framed, gzip | (fz) framed, zlib",
             ""]
    for k in ("k_inflate_size", "k_inflate", "k_inflate_framed"):
        r = res[k]
        if r:
            lines.append("%-16s %d VGPRs, %d SGPRs, %d bytes of LDS (%d units), scratch %d: %d wavefronts per CU" % (
                k, r["VGPRs"], r["TotalSGPRs"], r["LDS Size"], r["LDS units"], r["ScratchSize"], r["waves per CU"]))
    lines.append("")
    for r in res["rows"]:
        lines.append("%-5s level %d  %d bytes in %d members of 64 KiB (%d bytes of zlib members)" % (
            r["set"], r["level"], r["bytes"], r["members"], r["zlib_bytes"]))
        for k in ("p0", "pc", "s", "fg", "fz"):
            lines.append("    (%-2s) ms %s -> %.2f GB/s out" % (k, " ".join("%.3f" % x for x in r["ms"][k]), r["GBps_out"][k]))
        lines.append("    (s)/(p0) %.4f, spread of the rounds %.4f: %s" % (
            r["size_over_plain"], r["spread_of_the_rounds"],
            "below 1.0 by more than the spread" if r["size_below_plain_by_more_than_the_spread"] else "NOT below 1.0 by more than the spread"))
        lines.append("    (fg)/(pc) %.4f  %s   (fg)/(p0) %.4f" % (
            r["gzip_framed_over_plain_with_crc"], "within 5 %" if r["gzip_within_5_percent"] else "NOT within 5 %",
            r["gzip_framed_over_plain_without_crc"]))
        lines.append("    (fz)/(p0) %.4f: the Adler-32 pass, open and close add %.3f ms" % (
            r["zlib_framed_over_plain_without_crc"], r["zlib_adler_open_close_ms"]))
    lines += ["", "bar (a): the size pass below the plain inflate by more than the spread, on every row: %s" % ("met" if res["size_bar_met"] else "NOT met"),
              "bar (b): the framed call on gzip members within 5 %% of the plain inflate with CRC-32, on every row: %s" % ("met" if res["gzip_bar_met"] else "NOT met")]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framed_inflate_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.reps, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
