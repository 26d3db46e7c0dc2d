#!/usr/bin/env python3
"""Time of the device member index next to the inflate it feeds.

A BGZF image of FASTQ-like data (a seeded 64 MiB tile replicated to --gib GiB, as bench.py's decode runs replicate a
tile), written by this library's level-6 encoder and gathered on the device, stays in HBM.  After a warm-up, --reps
alternated repetitions of
    hipdeflate_index_members_dev          (the whole call: its kernels and the two host reads of a count in between)
    hipdeflate_batch_inflate_dev          on the table the index produced
are timed with device events.  The figures go to --out (profiles/member_index_timing.txt) and, as one JSON line, to
stdout.  The bar (DESIGN.md "Device member index"): the index takes at most a tenth of the inflate's time.

    python tools/member_index_bench.py [--gib 16] [--reps 5] [--out profiles/member_index_timing.txt]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes per second, MI355X


def count_candidates(torch, blob, chunk=1 << 28):
    """positions that can start a member (1f 8b 08, FLG & 0xe4 == 4), counted with torch: the index keeps its
    candidate list to itself"""
    n, total = blob.numel(), 0
    for o in range(0, n, chunk):
        v = blob[o:min(n, o + chunk + 3)]
        m = (v[:-3] == 0x1f) & (v[1:-2] == 0x8b) & (v[2:-1] == 8) & ((v[3:] & 0xe4) == 4)
        total += int(m.sum())
    return total


def measure(gib=16.0, reps=5, level=6, tile_mib=64):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    block = pkg.BGZF_BLOCK
    tile_bytes = (tile_mib << 20) // block * block
    tile = torch.from_numpy(synth.fastq_like(tile_bytes, seed=1234, first_record=100_000_000)).cuda()
    data = tile.repeat(max(1, int(gib * (1 << 30)) // tile_bytes))
    total = data.numel()
    # the file image: members by the level-6 encoder, gathered on the device, + the EOF member
    in_off, in_len = dev.block_table(total, block)
    nb = in_off.numel()
    enc = dev.DeviceDeflate(nb)
    enc.run(data, in_off, in_len, level=level)
    enc.scan()
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    comp = int(enc.total[0])
    blob = torch.empty(comp + len(pkg.BGZF_EOF), dtype=torch.uint8, device="cuda")
    enc.compact(blob)
    blob[comp:] = torch.frombuffer(bytearray(pkg.BGZF_EOF), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    del enc, in_off, in_len
    torch.cuda.empty_cache()

    dec = dev.DeviceInflate(nb + 1)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def inflate():
        dev.device_inflate(blob, dec.in_off[:nb + 1], dec.in_len, out, dec.out_off, dec.out_size, dec.out_len, dec.crc, dec.status)

    s = dec.index(blob)                                     # warm-up of both, and the check of what is timed
    assert (s.status, s.nmembers, s.out_bytes, s.end_offset) == (0, nb + 1, total, blob.numel()), \
        (s.status, s.nmembers, s.out_bytes, s.end_offset)
    inflate()
    assert dec.verify(nb + 1) == nb + 1 and torch.equal(out, data)
    t_index, t_inflate = [], []
    for _ in range(reps):
        t_index.append(timed(lambda: dec.index(blob))[0])
        t_inflate.append(timed(inflate)[0])
    assert dec.verify(nb + 1) == nb + 1
    idx_ms, inf_ms = sorted(t_index)[reps // 2], sorted(t_inflate)[reps // 2]
    rate = blob.numel() / (idx_ms * 1e-3)
    return {
        "workload": "BGZF image of %.2f GiB FASTQ-like data, level %d, resident in HBM" % (total / 2 ** 30, level),
        "uncompressed_bytes": total, "compressed_bytes": blob.numel(), "members": nb + 1,
        "candidates": count_candidates(torch, blob),
        "index_ms": [round(x, 4) for x in t_index], "inflate_ms": [round(x, 4) for x in t_inflate],
        "index_ms_median": round(idx_ms, 4), "inflate_ms_median": round(inf_ms, 4),
        "index_over_inflate": round(idx_ms / inf_ms, 5),
        "index_read_GBps": round(rate / 1e9, 1), "index_share_of_hbm_peak": round(rate / HBM_PEAK, 4),
        "inflate_moved_GBps": round((blob.numel() + total) / (inf_ms * 1e-3) / 1e9, 1),
        "bar": "index <= inflate / 10", "bar_met": bool(idx_ms * 10 <= inf_ms),
    }


def report(res):
    lines = ["member index timing -- tools/member_index_bench.py", res["workload"],
             "uncompressed bytes   %d" % res["uncompressed_bytes"], "compressed bytes     %d" % res["compressed_bytes"],
             "members              %d" % res["members"], "candidates           %d (positions with 1f 8b 08 and a fitting FLG)" % res["candidates"],
             "index   ms per call  %s   median %.4f" % (" ".join("%.4f" % x for x in res["index_ms"]), res["index_ms_median"]),
             "inflate ms per call  %s   median %.4f" % (" ".join("%.4f" % x for x in res["inflate_ms"]), res["inflate_ms_median"]),
             "index / inflate      %.5f   (bar: <= 0.1 -- %s)" % (res["index_over_inflate"], "met" if res["bar_met"] else "MISSED"),
             "index read rate      %.1f GB/s = %.2f %% of 8 TB/s (compressed bytes over the call's time)" % (
                 res["index_read_GBps"], 100 * res["index_share_of_hbm_peak"]),
             "inflate moved        %.1f GB/s (compressed in + uncompressed out)" % res["inflate_moved_GBps"]]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_index_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.reps, args.level, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
