#!/usr/bin/env python3
"""Time of a batch of ranged reads next to the inflate of exactly the members they touch.

A BGZF image of FASTQ-like data (a seeded 64 MiB tile replicated to --gib GiB, as tools/member_index_bench.py builds
it), written by this library's level-6 encoder and gathered on the device, stays in HBM with its member table.  Q seeded
random ranges of 4..256 KiB of the decoded file are read.  After a warm-up, --reps alternated repetitions of
    (a) hipdeflate_read_ranges_dev        the whole call: resolve, scans, inflate of the selected members, verify, gather
    (b) hipdeflate_batch_inflate_dev      over exactly those members, tables made on the host beforehand, into one buffer
                                          -- the path a caller had before, and the yardstick
    (p) hipdeflate_read_ranges_dev        as the sizing call (dst == NULL): the plan alone -- resolve, the five scans and
                                          the first of the call's two waits for its stream
    (w) hipdeflate_batch_inflate_dev      over the whole file, for scale
are timed with device events.  The figures go to --out (profiles/range_read_timing.txt) and, as one JSON line, to stdout.
No bar is set: (a) - (b) is what the passes around the inflate cost, and (p) says how much of that is the plan.

    python tools/range_read_bench.py [--gib 4] [--queries 4096] [--reps 5] [--out profiles/range_read_timing.txt]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def measure(gib=4.0, queries=4096, reps=5, level=6, tile_mib=64, min_kib=4, max_kib=256, seed=1):
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

    n = nb + 1
    dec = dev.DeviceInflate(n)
    s = dec.index(blob)
    assert (s.status, s.nmembers, s.out_bytes) == (0, n, total), (s.status, s.nmembers, s.out_bytes)

    rng = np.random.default_rng(seed)
    lens = rng.integers(min_kib << 10, (max_kib << 10) + 1, queries)
    begins = rng.integers(0, total - (max_kib << 10), queries)
    ends = begins + lens
    q_begin = torch.from_numpy(begins.astype(np.int64)).cuda()
    q_end = torch.from_numpy(ends.astype(np.int64)).cuda()
    out_bytes = int(lens.sum())
    out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")

    # (b)'s tables, made on the host from the index's: the members that hold a byte of some range, back to back
    h_out_off = dec.out_off.cpu().numpy()
    h_out_size = dec.out_size.cpu().numpy().view(np.uint32).astype(np.int64)
    first = np.searchsorted(h_out_off, begins, side="right") - 1
    last = np.searchsorted(h_out_off, ends - 1, side="right") - 1
    cover = np.zeros(n + 1, dtype=np.int64)
    np.add.at(cover, first, 1)
    np.add.at(cover, last + 1, -1)
    sel = np.flatnonzero((np.cumsum(cover)[:n] > 0) & (h_out_size > 0))
    sel_bytes = int(h_out_size[sel].sum())
    idx = torch.from_numpy(sel).cuda()
    b_in_off, b_in_len, b_cap = dec.in_off[idx].contiguous(), dec.in_len[idx].contiguous(), dec.out_size[idx].contiguous()
    b_out_off = torch.from_numpy(np.concatenate(([0], np.cumsum(h_out_size[sel])[:-1])).astype(np.int64)).cuda()
    b_out = torch.empty(sel_bytes, dtype=torch.uint8, device="cuda")
    b_len, b_crc, b_status = (torch.zeros(len(sel), dtype=torch.int32, device="cuda") for _ in range(3))
    whole = torch.empty(total, dtype=torch.uint8, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def ranged():
        return dec.ranges_call(blob, q_begin, q_end, pkg.RANGE_BYTES, n, out, out_bytes)

    def plan_only():
        return dec.ranges_call(blob, q_begin, q_end, pkg.RANGE_BYTES, n, None, 0)

    def selected_inflate():
        dev.device_inflate(blob, b_in_off, b_in_len, b_out, b_out_off, b_cap, b_len, b_crc, b_status)

    def whole_inflate():
        dev.device_inflate(blob, dec.in_off[:n], dec.in_len, whole, dec.out_off, dec.out_size, dec.out_len, dec.crc, dec.status)

    # warm-up of all four, and the check of what is timed
    dst_off, q_len, q_status, rs = ranged()
    assert (rs.status, rs.nrefused, rs.out_bytes, rs.nselected, rs.sel_bytes) == (0, 0, out_bytes, len(sel), sel_bytes), \
        (rs.status, rs.nrefused, rs.out_bytes, rs.nselected, rs.sel_bytes, len(sel), sel_bytes)
    offs = dst_off.cpu().numpy()
    for q in range(0, queries, max(1, queries // 64)):
        assert torch.equal(out[int(offs[q]):int(offs[q]) + int(lens[q])], data[int(begins[q]):int(ends[q])]), q
    assert plan_only()[3].status == 3
    selected_inflate()
    assert int(b_status.abs().sum()) == 0 and torch.equal(b_len, b_cap)
    whole_inflate()
    assert dec.verify(n) == n
    t = {"ranged": [], "selected": [], "plan": [], "whole": []}
    for _ in range(reps):
        t["ranged"].append(timed(ranged)[0])
        t["selected"].append(timed(selected_inflate)[0])
        t["plan"].append(timed(plan_only)[0])
        t["whole"].append(timed(whole_inflate)[0])
    med = {k: sorted(v)[reps // 2] for k, v in t.items()}
    extra = med["ranged"] - med["selected"]
    return {
        "workload": "BGZF image of %.2f GiB FASTQ-like data, level %d, resident in HBM; %d ranges of %d..%d KiB" % (
            total / 2 ** 30, level, queries, min_kib, max_kib),
        "uncompressed_bytes": total, "compressed_bytes": blob.numel(), "members": n, "queries": queries,
        "out_bytes": out_bytes, "nselected": len(sel), "sel_bytes": sel_bytes,
        "ranged_ms": [round(x, 4) for x in t["ranged"]], "selected_inflate_ms": [round(x, 4) for x in t["selected"]],
        "plan_ms": [round(x, 4) for x in t["plan"]], "whole_inflate_ms": [round(x, 4) for x in t["whole"]],
        "ranged_ms_median": round(med["ranged"], 4), "selected_inflate_ms_median": round(med["selected"], 4),
        "plan_ms_median": round(med["plan"], 4), "whole_inflate_ms_median": round(med["whole"], 4),
        "ranged_over_selected": round(med["ranged"] / med["selected"], 4),
        "extra_ms": round(extra, 4), "extra_ms_behind_the_plan": round(extra - med["plan"], 4),
        "ranged_delivered_GBps": round(out_bytes / (med["ranged"] * 1e-3) / 1e9, 1),
        "selected_inflate_GBps": round(sel_bytes / (med["selected"] * 1e-3) / 1e9, 1),
        "whole_inflate_GBps": round(total / (med["whole"] * 1e-3) / 1e9, 1),
        "whole_over_ranged": round(med["whole"] / med["ranged"], 2),
    }


def report(res):
    def row(key):
        return "%s   median %.4f" % (" ".join("%.4f" % x for x in res[key]), res[key + "_median"])
    lines = ["range read timing -- tools/range_read_bench.py", res["workload"],
             "uncompressed bytes            %d" % res["uncompressed_bytes"], "compressed bytes              %d" % res["compressed_bytes"],
             "members                       %d" % res["members"], "queries                       %d" % res["queries"],
             "out_bytes                     %d (sum of the ranges)" % res["out_bytes"],
             "nselected                     %d (distinct members decoded)" % res["nselected"],
             "sel_bytes                     %d (their ISIZE)" % res["sel_bytes"],
             "(a) read_ranges ms per call   " + row("ranged_ms"),
             "(b) inflate of the selected   " + row("selected_inflate_ms"),
             "(p) read_ranges, sizing call  " + row("plan_ms"),
             "(w) inflate of the whole file " + row("whole_inflate_ms"),
             "(a) / (b)                     %.4f" % res["ranged_over_selected"],
             "(a) - (b)                     %.4f ms, of which the plan (p) %.4f ms and tables + verify + gather + the second wait %.4f ms" % (
                 res["extra_ms"], res["plan_ms_median"], res["extra_ms_behind_the_plan"]),
             "(a) delivers                  %.1f GB/s of range bytes; (b) inflates %.1f GB/s; (w) inflates %.1f GB/s" % (
                 res["ranged_delivered_GBps"], res["selected_inflate_GBps"], res["whole_inflate_GBps"]),
             "(w) / (a)                     %.2f" % res["whole_over_ranged"]]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--tile-mib", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_read_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.queries, args.reps, args.level, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
