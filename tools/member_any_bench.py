#!/usr/bin/env python3
"""Time of the member index that sizes by decoding (hipdeflate_index_members_any_dev) next to the inflate it feeds.

Files of PLAIN gzip members -- no length field, zlib's streams -- of text and of FASTQ-like data: a seeded tile cut into
members of 16 KiB and of 64 KiB of input, coded by zlib at levels 1 and 6 on the host, and the tile's image replicated on
the device to --gib GiB of input (as bench.py's decode runs replicate a tile).  After a warm-up that checks the result,
--reps alternated repetitions of
    hipdeflate_index_members_any_dev      (the whole call: its kernels and the host reads of three counts in between)
    hipdeflate_batch_inflate_dev          on the table the index produced
are timed with device events, in the same run.  Then a BGZF image of the FASTQ-like data, written by this library's level-6
encoder, which has no member to size: the new call against hipdeflate_index_members_dev, alternated as well.  The figures
go to --out (profiles/member_any_timing.txt) and, as one JSON line, to stdout.  No bar: the index decodes every member once
without output, so about the size pass's share of an inflate is expected (profiles/framed_inflate_timing.txt: 0.51 .. 0.59).

    python tools/member_any_bench.py [--gib 1] [--reps 3] [--out profiles/member_any_timing.txt]
"""
import argparse
import importlib
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def plain_members(tile, member_in, level):
    """the tile as back-to-back gzip members of member_in input bytes, FLG 0 -> bytes"""
    out = []
    for o in range(0, len(tile), member_in):
        chunk = tile[o:o + member_in]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + c.compress(chunk) + c.flush() + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def median(v):
    return sorted(v)[len(v) // 2]


def measure_plain(torch, dev, tile, name, member_in, level, gib, reps):
    image = plain_members(tile, member_in, level)
    reps_n = max(1, int(gib * (1 << 30)) // len(tile))
    img = torch.frombuffer(bytearray(image), dtype=torch.uint8).cuda()
    blob = torch.empty(reps_n * len(image) + 16, dtype=torch.uint8, device="cuda")[:reps_n * len(image)]
    blob.view(reps_n, len(image))[:] = img[None, :]
    members = reps_n * ((len(tile) + member_in - 1) // member_in)
    total = reps_n * len(tile)
    dec = dev.DeviceInflate(members)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")

    def inflate():
        dev.device_inflate(blob, dec.in_off[:members], dec.in_len, out, dec.out_off, dec.out_size, dec.out_len, dec.crc, dec.status)

    s = dec.index_any(blob)                                  # warm-up of both, and the check of what is timed
    assert (s.status, s.nmembers, s.out_bytes, s.end_offset) == (0, members, total, blob.numel()), (s.status, s.nmembers, s.out_bytes, s.end_offset)
    inflate()
    assert dec.verify(members) == members
    ref = torch.frombuffer(bytearray(tile), dtype=torch.uint8).cuda()
    assert torch.equal(out[:len(tile)], ref) and torch.equal(out[-len(tile):], ref)
    t_index, t_inflate = [], []
    for _ in range(reps):
        t_index.append(timed(torch, lambda: dec.index_any(blob))[0])
        t_inflate.append(timed(torch, inflate)[0])
    i_ms, f_ms = median(t_index), median(t_inflate)
    return {"data": name, "member_in": member_in, "level": level, "uncompressed_bytes": total, "compressed_bytes": blob.numel(),
            "members": members, "ncandidates": s.ncandidates, "nsized": s.nsized,
            "index_ms": [round(x, 3) for x in t_index], "inflate_ms": [round(x, 3) for x in t_inflate],
            "index_ms_median": round(i_ms, 3), "inflate_ms_median": round(f_ms, 3), "index_over_inflate": round(i_ms / f_ms, 3),
            "index_plus_inflate_over_inflate": round((i_ms + f_ms) / f_ms, 3)}


def measure_bgzf(torch, pkg, dev, tile, gib, reps):
    block = pkg.BGZF_BLOCK
    t = torch.frombuffer(bytearray(tile[:len(tile) // block * block]), dtype=torch.uint8).cuda()
    data = t.repeat(max(1, int(gib * (1 << 30)) // t.numel()))
    total = data.numel()
    in_off, in_len = dev.block_table(total, block)
    nb = in_off.numel()
    enc = dev.DeviceDeflate(nb)
    enc.run(data, in_off, in_len, level=6)
    enc.scan()
    torch.cuda.synchronize()
    assert int(enc.status.abs().sum()) == 0
    comp = int(enc.total[0])
    blob = torch.empty(comp + len(pkg.BGZF_EOF), dtype=torch.uint8, device="cuda")
    enc.compact(blob)
    blob[comp:] = torch.frombuffer(bytearray(pkg.BGZF_EOF), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    del enc, data
    a, b = dev.DeviceInflate(nb + 1), dev.DeviceInflate(nb + 1)
    so, sn = a.index(blob), b.index_any(blob)
    assert (so.status, sn.status, sn.nsized) == (0, 0, 0) and (so.nmembers, so.out_bytes, so.end_offset) == (sn.nmembers, sn.out_bytes, sn.end_offset)
    for x, y in zip((a.in_off, a.in_len, a.out_size, a.out_off, a.crc_want), (b.in_off, b.in_len, b.out_size, b.out_off, b.crc_want)):
        assert torch.equal(x, y)
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(timed(torch, lambda: a.index(blob))[0])
        t_new.append(timed(torch, lambda: b.index_any(blob))[0])
    return {"compressed_bytes": blob.numel(), "members": nb + 1, "ncandidates_new": sn.ncandidates,
            "old_ms": [round(x, 3) for x in t_old], "new_ms": [round(x, 3) for x in t_new],
            "old_ms_median": round(median(t_old), 3), "new_ms_median": round(median(t_new), 3),
            "new_over_old": round(median(t_new) / median(t_old), 3)}


def measure(gib=1.0, reps=3, tile_mib=32):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    n = tile_mib << 20
    tiles = {"text": bytes(synth.text_like(n, seed=77)), "fastq": bytes(synth.fastq_like(n, seed=1234, first_record=100_000_000))}
    rows = [measure_plain(torch, dev, tiles[name], name, member_in, level, gib, reps)
            for name in ("text", "fastq") for member_in in (16 << 10, 64 << 10) for level in (1, 6)]
    return {"plain": rows, "bgzf": measure_bgzf(torch, pkg, dev, tiles["fastq"], gib, reps)}


def report(res):
    lines = ["member index that sizes by decoding -- tools/member_any_bench.py",
             "plain gzip members (zlib), %.2f GiB of input per file, resident in HBM; ms per call, every repetition and the median" %
             (res["plain"][0]["uncompressed_bytes"] / 2 ** 30),
             "data  member level  compressed  members  ncand  nsized | index ms (median) | inflate ms (median) | index/inflate  (index+inflate)/inflate"]
    for r in res["plain"]:
        lines.append("%-5s %5dK %5d %11d %8d %6d %7d | %s (%.3f) | %s (%.3f) | %.3f  %.3f" % (
            r["data"], r["member_in"] >> 10, r["level"], r["compressed_bytes"], r["members"], r["ncandidates"], r["nsized"],
            " ".join("%.3f" % x for x in r["index_ms"]), r["index_ms_median"], " ".join("%.3f" % x for x in r["inflate_ms"]),
            r["inflate_ms_median"], r["index_over_inflate"], r["index_plus_inflate_over_inflate"]))
    b = res["bgzf"]
    lines += ["BGZF image (level 6, %d members, %d bytes): no member to size" % (b["members"], b["compressed_bytes"]),
              "hipdeflate_index_members_dev      ms  %s   median %.3f" % (" ".join("%.3f" % x for x in b["old_ms"]), b["old_ms_median"]),
              "hipdeflate_index_members_any_dev  ms  %s   median %.3f   (%d candidates)" % (" ".join("%.3f" % x for x in b["new_ms"]),
                                                                                            b["new_ms_median"], b["ncandidates_new"]),
              "new / old                             %.3f" % b["new_over_old"]]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tile-mib", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_any_timing.txt"))
    args = ap.parse_args()
    res = measure(args.gib, args.reps, args.tile_mib)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
