#!/usr/bin/env python3
"""What a preset dictionary costs and gains the batch calls, and what the table snapshot saves over replaying the history.

--mib MiB of the text set and of the FASTQ-like set stay in HBM.  The dictionary is the set's first 32 KiB, the blocks are
what follows, in blocks of 2 KiB, 8 KiB and 64 KiB.  For levels 3 and 6, after a warm-up of all three, --reps rounds of
    (s) hipdeflate_batch_deflate_dict_dev                               the history's table built once and copied (the default)
    (r) the same behind hipdeflate_test_dict_replay(1)                   every block replays the history
    (p) hipdeflate_batch_deflate_dev, HD_FRAME_RAW                       no dictionary: the time and ratio baseline
are timed with device events, ALTERNATED in one run; medians.  (s) and (r) must write the same bytes; the first members of (s)
are inflated by zlib with zdict on the host and compared.  Then the decode of (s)'s members by
hipdeflate_batch_inflate_dict_dev against hipdeflate_batch_inflate_dev on (p)'s members of the same blocks.
The supposition this file confirms or refutes (README: 0.65 us per replayed piece): a 32 KiB dictionary costs a block about
21 us of serial table turns, several times the parse of a 2 KiB block, and the snapshot takes that away.
One process; every GPU step runs under its own time limit and the first failure ends the run.

    python tools/dict_bench.py [--mib 256] [--reps 3] [--out profiles/dict_timing.txt] [--results FILE]
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

DICT = 32768


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


def measure(mib=256, reps=3, levels=(3, 6), sizes=(2 << 10, 8 << 10, 64 << 10)):
    torch = importlib.import_module("torch")
    pkg = importlib.import_module("7bgzf_amd")
    dev = importlib.import_module("7bgzf_amd.device")
    synth = importlib.import_module("7bgzf_amd.synth")
    if not pkg.available():
        raise SystemExit("no usable MI355X; there is no CPU fallback to measure")
    L = pkg.lib()
    total = mib << 20

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
    sets = {"text": lambda n: synth.text_like(n, seed=4321), "fastq": lambda n: synth.fastq_like(n, seed=1234)}
    for name, make in sets.items():
        with Step("%s: input" % name, 300):
            host = make(DICT + total)
            data = torch.from_numpy(host).cuda()
            d = data[:DICT]
            torch.cuda.synchronize()
        for level in levels:
            for size in sizes:
                n = total // size
                off = DICT + torch.arange(n, dtype=torch.int64, device="cuda") * size
                ln = torch.full((n,), size, dtype=torch.int32, device="cuda")
                slot = int(L.hipdeflate_bound(size, level))
                out = {k: torch.empty(n * slot, dtype=torch.uint8, device="cuda") for k in "sp"}
                res = {k: [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)] for k in "srp"}

                def snap():
                    dev.deflate_dict_call(data, off, ln, level, d, out["s"], slot, slot, *res["s"])

                def replay():
                    L.hipdeflate_test_dict_replay(1)
                    try:
                        dev.deflate_dict_call(data, off, ln, level, d, out["s"], slot, slot, *res["r"])
                    finally:
                        L.hipdeflate_test_dict_replay(0)

                def plain():
                    pkg._check(L.hipdeflate_batch_deflate_dev(data.data_ptr(), off.data_ptr(), ln.data_ptr(), n, level, pkg.FRAME_RAW,
                                                              out["p"].data_ptr(), slot, slot, res["p"][0].data_ptr(),
                                                              res["p"][1].data_ptr(), res["p"][2].data_ptr(),
                                                              torch.cuda.current_stream().cuda_stream), "hipdeflate_batch_deflate_dev")
                with Step("%s level %d block %d: encode" % (name, level, size), 300):
                    replay()                                                              # warm-up of all three, and the checks
                    kept = out["s"].clone()
                    snap()
                    plain()
                    torch.cuda.synchronize()
                    assert all(int(res[k][2].abs().sum()) == 0 for k in "srp")
                    assert torch.equal(res["s"][0], res["r"][0]) and torch.equal(res["s"][1], res["r"][1])
                    lens_s = res["s"][0].cpu().tolist()
                    # (the slots' bytes behind a member are not the member's: compared member by member on the first of them)
                    a, b = kept.cpu().numpy(), out["s"].cpu().numpy()
                    for i in range(min(n, 64)):
                        m = bytes(b[i * slot:i * slot + lens_s[i]])
                        assert bytes(a[i * slot:i * slot + lens_s[i]]) == m, "replay and snapshot differ in member %d" % i
                        z = zlib.decompressobj(-15, zdict=bytes(host[:DICT]))
                        assert z.decompress(m) == bytes(host[DICT + i * size:DICT + (i + 1) * size]) and z.eof
                    del kept, a, b
                    ms = {k: [] for k in "srp"}
                    for _ in range(reps):                                                 # alternated
                        ms["s"].append(timed(snap))
                        ms["r"].append(timed(replay))
                        ms["p"].append(timed(plain))
                with Step("%s level %d block %d: decode" % (name, level, size), 300):
                    moff = torch.arange(n, dtype=torch.int64, device="cuda") * slot
                    dec = torch.empty(n * size, dtype=torch.uint8, device="cuda")
                    caps = torch.full((n,), size, dtype=torch.int32, device="cuda")
                    ooff = torch.arange(n, dtype=torch.int64, device="cuda") * size
                    r = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]

                    def dec_dict():
                        dev.inflate_dict_call(out["s"], moff, res["s"][0], pkg.FRAME_RAW, d, dec, ooff, caps, r[0], r[1], None, r[2])

                    def dec_plain():
                        dev.device_inflate(out["p"], moff, res["p"][0], dec, ooff, caps, r[0], r[1], r[2])
                    dec_plain()
                    assert int(r[2].abs().sum()) == 0 and torch.equal(dec, data[DICT:DICT + n * size])
                    dec.zero_()
                    dec_dict()
                    assert int(r[2].abs().sum()) == 0 and torch.equal(dec, data[DICT:DICT + n * size])
                    assert torch.equal(r[1], res["s"][1])                                # the CRC-32 of the output alone
                    dms = {"dict": [], "plain": []}
                    for _ in range(reps):
                        dms["dict"].append(timed(dec_dict))
                        dms["plain"].append(timed(dec_plain))
                nbytes = n * size
                med = {k: median(v) for k, v in ms.items()}
                rows.append({
                    "set": name, "level": level, "block": size, "nblocks": n, "bytes": nbytes,
                    "snapshot_ms": [round(x, 3) for x in ms["s"]], "replay_ms": [round(x, 3) for x in ms["r"]],
                    "plain_ms": [round(x, 3) for x in ms["p"]],
                    "snapshot_GBps": round(nbytes / med["s"] / 1e6, 2), "replay_GBps": round(nbytes / med["r"] / 1e6, 2),
                    "plain_GBps": round(nbytes / med["p"] / 1e6, 2),
                    "dict_ratio": round(sum(lens_s) / nbytes, 5), "plain_ratio": round(int(res["p"][0].sum()) / nbytes, 5),
                    "replay_minus_snapshot_us_per_block_per_cu": round((med["r"] - med["s"]) * 1e3 / max(1.0, n / 256.0), 3),
                    "decode_dict_ms": [round(x, 3) for x in dms["dict"]], "decode_plain_ms": [round(x, 3) for x in dms["plain"]],
                    "decode_dict_GBps": round(nbytes / median(dms["dict"]) / 1e6, 2),
                    "decode_plain_GBps": round(nbytes / median(dms["plain"]) / 1e6, 2),
                })
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                del out, res, dec
                torch.cuda.empty_cache()
        del data, d
        torch.cuda.empty_cache()
    assert L.hipdeflate_stall_count() == 0
    return {"rows": rows}


def report(res):
    lines = ["preset dictionary, batch calls -- tools/dict_bench.py",
             "32 KiB dictionary in front of the blocks; device events, alternated, medians; GB/s of input (encode) / output (decode)",
             "(s) table snapshot | (r) forced replay | (p) plain call without a dictionary; ratio = member bytes / input bytes", ""]
    for r in res["rows"]:
        lines.append("%-5s level %d block %6d  %d blocks" % (r["set"], r["level"], r["block"], r["nblocks"]))
        for k, tag in (("snapshot", "(s)"), ("replay", "(r)"), ("plain", "(p)")):
            lines.append("    %s ms %s -> %.2f GB/s%s" % (tag, " ".join("%.3f" % x for x in r[k + "_ms"]), r[k + "_GBps"],
                                                         "  ratio %.5f" % r["plain_ratio" if k == "plain" else "dict_ratio"]))
        lines.append("    (r) - (s) = %.3f us per block and CU (256 CUs, one workgroup each);  (s)/(p) time %.3f  bytes %.4f" % (
            r["replay_minus_snapshot_us_per_block_per_cu"], r["plain_GBps"] / r["snapshot_GBps"], r["dict_ratio"] / r["plain_ratio"]))
        lines.append("    decode: dictionary %s ms -> %.2f GB/s | plain members %s ms -> %.2f GB/s" % (
            " ".join("%.3f" % x for x in r["decode_dict_ms"]), r["decode_dict_GBps"],
            " ".join("%.3f" % x for x in r["decode_plain_ms"]), r["decode_plain_GBps"]))
    lines.append("")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_timing.txt"))
    ap.add_argument("--results", default=None, help="this tool's JSON line of an earlier run: write the report from it, measure nothing")
    args = ap.parse_args()
    if args.results:
        res = json.loads(open(args.results).read().strip().splitlines()[-1])
    else:
        res = measure(args.mib, args.reps)
    with open(args.out, "w") as f:
        f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
