#!/usr/bin/env python3
"""What the gather costs the level-1 encode kernel it runs beside, on the headline shapes (bench.py's data,
block table and two-buffer scheme), one GPU.  HIP events around the encode kernel and around the gather, three
legs in one process, each after its own warm-up:

  1. encode passes back to back, no scan and no gather anywhere;
  2. bench.py's pipeline: scan and gather of pass k on a second stream beside the encode kernel of pass k + 1;
  3. the gather alone, on an idle chip.

Legs 1 and 2 both run warm and differ in the side stream's work only, so encode_beside - encode_alone is what
the gather (and the 0.1 ms of scan) takes from the encoder.  pipeline_ms_per_step is leg 2 by the wall clock, the
last gather drained inside it, as bench.py times its steps: if it is not encode_beside plus a twentieth of a
gather, the two streams did not run beside each other.  One JSON line:

  python tools/gather_beside.py [--steps 10] [--warmup 2] [--level 1] [--gib 16] [--data fastq|text|random] [--lib FILE]

--lib: another build of the library than the package's own (parent against new from one checkout).  The grid the library
chose for the gathers of legs 2 and 3 (hipdeflate_test_compact_grid, where the build has it) is on the line as
gather_beside_grid / gather_alone_grid; HIPDEFLATE_GATHER_GRID=full|beside in the environment forces either, which is how
the rows of a sweep over HD_COMPACT_BESIDE_WAVES_PER_2CU are made: one build per value, run under `beside`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the headline's own data and block table)


def stats(ms):
    return {"avg": round(sum(ms) / len(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "n": len(ms)}


def setup(gib=16.0, tile_mib=64, first_record=0, data_kind="fastq", lib=None):
    """-> (Bench, data, off, ln, encs, packs): what bench.py's encode() sets up before its timed region"""
    args = argparse.Namespace(gpus=1, gib=gib, tile_mib=tile_mib, first_record=first_record)
    if lib:
        import importlib
        importlib.import_module("7bgzf_amd").LIB_PATH = os.path.abspath(lib)       # before the first lib()
    B = bench.Bench(args)
    _, data, _ = B.make_data(data_kind, bench.BGZF_BLOCK, whole_blocks=False)
    off, ln = B.dev.block_table(data.numel(), bench.BGZF_BLOCK)
    nb = off.numel()
    encs = [B.dev.DeviceDeflate(nb, slot=65536) for _ in range(2)]
    span = int(data.numel() * 1.01) + (1 << 20)
    packs = [B.torch.empty(span, dtype=B.torch.uint8, device="cuda") for _ in range(2)]
    # The second stream is the process's first, as bench.py's is, and stays the same for every call of measure(): the
    # runtime deals streams out over a few hardware queues in turn, and a side stream that lands on the main stream's
    # queue runs the gather BEHIND the encode kernel instead of beside it (both then show their stand-alone times and
    # the step takes the sum of the two)
    B.side = B.torch.cuda.Stream()
    return B, data, off, ln, encs, packs


def last_grid(B):
    """the grid of the library's last gather launch (None: a build without the hook)"""
    f = getattr(B.pkg.lib(), "hipdeflate_test_compact_grid", None)
    return int(f()) & 0xffffffff if f is not None else None


def pipeline(torch, main, side, encs, packs, encode, after_gather=None):
    """bench.py's software pipeline over two buffer sets -> (step, drain): step(keep_e, keep_g) queues the encode of the
    next pass on `main` (encode(i) fills encs[i]) and then, on `side`, scan and gather of the pass before it into packs[i];
    drain(keep_g) gathers the last pass, which has no encoder beside it.  The lists receive the event pairs round the
    encode and round the gather; after_gather(i) is called right behind every gather's launch."""
    coded = [torch.cuda.Event(), torch.cuda.Event()]
    gathered = [torch.cuda.Event(), torch.cuda.Event()]
    state = {"k": 0, "pending": None}

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def gather(i, keep):
        with torch.cuda.stream(side):
            side.wait_event(coded[i])
            encs[i].scan()
            g0, g1 = ev(), ev()
            g0.record(side)
            encs[i].compact(packs[i])
            g1.record(side)
            gathered[i].record(side)
        if after_gather is not None:
            after_gather(i)
        keep.append((g0, g1))

    def step(keep_e, keep_g):
        i = state["k"] & 1
        state["k"] += 1
        e0, e1 = ev(), ev()
        main.wait_event(gathered[i])
        e0.record()
        encode(i)
        e1.record()
        coded[i].record(main)
        if state["pending"] is not None:
            gather(state["pending"], keep_g)
        state["pending"] = i
        keep_e.append((e0, e1))

    def drain(keep_g):
        if state["pending"] is not None:
            gather(state["pending"], keep_g)
            state["pending"] = None
        main.wait_stream(side)

    return step, drain


def measure(B, data, off, ln, encs, packs, steps=10, warmup=2, level=1):
    torch, frame = B.torch, B.pkg.FRAME_BGZF
    main, side = torch.cuda.current_stream(), B.side

    def ev():
        return torch.cuda.Event(enable_timing=True)

    # ---- leg 1: encode alone ----------------------------------------------------------------------------------
    def encode_alone(n, keep):
        for k in range(n):
            e0, e1 = ev(), ev()
            e0.record()
            encs[k & 1].run(data, off, ln, level=level, frame=frame)
            e1.record()
            keep.append((e0, e1))
    encode_alone(warmup, [])
    torch.cuda.synchronize()
    alone = []
    encode_alone(steps, alone)
    torch.cuda.synchronize()
    enc_alone = [a.elapsed_time(b) for a, b in alone]

    # ---- leg 2: bench.py's pipeline ---------------------------------------------------------------------------
    step, drain = pipeline(torch, main, side, encs, packs,
                           lambda i: encs[i].run(data, off, ln, level=level, frame=frame))

    for _ in range(warmup):
        step([], [])
    drain([])
    torch.cuda.synchronize()
    be, bg = [], []
    t0 = time.perf_counter()
    for _ in range(steps):
        step(be, bg)
    grid_beside = last_grid(B)
    lone = []
    drain(lone)                                  # the last gather has no encoder beside it: kept out of the figure
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / steps     # what bench.py calls ms_per_step (the drain inside)
    # the first timed encode has no gather beside it (nothing pending after the drain): kept out too
    enc_beside = [a.elapsed_time(b) for a, b in be[1:]]
    gat_beside = [a.elapsed_time(b) for a, b in bg]

    # ---- leg 3: the gather alone ------------------------------------------------------------------------------
    encs[0].scan()
    for _ in range(warmup):
        encs[0].compact(packs[0])
    torch.cuda.synchronize()
    ga = []
    for _ in range(steps):
        g0, g1 = ev(), ev()
        g0.record()
        encs[0].compact(packs[0])
        g1.record()
        ga.append((g0, g1))
    torch.cuda.synchronize()
    gat_alone = [a.elapsed_time(b) for a, b in ga]
    grid_alone = last_grid(B)

    assert int(encs[0].status.abs().sum()) == 0 and int(encs[1].status.abs().sum()) == 0
    comp = int(encs[0].total.item())
    res = {"encode_alone_ms": stats(enc_alone), "encode_beside_ms": stats(enc_beside),
           "gather_alone_ms": stats(gat_alone), "gather_beside_ms": stats(gat_beside),
           "encode_beside_minus_alone_ms": round(stats(enc_beside)["avg"] - stats(enc_alone)["avg"], 3),
           "pipeline_ms_per_step": round(wall_ms, 3),
           "gather_beside_grid": grid_beside, "gather_alone_grid": grid_alone,
           "gather_grid_env": os.environ.get("HIPDEFLATE_GATHER_GRID", ""),
           "gather_alone_GBps_copied": round(comp / (stats(gat_alone)["avg"] * 1e-3) / 1e9, 1),
           "members": int(off.numel()), "input_bytes": int(data.numel()), "gathered_bytes": comp,
           "level": level, "steps": steps, "warmup": warmup}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--data", default="fastq", choices=["fastq", "text", "random"])
    ap.add_argument("--lib", default=None, help="another build of libhipdeflate.so than the package's own")
    a = ap.parse_args()
    B, data, off, ln, encs, packs = setup(gib=a.gib, data_kind=a.data, lib=a.lib)
    res = measure(B, data, off, ln, encs, packs, a.steps, a.warmup, a.level)
    res["data"] = a.data
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
