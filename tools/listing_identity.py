#!/usr/bin/env python3
"""Which kernels of two builds are the same instructions: the device listings (7bgzf_amd/csrc/hd_api.device.s, `make -C
7bgzf_amd/csrc hd_api.device.s`) of a parent checkout and of this tree, compared kernel by kernel.  Needs no GPU.

A kernel's text is what stands between its label and its end label, comments dropped; what the compiler numbers per file --
basic-block labels, temporary labels, the ids of labels inside asm statements -- is renumbered per kernel, so that a kernel
counts as changed only where an instruction, an operand or their order changed.

    python tools/listing_identity.py PARENT.device.s NEW.device.s [--must-match REGEX] [--out FILE]

Exit status 1 if a kernel that --must-match names differs or is gone.
"""
import argparse
import re
import sys


def kernels(path):
    out, name, buf, ids = {}, None, [], {}
    for line in open(path):
        m = re.match(r"^(_ZN2hd\w+):", line)
        if m and name is None:
            name, buf, ids = m.group(1), [], {}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = buf
            name = None
            continue
        t = line.split(";")[0].rstrip()
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"\.Ltmp\d+", ".Ltmp", t)
        t = re.sub(r"(Lhd_\w+?_)(\d+)\b", lambda m: m.group(1) + str(ids.setdefault(m.group(2), len(ids))), t)
        if t.strip():
            buf.append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--must-match", default=None, help="kernels (mangled names, a regular expression) that have to be identical")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a, b = kernels(args.parent), kernels(args.new)
    must = re.compile(args.must_match) if args.must_match else None
    lines, bad = [], 0
    for k in sorted(a):
        held = bool(must and must.search(k))
        if k not in b:
            verdict = "GONE"
        elif a[k] == b[k]:
            verdict = "same"
        else:
            verdict = "DIFFERS"
        bad += held and verdict != "same"
        lines.append("%-8s%s %6d lines  %s" % (verdict, "*" if held else " ", len(a[k]), k))
    new = [k for k in sorted(b) if k not in a]
    lines += ["new       %6d lines  %s" % (len(b[k]), k) for k in new]
    same = sum(1 for k in a if k in b and a[k] == b[k])
    lines.append("")
    lines.append("%d kernels of the parent: %d the same instructions, %d different, %d gone; %d new%s" % (
        len(a), same, sum(1 for k in a if k in b and a[k] != b[k]), sum(1 for k in a if k not in b), len(new),
        "" if not must else "; of the %d held (*) %d differ" % (sum(1 for k in a if must.search(k)), bad)))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
