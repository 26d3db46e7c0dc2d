"""The scratch layouts of the device-resident calls (7bgzf_amd/csrc/hd_scratch.hpp) on the CPU.

hd_api.hip takes every scratch column of the member index, the ranged reads, the stream encode, the three stream decoders, the
fold and the stream indexes from this header; a miscounted column is an out-of-bounds write by a kernel, which shows only on a
GPU.  tests/native/scratch_check.cpp includes the header alone -- plain C++, no HIP, nothing loaded into Python -- and is built
with the host compiler under AddressSanitizer + UBSan, the way tests/test_host_tables.py builds tables_check.cpp.  It states
every layout's columns a second time, as (type, element count), and for n, nq, ncand in 1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048,
2049, 65536 holds: the counting walk and the placing walk end at the same byte; every column aligned to its type over a
16-aligned base; the columns disjoint but for the stated overlay (rank over succ0 | succ1) and inside bytes(); each column as
long as stated; a pattern written through every column into a heap buffer of exactly bytes() read back intact."""
import os
import subprocess

import hdtest

SRC = os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")
NAT = os.path.join(hdtest.ROOT, "tests", "native")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")


def test_scratch_layouts_hold_for_every_size_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "scratch_check")
    p = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       ["-I" + SRC, "-o", exe, os.path.join(NAT, "scratch_check.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == 0 and "12 sizes, 360 layouts, 0 bad" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
