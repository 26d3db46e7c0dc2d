"""The host layer's two metadata tables (7bgzf_amd/csrc/hd_tables.hpp: EncTable, DecTable) on the CPU.

hd_api.hip carves every per-block table of the batch calls, the pipes, the latency contexts and the per-call inflate batcher
out of one raw buffer through this header; an off-by-one in it used to show only on a GPU.  tests/native/tables_check.cpp
includes the header alone -- plain C++, no HIP, nothing loaded into Python -- and is built with the host compiler under
AddressSanitizer + UBSan, the way tests/test_sanitize_hosts.py builds the container readers.  For n in 1, 2, 3, 5, 64, 65, 1024,
65536 it holds: every u64 column 8-aligned over an aligned base; the columns back to back, disjoint and ending at bytes(n);
the "inputs" and "results" copy ranges exactly their columns; a pattern written through every accessor into a heap buffer of
exactly bytes(n) read back intact."""
import os
import subprocess

import hdtest

SRC = os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")
NAT = os.path.join(hdtest.ROOT, "tests", "native")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")


def test_table_layouts_hold_for_every_n_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tables_check")
    p = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       ["-I" + SRC, "-o", exe, os.path.join(NAT, "tables_check.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert p.returncode == 0 and "8 sizes, 0 bad" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
