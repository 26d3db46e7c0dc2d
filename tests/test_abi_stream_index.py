"""CPU-only checks of the stream index's boundary: its three entry points are declared, exported and bound, the summary has
the layout the header gives it, and k_inflate_piece and the new passes of the build use no scratch memory."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest

SYMBOLS = {"hipdeflate_stream_index_dev": 11, "hipdeflate_stream_inflate_table_dev": 12, "hip_inflate_stream": 6}
KERNELS = ("k_inflate_piece", "k_stream_flag", "k_stream_write", "k_stream_links", "k_stream_rows", "k_stream_verdict",
           "k_stream_check_rows")


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def header_text():
    text = open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name, nargs in SYMBOLS.items():
        assert name in exported, name
        assert name in pkg.EXPORTS, name
        assert len(getattr(pkg.lib(), name).argtypes) == nargs, name


def test_symbols_are_declared_with_as_many_arguments():
    text = header_text()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))


def test_summary_layout(pkg):
    s = pkg.StreamIndexSummary
    assert ctypes.sizeof(s) == 40
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("nchunks", 0), ("out_bytes", 8), ("end_offset", 16), ("ncandidates", 24), ("hdr_bytes", 32), ("status", 36)]
    m = re.search(r"typedef struct hipdeflate_stream_index_summary \{(.*?)\} hipdeflate_stream_index_summary;", header_text(), flags=re.S)
    assert m
    fields = re.findall(r"\b(uint64_t|uint32_t)\s+(\w+)\s*;", m.group(1))
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    assert [(n, ctype[t]) for t, n in fields] == list(s._fields_)


def test_new_kernels_use_no_scratch(pkg):
    log = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "hd_api.resources.log")
    assert os.path.exists(log), "build with make -C 7bgzf_amd/csrc"
    kernels, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    for name in KERNELS:
        ours = {k: v for k, v in kernels.items() if name in k}
        assert ours, (name, list(kernels))
        for k, v in ours.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    # the piece decoder is the size pass again: the same LDS, and with it the same wavefronts per CU
    (piece,) = [v for k, v in kernels.items() if "k_inflate_piece" in k]
    (size,) = [v for k, v in kernels.items() if "k_inflate_size" in k]
    assert piece["LDS Size"] == size["LDS Size"] and piece["Occupancy"] == size["Occupancy"]
