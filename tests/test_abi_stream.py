"""CPU-only checks of the single-stream path's boundary: its entry points are declared, exported and bound, the summary
has the layout the header gives it, HD_STREAM_WINDOW_BYTES agrees between header and package, and none of the k_stream_* /
k_check_combine / k_chunk_adler kernels of the build uses scratch memory."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest

SYMBOLS = {"hipdeflate_stream_bound": 4, "hipdeflate_stream_deflate_dev": 10, "hipdeflate_stream_inflate_dev": 11,
           "hipdeflate_check_combine_dev": 6, "hip_deflate_stream": 7}


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def header_text():
    return open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()


def test_symbols_are_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name, nargs in SYMBOLS.items():
        assert name in exported, name
        assert name in pkg.EXPORTS, name
        assert len(getattr(pkg.lib(), name).argtypes) == nargs, name
    assert "hipdeflate_test_stream_window" in exported and "hipdeflate_test_stream_window" in pkg.EXPORTS
    assert pkg.lib().hipdeflate_stream_bound.restype is ctypes.c_uint64


def test_symbols_are_declared_in_the_header():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\buint64_t\s+hipdeflate_stream_bound\s*\(", text)
    for name in ("hipdeflate_stream_deflate_dev", "hipdeflate_stream_inflate_dev", "hipdeflate_check_combine_dev",
                 "hip_deflate_stream"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"\bvoid\s+hipdeflate_test_stream_window\s*\(\s*uint32_t", text)
    assert "hipdeflate_stream_summary" in text


def test_summary_layout_and_constants(pkg):
    s = pkg.StreamSummary
    assert ctypes.sizeof(s) == 40
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("out_bytes", 0), ("in_bytes", 8), ("bad_chunk", 16), ("nchunks", 24), ("check", 28), ("status", 32)]
    params = open(os.path.join(hdtest.ROOT, "include", "hipdeflate_params.h")).read()
    m = re.search(r"#define\s+HD_STREAM_WINDOW_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", params)
    assert m and int(m.group(1)) << int(m.group(2)) == pkg.STREAM_WINDOW_BYTES == 1 << 30
    assert (pkg.CHECK_CRC32, pkg.CHECK_ADLER32) == (0, 1)


def test_stream_bound_needs_no_device(pkg):
    """the bound is host arithmetic: header + the worst case of every chunk + 03 00 + trailer"""
    L = pkg.lib()
    for frame, ends in ((pkg.FRAME_RAW, 2), (pkg.FRAME_ZLIB, 8), (pkg.FRAME_GZIP, 20)):
        assert L.hipdeflate_stream_bound(0, 4096, 6, frame) == ends
        # stored blocks of at most 65535 bytes, 5 bytes each, and the flush suffix
        assert L.hipdeflate_stream_bound(3 * 4096 + 1, 4096, 6, frame) == ends + 3 * (4096 + 10) + (1 + 10)
    assert L.hipdeflate_stream_bound(100, 24, 6, pkg.FRAME_RAW) == 0           # not a multiple of 16
    assert L.hipdeflate_stream_bound(100, (64 << 20) + 16, 6, pkg.FRAME_RAW) == 0


def test_stream_kernels_use_no_scratch(pkg):
    log = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "hd_api.resources.log")
    assert os.path.exists(log), "build with make -C 7bgzf_amd/csrc"
    kernels, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    ours = {k: v for k, v in kernels.items() if "k_stream_" in k or "k_check_combine" in k or "k_chunk_adler" in k}
    for name in ("k_stream_table", "k_stream_ends", "k_stream_check_table", "k_stream_trailer", "k_check_combine",
                 "k_chunk_adler"):
        assert any(name in k for k in ours), (name, list(ours))
    for k, v in ours.items():
        assert v["ScratchSize"] == 0, (k, v)
