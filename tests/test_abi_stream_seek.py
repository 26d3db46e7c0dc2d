"""CPU-only checks of the seek index's boundary: its two entry points are declared, exported and bound, answer HD_E_NODEVICE
where there is no device, and the k_seek_* kernels of the build use no scratch memory and no LDS and fall into no count of the
existing ABI tests."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest
from test_abi_stream_carry import TAKEN, header_text, resource_log

SYMBOLS = {"hipdeflate_stream_windows_dev": 12, "hipdeflate_stream_read_ranges_dev": 24}
KERNELS = ("k_seek_check_out", "k_seek_windows", "k_seek_check_win", "k_seek_tables", "k_seek_resolve", "k_seek_check_crc")


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def test_symbols_are_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name, nargs in SYMBOLS.items():
        assert name in exported, name
        assert name in pkg.EXPORTS, name
        assert len(getattr(pkg.lib(), name).argtypes) == nargs, name
    text = open(os.path.join(hdtest.ROOT, "7bgzf_amd", "device.py")).read()
    for name in ("def stream_windows_call(", "def stream_read_ranges_call(", "class SeekIndex", "def build(", "def read_ranges(",
                 "def read(", "def save(", "def load("):
        assert name in text, name
    assert (pkg.ROWS_BYTES, pkg.ROWS_BITS) == (0, 1)
    assert ctypes.sizeof(pkg.WindowSummary) == 24


def test_symbols_are_declared_with_as_many_arguments():
    text = header_text()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    assert re.search(r"#define\s+HD_ROWS_BYTES\s+0\b", text) and re.search(r"#define\s+HD_ROWS_BITS\s+1\b", text)
    m = re.search(r"typedef struct hipdeflate_window_summary \{(.*?)\}", text, flags=re.S)
    assert m and re.findall(r"(\w+);", m.group(1)) == ["win_bytes", "bad_row", "status"]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: covered by the gpu tests")
def test_without_a_device_the_calls_say_so(pkg):
    lib = pkg.lib()
    w, s = pkg.WindowSummary(), pkg.RangeSummary()
    assert lib.hipdeflate_stream_windows_dev(None, 0, None, None, None, 0, None, None, 0, None, ctypes.byref(w), None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_stream_read_ranges_dev(None, 0, pkg.FRAME_RAW, pkg.ROWS_BITS, None, None, None, None, None, None, None, 0, None, 0,
                                                 None, None, 0, None, 0, None, None, None, ctypes.byref(s), None) == pkg.HD_E_NODEVICE


def test_seek_kernels_use_no_scratch_and_no_lds(pkg):
    kernels = resource_log(pkg)
    for name in KERNELS:
        ours = {k: v for k, v in kernels.items() if name in k}
        assert len(ours) == 1, (name, list(kernels))
        for k, v in ours.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["LDS Size"] == 0, (k, v)
    seek = [k for k in kernels if "k_seek_" in k]
    assert len(seek) == len(KERNELS), seek
    for k in seek:
        assert not any(t in k for t in TAKEN) and "k_carry_" not in k and "k_blocks_" not in k and "k_range_" not in k, k
    (res,) = [v for k, v in kernels.items() if "k_seek_resolve" in k]
    assert res["VGPRs"] <= 64, res                                                       # eight wavefronts a SIMD
