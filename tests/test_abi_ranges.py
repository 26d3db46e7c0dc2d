"""CPU-only checks of the ranged read's boundary: hipdeflate_read_ranges_dev is declared, exported and bound, its summary
has the layout the header gives it, and none of the k_range_* kernels of the build uses scratch memory."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def header_text():
    return open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()


def test_symbol_is_exported(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert "hipdeflate_read_ranges_dev" in exported
    assert "hipdeflate_read_ranges_dev" in pkg.EXPORTS
    assert len(pkg.lib().hipdeflate_read_ranges_dev.argtypes) == 18


def test_symbol_is_declared_in_the_header():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+hipdeflate_read_ranges_dev\s*\(", text)
    assert re.search(r"#define\s+HD_RANGE_BYTES\s+0\b", text) and re.search(r"#define\s+HD_RANGE_VOFFSET\s+1\b", text)
    assert "hipdeflate_range_summary" in text


def test_summary_layout_and_constants(pkg):
    s = pkg.RangeSummary
    assert ctypes.sizeof(s) == 48
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("out_bytes", 0), ("nselected", 8), ("sel_bytes", 16), ("nrefused", 24), ("bad_member", 32), ("status", 40)]
    assert (pkg.RANGE_BYTES, pkg.RANGE_VOFFSET) == (0, 1)
    params = open(os.path.join(hdtest.ROOT, "include", "hipdeflate_params.h")).read()
    m = re.search(r"#define\s+HD_RANGE_PIECE\s+\((\d+)u\s*<<\s*(\d+)\)", params)
    assert m and int(m.group(1)) << int(m.group(2)) == pkg.RANGE_PIECE
    # HIPDEFLATE_VOFFSET: coffset << 16 | the low 16 bits of uoffset
    assert pkg.voffset(0x123456789, 0xfedc) == 0x123456789fedc and pkg.voffset(1, 0x10000) == 0x10000


def test_range_kernels_use_no_scratch(pkg):
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
    ranged = {k: v for k, v in kernels.items() if "k_range_" in k}
    for name in ("k_range_resolve", "k_range_tables", "k_range_gather"):
        assert any(name in k for k in ranged), (name, list(ranged))
    for k, v in ranged.items():
        assert v["ScratchSize"] == 0, (k, v)
