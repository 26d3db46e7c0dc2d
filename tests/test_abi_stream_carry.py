"""CPU-only checks of the carry decode's boundary: its four entry points are declared, exported and bound, answer
HD_E_NODEVICE where there is no device, and the k_carry_* kernels of the build use no scratch memory and stay inside a CU's
LDS."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest

SYMBOLS = {"hipdeflate_stream_index_carry_dev": 12, "hipdeflate_stream_inflate_carry_dev": 13, "hip_inflate_stream_carry": 6,
           "hipdeflate_test_carry_group": 1, "hipdeflate_test_carry_times": 1}
KERNELS = ("k_carry_piece", "k_carry_reach_rows", "k_carry_check_reach", "k_carry_cut", "k_carry_group", "k_carry_decode",
           "k_carry_tails", "k_carry_resolve", "k_carry_verify", "k_carry_parts", "k_carry_crc")
# names the existing ABI tests select kernels by: no new kernel may fall into their counts
TAKEN = ("k_inflate_piece", "k_inflate_size", "k_inflateE", "k_inflate_lat", "k_inflate_framed", "k_compact", "k_deflate_",
         "k_parse_wg", "k_emit_wg")


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def header_text():
    text = open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def resource_log(pkg):
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
    return kernels


def test_symbols_are_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name, nargs in SYMBOLS.items():
        assert name in exported, name
        assert name in pkg.EXPORTS, name
        assert len(getattr(pkg.lib(), name).argtypes) == nargs, name
    for name in ("index_stream_carry_call", "index_stream_carry", "inflate_stream_carry_call", "inflate_stream_carry"):
        assert name in open(os.path.join(hdtest.ROOT, "7bgzf_amd", "device.py")).read(), name
    assert callable(pkg.hip_inflate_stream_carry)


def test_symbols_are_declared_with_as_many_arguments():
    text = header_text()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    params = open(os.path.join(hdtest.ROOT, "include", "hipdeflate_params.h")).read()
    assert re.search(r"#define\s+HD_CARRY_GROUP_BYTES\s+\(256u << 20\)", params)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: covered by the gpu tests")
def test_without_a_device_the_calls_say_so(pkg):
    lib = pkg.lib()
    s, x = pkg.StreamSummary(), pkg.StreamIndexSummary()
    buf = (ctypes.c_uint8 * 64)()
    n = ctypes.c_size_t(64)
    assert lib.hipdeflate_stream_index_carry_dev(None, 0, pkg.FRAME_RAW, 0, 0, None, None, None, None, None, ctypes.byref(x),
                                                 None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_stream_inflate_carry_dev(None, 0, pkg.FRAME_RAW, None, None, None, None, None, 0, None, 0,
                                                   ctypes.byref(s), None) == pkg.HD_E_NODEVICE
    assert lib.hip_inflate_stream_carry(buf, ctypes.byref(n), buf, 64, pkg.FRAME_RAW, None) == pkg.HD_E_NODEVICE
    lib.hipdeflate_test_carry_group(4096)
    lib.hipdeflate_test_carry_group(0)


def test_carry_kernels_use_no_scratch_and_fit_a_cu(pkg):
    kernels = resource_log(pkg)
    for name in KERNELS:
        ours = {k: v for k, v in kernels.items() if name in k}
        assert len(ours) == 1, (name, list(kernels))
        for k, v in ours.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    carry = [k for k in kernels if "k_carry_" in k]
    assert len(carry) == len(KERNELS), carry
    for k in carry:
        assert not any(t in k for t in TAKEN), k
    (tails,) = [v for k, v in kernels.items() if "k_carry_tails" in k]
    assert tails["LDS Size"] <= 160 * 1024 and tails["VGPRs"] <= 128, tails          # one workgroup of sixteen wavefronts
    (dec,) = [v for k, v in kernels.items() if "k_carry_decode" in k]
    assert dec["LDS Size"] <= 80 * 1024, dec                                          # two rows per CU at the least
    # the carried piece decoder is the piece decoder again: the same LDS
    (piece,) = [v for k, v in kernels.items() if "k_inflate_pieceE" in k]
    (cpiece,) = [v for k, v in kernels.items() if "k_carry_pieceE" in k]
    assert cpiece["LDS Size"] == piece["LDS Size"] and cpiece["VGPRs"] <= 64
