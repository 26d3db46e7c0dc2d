"""CPU-only checks of the boundary of the stream encoder whose chunks carry the window: its two entry points are declared,
exported and bound with the independent form's arguments, answer HD_E_NODEVICE where there is no device, and the primed
parse kernels of the build are kernels of their own name that use no scratch memory and hold the plain parse's budgets."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest

SYMBOLS = {"hipdeflate_stream_deflate_carry_dev": 10, "hip_deflate_stream_carry": 7}
TWINS = {"hipdeflate_stream_deflate_carry_dev": "hipdeflate_stream_deflate_dev", "hip_deflate_stream_carry": "hip_deflate_stream"}
# names the existing ABI tests select kernels by: no new kernel may fall into their counts
TAKEN = ("k_inflate_piece", "k_inflate_size", "k_inflateE", "k_inflate_lat", "k_inflate_framed", "k_compact", "k_deflate_",
         "k_parse_wg", "k_emit_wg", "k_carry_", "k_stream_")


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
        assert list(getattr(pkg.lib(), name).argtypes) == list(getattr(pkg.lib(), TWINS[name]).argtypes), name
    text = open(os.path.join(hdtest.ROOT, "7bgzf_amd", "device.py")).read()
    for name in ("deflate_stream_carry_call", "deflate_stream_carry"):
        assert re.search(r"^def %s\(" % name, text, flags=re.M), name
    assert callable(pkg.hip_deflate_stream_carry)


def test_symbols_are_declared_with_the_independent_forms_arguments():
    text = header_text()

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        return [" ".join(p.split()) for p in m.group(1).split(",")]
    for name, nargs in SYMBOLS.items():
        assert len(params(name)) == nargs, name
        assert params(name) == params(TWINS[name]), name


def test_header_states_the_form_and_its_price():
    text = " ".join(open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read().replace("*", " ").split())
    for phrase in ("min(32768, s) & ~1023", "16-byte aligned", "status 2", "hipdeflate_stream_inflate_carry_dev",
                   "exactly the bytes of hipdeflate_stream_deflate_dev"):
        assert phrase in text, phrase


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: covered by the gpu tests")
def test_without_a_device_the_calls_say_so(pkg):
    lib = pkg.lib()
    s = pkg.StreamSummary()
    buf = (ctypes.c_uint8 * 64)()
    n = ctypes.c_size_t(64)
    assert lib.hipdeflate_stream_deflate_carry_dev(None, 0, 4096, 6, pkg.FRAME_GZIP, None, 0, None, ctypes.byref(s),
                                                   None) == pkg.HD_E_NODEVICE
    assert lib.hip_deflate_stream_carry(buf, ctypes.byref(n), buf, 64, 6, pkg.FRAME_GZIP, 4096) == pkg.HD_E_NODEVICE


def test_primed_parse_kernels_hold_the_plain_parses_budgets(pkg):
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
    primed = {k: v for k, v in kernels.items() if "k_primed_wg" in k}
    plain = {k: v for k, v in kernels.items() if "k_parse_wg" in k}
    assert len(primed) == 8 and len(plain) == 8, list(kernels)
    for k, v in primed.items():
        assert not any(t in k for t in TAKEN), k
        twin = plain[k.replace("11k_primed_wg", "10k_parse_wg")]          # the same <WAYS, LAZY, BESIDE>
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        # the same LDS (BESIDE: none of its own, passed at launch), the same waves per SIMD, and the registers of the budget the
        # plain parse is held to in tests/test_abi.py: 96 beside the emit wavefronts, 128 alone
        assert v["LDS Size"] == twin["LDS Size"] and v["Occupancy"] == twin["Occupancy"], (k, v, twin)
        assert v["VGPRs"] <= (96 if k.endswith("ELi1EEEvNS_11DeflateArgsE") else 128), (k, v)
