"""CPU-only checks of the boundary of the preset-dictionary calls: the five entry points are declared, exported and bound, the
device calls take the plain calls' arguments with (dict, dict_len) behind level / frame, they answer HD_E_NODEVICE where there
is no device, the header states the rounding, the two limits and the DICTID rule, and the new kernels of the build are kernels
of their own name that use no scratch memory and hold the budgets of the kernels they are made from."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest

# name -> (the plain call it follows, the index at which `dict, dict_len` stand, the plain call's argument left out there)
SYMBOLS = {
    "hipdeflate_batch_deflate_dict_dev": ("hipdeflate_batch_deflate_dev", 5, "int frame"),
    "hipdeflate_batch_inflate_dict_dev": ("hipdeflate_batch_inflate_framed_dev", 5, None),
    "hipdeflate_batch_deflate_dict": ("hipdeflate_batch_deflate", 5, "int frame"),
    "hipdeflate_batch_inflate_dict": ("hipdeflate_batch_inflate_framed", 5, None),
}
# names the existing ABI tests select kernels by: no new kernel may fall into their counts
TAKEN = ("k_inflate_piece", "k_inflate_size", "k_inflateE", "k_inflate_lat", "k_inflate_framed", "k_compact", "k_deflate_",
         "k_parse_wg", "k_primed_wg", "k_emit_wg", "k_carry_", "k_stream_")


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    if not os.path.exists(p.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")], check=True)
    return p


def header_text():
    text = open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def params(text, name):
    m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_are_exported_and_bound(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name, (twin, at, dropped) in SYMBOLS.items():
        assert name in exported and name in pkg.EXPORTS, name
        have, plain = list(getattr(pkg.lib(), name).argtypes), list(getattr(pkg.lib(), twin).argtypes)
        if dropped:
            plain = plain[:at] + plain[at + 1:]
        assert have == plain[:at] + [ctypes.c_void_p, ctypes.c_uint32] + plain[at:], name
    assert "hipdeflate_test_dict_replay" in exported and "hipdeflate_test_dict_replay" in pkg.EXPORTS
    assert list(pkg.lib().hipdeflate_test_dict_replay.argtypes) == [ctypes.c_int]
    text = open(os.path.join(hdtest.ROOT, "7bgzf_amd", "device.py")).read()
    for name in ("deflate_dict_call", "inflate_dict_call", "deflate_dict", "inflate_dict"):
        assert re.search(r"^def %s\(" % name, text, flags=re.M), name
    assert callable(pkg.batch_deflate_dict) and callable(pkg.batch_inflate_dict)


def test_symbols_are_declared_with_the_plain_calls_arguments_and_the_dictionary():
    text = header_text()
    for name, (twin, at, dropped) in SYMBOLS.items():
        plain = params(text, twin)
        if dropped:
            assert plain[at] == dropped, (name, plain[at])
            plain = plain[:at] + plain[at + 1:]
        const = "const void" if name.endswith("_dev") else "const uint8_t"
        assert params(text, name) == plain[:at] + ["%s *dict" % const, "uint32_t dict_len"] + plain[at:], name
    assert params(text, "hipdeflate_test_dict_replay") == ["int on"]


def test_header_states_the_rounding_the_limits_and_the_dictid_rule():
    text = " ".join(open(os.path.join(hdtest.ROOT, "include", "hipdeflate.h")).read().replace("*", " ").split())
    for phrase in ("used = min(32768, dict_len) & ~1023", "SHORTER THAN 1024 BYTES is accepted and NOT USED",
                   "UP TO 1023 BYTES AT THE FRONT", "Adler-32 of the WHOLE dictionary as given, all dict_len bytes",
                   "d <= p + D", "A member WITHOUT FDICT is decoded without the dictionary", "in_used counts the six header bytes",
                   "deflateSetDictionary (lib/zlib/deflate.c:", "inflateSetDictionary (lib/zlib/inflate.c:",
                   "dict == NULL with dict_len != 0 is HD_E_ARG", "keeps refusing FDICT"):
        assert phrase in text, phrase


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: covered by the gpu tests")
def test_without_a_device_the_calls_say_so(pkg):
    lib = pkg.lib()
    buf = (ctypes.c_uint8 * 64)()
    assert lib.hipdeflate_batch_deflate_dict_dev(None, None, None, 0, 6, None, 0, None, 0, 0, None, None, None, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_batch_deflate_dict_dev(None, None, None, 0, 6, None, 64, None, 0, 0, None, None, None, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_batch_inflate_dict_dev(None, None, None, 0, pkg.FRAME_RAW, None, 0, None, None, None, None, None, None,
                                                 None, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_batch_deflate_dict(buf, None, None, 0, 6, buf, 64, buf, 64, 64, None, None, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_batch_inflate_dict(buf, None, None, 0, pkg.FRAME_ZLIB, buf, 64, buf, None, None, None, None, None,
                                             None) == pkg.HD_E_NODEVICE
    lib.hipdeflate_test_dict_replay(1)
    lib.hipdeflate_test_dict_replay(0)


def kernel_resources(pkg):
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


def test_dictionary_kernels_hold_their_budgets(pkg):
    kernels = kernel_resources(pkg)
    new = {k: v for k, v in kernels.items() if "k_dict_" in k}
    parse = {k: v for k, v in new.items() if "9k_dict_wgI" in k}
    table = {k: v for k, v in new.items() if "12k_dict_tableI" in k}
    inflate = {k: v for k, v in new.items() if "14k_dict_inflateE" in k}
    opened = {k: v for k, v in new.items() if "11k_dict_openE" in k}
    assert (len(parse), len(table), len(inflate), len(opened), len(new)) == (4, 3, 1, 1, 9), list(new)
    for k, v in new.items():
        assert not any(t in k for t in TAKEN), k
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["SGPRs Spill"] == 0 or k in inflate, (k, v)
    # the dictionary parse: its plain twin's LDS and waves per SIMD -- one workgroup a CU -- and the registers of the budget the
    # plain parse is held to alone (tests/test_abi.py: 128; it never runs beside the emit wavefronts)
    for k, v in parse.items():
        twin = kernels[k.replace("9k_dict_wgI", "10k_parse_wgI").replace("EEEvNS_11DeflateArgsENS_6WgDictE", "ELi0EEEvNS_11DeflateArgsE")]
        assert v["LDS Size"] == twin["LDS Size"] and v["Occupancy"] == twin["Occupancy"] and v["VGPRs"] <= 128, (k, v, twin)
    for k, v in table.items():
        assert v["LDS Size"] == 131200 and v["Occupancy"] == 4 and v["VGPRs"] <= 128, (k, v)
    # the dictionary decoder: k_inflate_framed's line in tests/test_abi.py
    (v,) = inflate.values()
    framed = kernels["_ZN2hd16k_inflate_framedENS_17InflateFramedArgsE"]
    assert v["VGPRs"] <= 80 and v["LDS Size"] <= 6400 and v["Occupancy"] >= framed["Occupancy"], (v, framed)
    # (inflate_stream keeps its reader and positions in scalar registers and parks some of them in lanes of vector registers, never
    # in memory: 79 in k_inflate_framed.  The dictionary adds three uniform values -- a 64-bit address and the lowest position)
    assert v["SGPRs Spill"] <= framed["SGPRs Spill"] + 4, (v, framed)
