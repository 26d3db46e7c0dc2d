"""CPU-only checks of the block index's boundary: its entry points are declared, exported and bound, answer HD_E_NODEVICE
where there is no device, and the k_blocks_* kernels of the build use no scratch memory, the piece kernel stays within four
LDS allocation units and the decode instantiation within the LDS of the existing one."""
import ctypes
import os
import re
import subprocess

import pytest

import hdtest
from test_abi_stream_carry import TAKEN, header_text, resource_log

SYMBOLS = {"hipdeflate_stream_index_blocks_dev": 13, "hipdeflate_stream_inflate_blocks_dev": 13, "hip_inflate_stream_blocks": 6,
           "hipdeflate_test_block_headers_dev": 6, "hipdeflate_test_blocks_times": 1, "hipdeflate_test_blocks_counts": 1,
           "hipdeflate_test_block_candidates_dev": 7}
KERNELS = ("k_blocks_rule", "k_blocks_flag", "k_blocks_write", "k_blocks_count", "k_blocks_piece", "k_blocks_links", "k_blocks_sizes", "k_blocks_starts",
           "k_blocks_heads", "k_blocks_rowsE", "k_blocks_reach", "k_blocks_verdict", "k_blocks_check_rows", "k_blocks_decode")


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
    for name in ("index_stream_blocks_call", "index_stream_blocks", "inflate_stream_blocks_call", "inflate_stream_blocks"):
        assert "def %s(" % name in text, name
    assert callable(pkg.hip_inflate_stream_blocks)
    assert ctypes.sizeof(pkg.BlockIndexSummary) == 56


def test_symbols_are_declared_with_as_many_arguments(pkg):
    text = header_text()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    params = open(os.path.join(hdtest.ROOT, "include", "hipdeflate_params.h")).read()
    assert re.search(r"#define\s+HD_BLOCK_ROW_BYTES\s+\(128u << 10\)", params) and pkg.BLOCK_ROW_BYTES == 128 << 10


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: covered by the gpu tests")
def test_without_a_device_the_calls_say_so(pkg):
    lib = pkg.lib()
    s, x = pkg.StreamSummary(), pkg.BlockIndexSummary()
    buf = (ctypes.c_uint8 * 64)()
    n = ctypes.c_size_t(64)
    assert lib.hipdeflate_stream_index_blocks_dev(None, 0, pkg.FRAME_RAW, 0, 0, 0, None, None, None, None, None, ctypes.byref(x),
                                                  None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_stream_inflate_blocks_dev(None, 0, pkg.FRAME_RAW, None, None, None, None, None, 0, None, 0,
                                                    ctypes.byref(s), None) == pkg.HD_E_NODEVICE
    assert lib.hip_inflate_stream_blocks(buf, ctypes.byref(n), buf, 64, pkg.FRAME_RAW, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_test_block_headers_dev(None, 0, None, 0, None, None) == pkg.HD_E_NODEVICE
    assert lib.hipdeflate_test_block_candidates_dev(None, 0, 0, None, 0, ctypes.byref(ctypes.c_uint64()), None) == pkg.HD_E_NODEVICE
    lib.hipdeflate_test_blocks_times(None)


def test_block_kernels_use_no_scratch_and_keep_the_lds_of_their_models(pkg):
    kernels = resource_log(pkg)
    for name in KERNELS:
        ours = {k: v for k, v in kernels.items() if name in k}
        assert len(ours) == 1, (name, list(kernels))
        for k, v in ours.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    blocks = [k for k in kernels if "k_blocks_" in k]
    assert len(blocks) == len(KERNELS), blocks
    for k in blocks:
        assert not any(t in k for t in TAKEN) and "k_carry_" not in k, k
    (piece,) = [v for k, v in kernels.items() if "k_blocks_pieceE" in k]
    assert piece["LDS Size"] <= 4 * 1280 and piece["VGPRs"] <= 64, piece                # four allocation units, 32 wavefronts per CU
    (dec,) = [v for k, v in kernels.items() if "k_blocks_decodeE" in k]
    (cdec,) = [v for k, v in kernels.items() if "k_carry_decodeE" in k]
    assert dec["LDS Size"] <= cdec["LDS Size"], (dec, cdec)
    for name in KERNELS:                                                                 # the filter and its passes need no LDS
        if name not in ("k_blocks_piece", "k_blocks_decode"):
            (v,) = [v for k, v in kernels.items() if name in k]
            assert v["LDS Size"] == 0, (name, v)
