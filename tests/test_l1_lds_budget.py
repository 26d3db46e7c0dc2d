"""The level-1 encode kernel's occupancy, held by the compiler's resource report of the build
(7bgzf_amd/csrc/hd_api.resources.log, written by the Makefile).

LDS is granted in 1280-byte units and a CU has 128 of them: six units per wavefront are 21 wavefronts per CU, seven are 18.
The two level-1 instantiations of k_deflate_static (TOK = 0: plain and PRIMED) fit six units since their token queue moved
into a register and their staging ring shrank to one emit pass (hd_deflate_static.hpp: ring 4112 + table 3072 + staging 256 =
7440 B).  21 per CU also needs six wavefronts on one SIMD, i.e. an allocation of at most 80 of its 512 registers -- the build
reached 79 -- and no scratch.  A byte or a register over and the kernel silently runs 18 (or 20) per CU again: this test
says so at build time.  (The TOK = 1 instantiation, level 2's parse, keeps its LDS queue and its seven units:
tests/test_abi.py::test_kernel_resource_budgets_by_template_args holds that one.)"""
import os
import re

import hdtest

LDS_UNIT = 1280
L1_UNITS = 6
L1_VGPRS = 80          # the allocation the build reached: six wavefronts per SIMD


def _static_kernels():
    log = os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_api.resources.log")
    assert os.path.exists(log), "build with make -C 7bgzf_amd/csrc"
    kernels, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {}) if "k_deflate_static" in m.group(1) else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    out = {}
    for k, v in kernels.items():
        # k_deflate_static<WIN_BITS, HASH_BITS, TOK, INTRA, PRIMED>, read back from the mangled name
        m = re.search(r"k_deflate_staticI((?:L[ib]\d+E)+)EEvNS_11DeflateArgsE$", k)
        assert m, k
        out[tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))] = v
    return out


def test_level1_kernels_fit_six_lds_units_and_eighty_registers():
    sta = _static_kernels()
    assert len(sta) == 3, sorted(sta)
    l1 = {k: v for k, v in sta.items() if k[2] == 0}
    assert sorted(k[4] for k in l1) == [0, 1], sorted(sta)           # plain and PRIMED
    for k, v in l1.items():
        assert v["LDS Size"] <= L1_UNITS * LDS_UNIT, (k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= L1_VGPRS, (k, v)
        assert v.get("AGPRs", 0) == 0, (k, v)                        # (they would count against the same 512)
