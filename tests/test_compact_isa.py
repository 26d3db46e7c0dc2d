"""The gather kernel's body loop, held by the device listing of the build (7bgzf_amd/csrc/hd_api.device.s) and the
compiler's resource report beside it (hd_api.resources.log), read the way test_l1_step_isa.py and test_l1_lds_budget.py
read them.

k_compact runs on a second stream beside the level-1 encode kernel.  Its body loop moves COMPACT_GROUP
bytes per wavefront and trip with COMPACT_UNROLL 16-byte loads, which are all requested before the first wait,
COMPACT_UNROLL 16-byte stores and one back edge -- and no dword access, the form the kernel had (two loads, a wait for both
and one store per 256 bytes).  The bytes a wavefront keeps in flight are what the persistent grid of three wavefronts per CU
is sized by, so the unroll factor and the grid belong together.  Its registers stay few enough for the wavefront slots the
encoder leaves (21 encoder wavefronts of at most 80 registers on a CU's four SIMDs are six on one SIMD and five on three:
32 and 112 of a SIMD's 512 stay free, room for one and three wavefronts of 32), and it uses no scratch."""
import os
import re

import hdtest
import test_l1_step_isa as isa
import test_gpu_gather_wide as wide

VGPRS = 32             # the allocation the build reached: one gather wavefront fits beside six encoder wavefronts on a SIMD


def _header_constant(name):
    src = open(os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_compact.hpp")).read()
    m = re.search(r"^#define\s+HD_%s\s+(\d+)\s*$" % name, src, re.M)
    assert m, name
    return int(m.group(1))


def _kernel():
    text = isa._listing()
    starts = [i for i, l in enumerate(text) if re.match(r"^_ZN2hd9k_compactE\w*:", l)]
    assert len(starts) == 1, "one k_compact in the listing"
    a = starts[0]
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[a:b]


def _body_loop(lines):
    """the innermost loop that stores 16 bytes per lane: from its header's label to its back edge"""
    found = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if not m:
            continue
        ends = [k for k in range(i + 1, len(lines)) if re.search(r"s_cbranch\S*\s+" + re.escape(m.group(1)) + r"\b", lines[k])]
        if not ends:
            continue
        inner = lines[i + 1:ends[-1] + 1]
        if any(re.match(r"^\.LBB\d+_\d+:", x) for x in inner):
            continue                                   # an outer loop
        if any("global_store_dwordx4" in x for x in inner):
            found.append(isa._instructions(inner))
    assert len(found) == 1, "one body loop"
    return found[0]


def test_group_constant_is_the_header_s():
    unroll = _header_constant("COMPACT_UNROLL")
    assert unroll >= 4
    assert wide.GROUP == 64 * 16 * unroll          # what tests/test_gpu_gather_wide.py puts its lengths round


def test_body_loop_is_sixteen_byte_accesses_all_loads_ahead_of_the_first_wait():
    unroll = _header_constant("COMPACT_UNROLL")
    body = _body_loop(_kernel())
    print("\n".join(body))
    loads = [n for n, t in enumerate(body) if t.startswith("global_load_dwordx4")]
    stores = [n for n, t in enumerate(body) if t.startswith("global_store_dwordx4")]
    assert len(loads) == unroll and len(stores) == unroll
    narrow = [t for t in body if re.match(r"(global|flat|buffer)_(load|store)_", t) and "_dwordx4" not in t]
    assert not narrow, narrow                      # no global_load_dword / global_store_dword / byte access in the loop
    waits = [n for n, t in enumerate(body) if t.startswith("s_waitcnt") and "vmcnt" in t]
    assert waits and sum(1 for n in loads if n < waits[0]) >= 4, "at least four loads in flight before the first wait"
    assert max(loads) < min(stores)
    branches = [t for t in body if t.startswith(("s_branch", "s_cbranch"))]
    assert len(branches) == 1 and body[-1] == branches[0], "one back edge per group"
    # the copy computes nothing but its two addresses
    valu = [t for t in body if t.startswith("v_")]
    assert len(valu) <= 2, valu


def test_loads_and_stores_pass_the_l1_by():
    """nontemporal accesses (the `nt` bit): the CU's L1 stays the encode kernel's"""
    body = _body_loop(_kernel())
    for t in body:
        if t.startswith(("global_load_dwordx4", "global_store_dwordx4")):
            assert re.search(r"\bnt\b", t), t


def test_registers_and_scratch():
    log = os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_api.resources.log")
    assert os.path.exists(log), "build with make -C 7bgzf_amd/csrc"
    kernels, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {}) if re.match(r"_ZN2hd9k_compactE", m.group(1)) else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(kernels) == 1, sorted(kernels)
    v = next(iter(kernels.values()))
    print(v)
    assert v["VGPRs"] <= VGPRS and v.get("AGPRs", 0) == 0, v
    assert v["ScratchSize"] == 0 and v["LDS Size"] == 0, v
