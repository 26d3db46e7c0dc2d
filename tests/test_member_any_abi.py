"""CPU-only checks of the built library for the member index that sizes by decoding: the new symbols are exported, the
summary has the header's layout, and k_inflate_member keeps the size pass's budget -- read from the compiler's resource
report the way tests/test_abi.py reads the other kernels."""
import ctypes
import os
import re
import subprocess

import hdtest


def kernels_of_the_build():
    log = os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_api.resources.log")
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
    return kernels


def test_symbols_are_exported_and_the_summary_is_48_bytes():
    pkg = hdtest.pkg()
    assert os.path.exists(pkg.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name in ("hipdeflate_index_members_any_dev", "hip_inflate_members"):
        assert name in exported and name in pkg.EXPORTS, name
        assert getattr(pkg.lib(), name) is not None
    # ... and the code object inside the library holds the two wavefront-per-candidate kernels
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"k_inflate_member" in blob and b"k_member_open" in blob
    s = pkg.MemberAnySummary
    assert ctypes.sizeof(s) == 48
    assert [(f, getattr(s, f).offset) for f, _ in s._fields_] == [("nmembers", 0), ("out_bytes", 8), ("end_offset", 16), ("ncandidates", 24),
                                                                 ("nsized", 32), ("status", 40)]


def test_member_form_keeps_the_size_pass_budget():
    kernels = kernels_of_the_build()
    member = {k: v for k, v in kernels.items() if "k_inflate_memberE" in k}
    assert len(member) == 1, list(kernels)
    (v,) = member.values()
    assert v["VGPRs"] <= 64 and -(-v["LDS Size"] // 1280) <= 4 and v["ScratchSize"] == 0, v
    # the new index kernels spill nothing either
    new = {k: v for k, v in kernels.items() if re.search(r"k_(any_\w+?|member_open)E", k)}
    assert len(new) == 8, sorted(new)
    for k, v in new.items():
        assert v["ScratchSize"] == 0, (k, v)
