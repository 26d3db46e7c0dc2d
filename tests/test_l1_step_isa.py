"""The level-1 encode kernel's step, held at instruction level by the device listing of the build
(7bgzf_amd/csrc/hd_api.device.s, written by the Makefile next to hd_api.resources.log).

The kernel's 16 GiB rate follows the number of instructions a wavefront issues per 64-byte step and the LDS round trips it
waits for, so what the compiler makes of the step is part of the product.  The listing's 4 x 4-step group loop of the plain
instantiation (k_deflate_static<12, 11, false, 0, false>: four unrolled INNER steps, their emit passes and the long-match
blocks) is located the way tools/valu_by_phase.py locates it, and held to:
  * no v_readfirstlane_b32 of the lane-id register: the compiler's placeholder definition for loop-carried scalars that
    one exit of the step left undefined (three per step while the queue was merged where it was pushed; the merges they
    stood in front of went with that) -- issued on the vector pipe, computing nothing;
  * a wait for the token queue's ds_permute_b32 only inside the emit pass: the pushed register joins the queue one step
    later, so no always-run s_waitcnt lgkmcnt(0) stands between the push and the step's end;
  * at most the number of vector instructions this build reached."""
import os
import re

import hdtest

L1_LOOP_VALU = 505       # the loop body's vector instructions this build reached (the parent commit's listing: 536)
L1_LOOP_VALU_PARENT = 536
PLAIN = "_ZN2hd16k_deflate_staticILi12ELi11ELb0ELi0ELb0EEEvNS_11DeflateArgsE"


def _listing():
    path = os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_api.device.s")
    assert os.path.exists(path), "build with make -C 7bgzf_amd/csrc"
    return open(path).read().split("\n")


def _kernel(text):
    a = next(i for i, l in enumerate(text) if l.startswith(PLAIN + ":"))
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[a:b]


def _group_loop(lines):
    """the first depth-2 loop of the kernel, from its header's label to its back edge"""
    h = next(i for i, l in enumerate(lines) if "This Loop Header: Depth=2" in l)
    start = max(i for i in range(h) if re.match(r"^\.LBB\d+_\d+:", lines[i]))
    hdr = lines[start].split(":")[0]
    end = max(i for i in range(start + 1, len(lines)) if re.search(r"s_c?branch\S*\s+" + re.escape(hdr) + r"\b", lines[i]))
    return lines[start:end + 1]


def _instructions(lines):
    out = []
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out.append(t)
    return out


def test_group_loop_is_the_four_step_body():
    body = _instructions(_group_loop(_kernel(_listing())))
    # four unrolled steps: four greedy scans of 22 v_perm_b32 each (hd_device.hpp fn8_scan: 4 x 4 + 4 + 2) ... and four pushes
    assert sum(1 for t in body if t.startswith("v_perm_b32")) == 44, "not the 4-step group loop"
    assert sum(1 for t in body if t.startswith("ds_permute_b32")) == 4


def test_no_placeholder_readfirstlane_of_the_lane_id():
    body = _instructions(_group_loop(_kernel(_listing())))
    # v0 is the workitem id the kernel starts with: the lane id for as long as nothing writes it, and nothing in the loop does
    written = [t for t in body if re.match(r"(v_|ds_read|ds_permute|ds_bpermute|global_load|buffer_load|flat_load)\S*\s+v(0|\[0:\d+\])\s*,", t)
               and not t.startswith("v_cmp")]
    assert not written, written[:3]
    bad = [t for t in body if re.match(r"v_readfirstlane_b32\s+s\d+,\s*v0$", t)]
    assert not bad, bad


def _with_labels(lines):
    out = []
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        out.append(t)
    return out


def test_queue_push_is_not_waited_for_where_it_is_issued():
    """from every push, along the path that does NOT run the emit pass (the taken side of the first conditional branch
    behind the push: 'fewer than 64 queued'), the next step's first LDS read is issued before any s_waitcnt lgkmcnt(0)"""
    body = _with_labels(_group_loop(_kernel(_listing())))
    label = {t[:-1]: i for i, t in enumerate(body) if t.endswith(":")}
    pushes = [i for i, t in enumerate(body) if t.startswith("ds_permute_b32")]
    assert len(pushes) == 4
    for i in pushes:
        k, seen, branched, reads = i + 1, 0, False, None
        while reads is None:
            assert seen < 400, "no LDS read behind the push at %d" % i
            seen += 1
            t = body[k % len(body)]                     # (the back edge: the loop's first step follows its last)
            k = k % len(body) + 1
            if t.startswith("s_waitcnt"):
                assert "lgkmcnt(0)" not in t, (body[i], t)
            elif t.startswith("s_cbranch_scc1") and not branched:
                branched = True                         # queue not full: the step ends here
                k = label[t.split()[1]]
            elif t.startswith("s_branch"):
                k = label[t.split()[1]] if t.split()[1] in label else 0
            elif t.startswith("ds_read"):
                reads = t
        assert branched, "no 'queue not full' branch behind the push at %d" % i


def test_vector_instruction_count_of_the_group_loop():
    body = _instructions(_group_loop(_kernel(_listing())))
    valu = sum(1 for t in body if t.startswith("v_"))
    assert L1_LOOP_VALU <= L1_LOOP_VALU_PARENT
    assert valu <= L1_LOOP_VALU, (valu, L1_LOOP_VALU)
