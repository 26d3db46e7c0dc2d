"""The greedy scan of the level-1 step, held at instruction level by the device listing of the build
(7bgzf_amd/csrc/hd_api.device.s), the way tests/test_l1_step_isa.py holds the step around it.

The kernel runs with its vector pipe about nine tenths busy, so every vector instruction on the
always-run path is paid for in full.  In the plain instantiation's group loop body (four unrolled INNER steps):
  * the scan's two cross-row stages write the shifted rows into the registers that hold their identity constants
    (hd_device.hpp fn8_scan_state0): no v_mov_b32_e32 seeds a destination anywhere between a step's first row_shr:1
    stage and the last v_perm_b32 of its scan;
  * "state entering lane l" is the mask of "state 0 behind lane l" shifted in scalar registers: no DPP instruction with
    wave_shr is left in the loop;
  * at most the number of vector instructions this build reached."""
import os
import re

import hdtest

L1_LOOP_VALU = 483       # the loop body's vector instructions this build reached
L1_LOOP_VALU_PARENT = 499   # the parent commit's listing
PLAIN = "_ZN2hd16k_deflate_staticILi12ELi11ELb0ELi0ELb0EEEvNS_11DeflateArgsE"


def _listing():
    path = os.path.join(os.path.dirname(hdtest.pkg().LIB_PATH), "csrc", "hd_api.device.s")
    assert os.path.exists(path), "build with make -C 7bgzf_amd/csrc"
    return open(path).read().split("\n")


def _body():
    """the instructions of the first depth-2 loop of the plain kernel, from its header's label to its back edge"""
    text = _listing()
    a = next(i for i, l in enumerate(text) if l.startswith(PLAIN + ":"))
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    lines = text[a:b]
    h = next(i for i, l in enumerate(lines) if "This Loop Header: Depth=2" in l)
    start = max(i for i in range(h) if re.match(r"^\.LBB\d+_\d+:", lines[i]))
    hdr = lines[start].split(":")[0]
    end = max(i for i in range(start + 1, len(lines)) if re.search(r"s_c?branch\S*\s+" + re.escape(hdr) + r"\b", lines[i]))
    out = []
    for l in lines[start:end + 1]:
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    return out


def _scans(body):
    """[first row_shr:1 stage, last v_perm_b32 of the scan] of each step: the scan is the only user of row_shr:1 with a full
    row mask on a v_or_b32 (the emit pass's prefix sum adds), and its 11 v_perm_b32 follow"""
    first = [i for i, t in enumerate(body) if t.startswith("v_or_b32_dpp") and "row_shr:1 " in t]
    spans = []
    for i in first:
        if spans and i <= spans[-1][1]:
            continue                                   # the stage's second dword
        perms, k = 0, i
        while perms < 11:
            k += 1
            assert k < len(body), "a scan without its 11 v_perm_b32"
            perms += body[k].startswith("v_perm_b32")
        spans.append((i, k))
    return spans


def test_the_loop_holds_four_scans():
    body = _body()
    assert sum(1 for t in body if t.startswith("v_perm_b32")) == 44, "not the 4-step group loop"
    spans = _scans(body)
    assert len(spans) == 4, spans
    for a, b in spans:
        # nothing but the scan in between: its DPP stages, its lookups and the wait states
        assert b - a < 40, (a, b)


def test_no_wave_shr_in_the_loop():
    bad = [t for t in _body() if "wave_shr" in t]
    assert not bad, bad[:3]


def test_no_seed_move_inside_a_scan():
    body = _body()
    for a, b in _scans(body):
        bad = [t for t in body[a:b + 1] if t.startswith("v_mov_b32_e32")]
        assert not bad, bad
        # the cross-row stages are the seedless form: three v_mov_b32_dpp with a row mask, no v_or_b32_dpp with one
        moves = [t for t in body[a:b + 1] if t.startswith("v_mov_b32_dpp") and "row_bcast" in t]
        assert len(moves) == 3, moves
        assert not [t for t in body[a:b + 1] if t.startswith("v_or_b32_dpp") and "row_bcast" in t]


def test_vector_instruction_count_of_the_group_loop():
    valu = sum(1 for t in _body() if t.startswith("v_"))
    assert L1_LOOP_VALU < L1_LOOP_VALU_PARENT
    assert valu <= L1_LOOP_VALU, (valu, L1_LOOP_VALU, "parent", L1_LOOP_VALU_PARENT)
