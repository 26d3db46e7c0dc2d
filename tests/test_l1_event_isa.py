"""The level-1 encode kernel's long-match event, held by the device listing of the build (7bgzf_amd/csrc/hd_api.device.s),
read the way test_l1_step_isa.py and test_l1_mem_wait_order.py read it.

A wavefront's time per 64-byte step is its own serial chain -- scalar instructions, branches, wait-state fillers and the
LDS round trips it waits for -- more than its vector instructions, and the largest single item of that
chain is the long-match event: a match whose first eight bytes agree and that the parse takes, 1.42 of them per step on
FASTQ-like data.  The event is one block of assembly per step (hd_deflate_static.hpp, HD_L1_EVENTS): the lane of the event
lives in M0, the extension's scalar address half is the walk's first lane, no clamp and no wait-state filler is left in it.
Held here, in the plain instantiation, each to the count this build reached and none above the parent commit's:
  * scalar ALU instructions, branches and s_nop in the four long-match loops (depth 3, one per unrolled step);
  * s_nop in the whole 4-step group loop body;
  * scalar ALU instructions in the body."""
import re

import test_l1_step_isa as isa

#                       this build, the parent commit's listing
LOOPS_SALU = (96, 108)           # the four loops together: s_* without waits, s_nop and branches (24 per loop; parent 27)
LOOPS_BRANCHES = (28, 36)        # s_branch + s_cbranch_* (7 per loop; parent 9)
LOOPS_NOP = (0, 4)               # (parent: the one behind s_mov_b32 m0 in each loop)
BODY_NOP = (59, 63)
BODY_SALU = (285, 301)

_NOT_ALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch")


def _body_lines():
    return isa._group_loop(isa._kernel(isa._listing()))


def _loop_instructions(lines):
    """{header label: [instructions]} of the depth-3 loops inside `lines`, by the compiler's own loop annotations"""
    loops, cur = {}, None
    for n, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.\d+:", l)
        if m:
            cur = None
            member = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=3", l)
            if member:
                cur = ".L" + member.group(1)
            elif m.group(1):
                k = n + 1
                while k < len(lines) and lines[k].lstrip().startswith(";") and not lines[k].startswith("; %bb"):
                    if "This Inner Loop Header: Depth=3" in lines[k]:
                        cur = m.group(1)
                    k += 1
            continue
        t = l.split(";")[0].strip()
        if cur and t and not t.startswith(".") and not t.endswith(":"):
            loops.setdefault(cur, []).append(t)
    return loops


def _count(ins, what):
    if what == "salu":
        return sum(1 for t in ins if t.startswith("s_") and not t.startswith(_NOT_ALU))
    if what == "branches":
        return sum(1 for t in ins if t.startswith(("s_branch", "s_cbranch")))
    return sum(1 for t in ins if t.startswith("s_nop"))


def test_long_match_loops_scalar_branch_and_nop_count():
    loops = _loop_instructions(_body_lines())
    assert len(loops) == 4, list(loops)
    for what, (now, parent) in (("salu", LOOPS_SALU), ("branches", LOOPS_BRANCHES), ("nop", LOOPS_NOP)):
        per = {k: _count(v, what) for k, v in loops.items()}
        total = sum(per.values())
        print("long-match loops,", what, per, total)
        assert now <= parent
        assert total <= now, (what, per, now)


def test_group_loop_body_nop_and_scalar_count():
    body = isa._instructions(_body_lines())
    for what, (now, parent) in (("nop", BODY_NOP), ("salu", BODY_SALU)):
        got = _count(body, what)
        print("group loop body,", what, got)
        assert now <= parent
        assert got <= now, (what, got, now)
