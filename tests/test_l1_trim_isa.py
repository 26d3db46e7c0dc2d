"""Four vector instructions per step that the level-1 encode kernel no longer issues, held by the device listing of the build
(7bgzf_amd/csrc/hd_api.device.s) and the compiler's resource report beside it, read the way test_l1_step_isa.py,
test_l1_event_isa.py and test_l1_lds_budget.py read them:
  * the candidate's bytes are aligned by the candidate's position itself -- v_alignbyte_b32 reads bits [1:0] of its shift
    operand -- so no v_and_b32 ..., 3 feeds one;
  * the match token word is a v_sub_u32 from a position register that carries the word's constant part and one
    v_lshl_add_u32 (no v_sub_u32_sdwa + v_add3_u32 with the constant);
  * the queue push sends from every lane, the select that kept the lanes without a token out is gone: 52 v_cndmask_b32
    in the body where the parent commit's listing has 56;
  * the long-match events mask their addresses into the ring with v_and_b32 and a literal: no v_and_or_b32 in the four
    depth-3 loops.  That form is right only while the ring is the kernel's first LDS object, LDS [0, 4112): the table behind it
    is addressed with offset:4112 in every access of the body, in the plain and in the PRIMED instantiation -- an LDS object
    that moved in front of the ring would show here.
The counts are the ones this build reached; none is above the parent commit's listing (467 / 285 / 56), the scan's lookups are
the 44 that test_l1_step_isa.py and test_l1_scan_isa.py hold, and no resource line grew: at most 80 VGPRs for both level-1
instantiations (six wavefronts per SIMD), and level 2's parse kernel, which compiles the same step, at most its parent's 89."""
import re

import test_l1_event_isa as ev
import test_l1_lds_budget as budget
import test_l1_step_isa as isa

BODY_VALU = (455, 467)           # this build, the parent commit's listing
BODY_SALU = 285
BODY_PERM = 44
BODY_CNDMASK = (52, 56)
TABLE_OFFSET = 4112              # ring 4096 + its 16 mirrored bytes
L1_VGPRS = 80
L2_PARSE_VGPRS = 89              # the parent commit's listing
PRIMED = isa.PLAIN.replace("Lb0EEEvNS_11DeflateArgsE", "Lb1EEEvNS_11DeflateArgsE")


def _kernel(name):
    text = isa._listing()
    a = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[a:b]


def _body_lines(name=isa.PLAIN):
    return isa._group_loop(_kernel(name))


def test_body_counts():
    body = isa._instructions(_body_lines())
    valu = sum(1 for t in body if t.startswith("v_"))
    salu = ev._count(body, "salu")
    perm = sum(1 for t in body if t.startswith("v_perm_b32"))
    cnd = sum(1 for t in body if t.startswith("v_cndmask_b32"))
    print("group loop body: v_* %d, scalar ALU %d, v_perm_b32 %d, v_cndmask_b32 %d" % (valu, salu, perm, cnd))
    assert BODY_VALU[0] < BODY_VALU[1] and BODY_CNDMASK[0] < BODY_CNDMASK[1]
    assert valu <= BODY_VALU[0], valu
    assert salu <= BODY_SALU, salu
    assert perm == BODY_PERM, perm
    assert cnd <= BODY_CNDMASK[0], cnd


def test_no_and_or_in_the_long_match_loops():
    loops = ev._loop_instructions(_body_lines())
    assert len(loops) == 4, list(loops)
    for k, ins in loops.items():
        assert not [t for t in ins if t.startswith("v_and_or_b32")], (k, ins)
        # ... and the two addresses of a pass are masked by the literal W - 1
        assert sum(1 for t in ins if re.match(r"v_and_b32(_e32)?\s+v\d+, 0xfff, v\d+$", t)) == 2, (k, ins)


def test_no_shift_amount_mask_feeds_an_alignbyte():
    body = isa._instructions(_body_lines())
    aligns = [i for i, t in enumerate(body) if t.startswith("v_alignbyte_b32")]
    assert len(aligns) >= 16, len(aligns)            # four per step: own bytes and candidate bytes, low and high dword
    for i in aligns:
        shift = body[i].replace(",", " ").split()[-1]
        assert re.match(r"v\d+$", shift), body[i]
        # the instruction that wrote the shift operand last, walking back round the loop
        for k in range(1, len(body)):
            t = body[(i - k) % len(body)]
            if re.match(r"v_\S+\s+" + shift + r"\b", t) and not t.startswith("v_cmp"):
                assert not re.match(r"v_and_b32(_e32|_e64)?\s+v\d+, 3, v\d+$", t), (t, body[i])
                break


def test_table_follows_the_ring_at_4112():
    for name in (isa.PLAIN, PRIMED):
        body = isa._instructions(_body_lines(name))
        table = [t for t in body if t.startswith(("ds_read_u16", "ds_write_b16"))]
        assert len(table) == 8, (name, table)           # a lookup and a publish per step
        assert all(t.endswith("offset:%d" % TABLE_OFFSET) for t in table), (name, table)
        # the staging ring behind the table: 4112 + 3072
        stage = [t for t in body if t.startswith("ds_or_b32")]
        assert stage and all(t.endswith("offset:%d" % (TABLE_OFFSET + 3072)) for t in stage), (name, stage)
        # the ring's own accesses carry no base: at most the dword offsets inside an index's three dwords
        ring = [t for t in body if t.startswith(("ds_read_u8", "ds_read_b32", "ds_read2_b32")) and "offset:%d" % (TABLE_OFFSET + 3072) not in t]
        for t in ring:
            m = re.search(r"offset:(\d+)$", t)
            assert not m or int(m.group(1)) <= 16, (name, t)


def test_no_resource_line_grew():
    sta = budget._static_kernels()
    assert len(sta) == 3, sorted(sta)
    for k, v in sta.items():
        print(k, v["VGPRs"], v["LDS Size"], v["ScratchSize"])
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= (L2_PARSE_VGPRS if k[2] else L1_VGPRS), (k, v)
