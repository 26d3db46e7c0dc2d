"""The greedy scan's first three stages fetch no upper dword (hd_device.hpp Fn8Ident, fn8_scan_state0), held by the
device listing of the build (7bgzf_amd/csrc/hd_api.device.s) at the loop tests/test_l1_scan_isa.py reads: the plain
instantiation's group loop body, four unrolled INNER steps.

Every lane's map is elementary, so the upper dword that row_shr:1, :2 and :4 would bring is a constant of the lane
and sits in a register; those stages move the lower dword alone.  In each of the body's four scans:
  * row_shr:1, row_shr:2 and row_shr:4 stand on exactly one v_or_b32_dpp each, row_shr:8 (maps of eight lanes: data)
    on two;
and in the body:
  * at most the vector instructions this build reached, strictly below the parent's 483 (16 fewer: 3 DPP and one
    v_cndmask_b32 a step);
  * no more scalar ALU instructions than the parent's 285 (the wave-uniform upper dword of the lanes' own maps lives
    in a scalar register set outside the loop)."""
import test_l1_event_isa as event
import test_l1_scan_isa as scan

L1_LOOP_VALU = 467          # the loop body's vector instructions this build reached
L1_LOOP_VALU_PARENT = 483   # the parent commit's listing
L1_LOOP_SALU = 285          # scalar ALU instructions (tests/test_l1_event_isa.py BODY_SALU)


def test_each_scan_moves_one_dword_in_its_first_three_stages():
    body = scan._body()
    spans = scan._scans(body)
    assert len(spans) == 4, spans
    for a, b in spans:
        ors = [t for t in body[a:b + 1] if t.startswith("v_or_b32_dpp")]
        per = {d: sum(1 for t in ors if "row_shr:%d " % d in t) for d in (1, 2, 4, 8)}
        assert per == {1: 1, 2: 1, 4: 1, 8: 2}, (per, ors)
        assert len(ors) == 5, ors
        # the lookups all stay (tests/test_l1_scan_isa.py holds a scan to eleven)
        assert sum(1 for t in body[a:b + 1] if t.startswith("v_perm_b32")) == 11


def test_no_other_row_shift_of_the_scan_is_left_in_the_body():
    body = scan._body()
    for d, n in ((1, 4), (2, 4), (4, 4), (8, 8)):
        got = [t for t in body if t.startswith("v_or_b32_dpp") and "row_shr:%d " % d in t and "row_mask:0xf bank_mask:0xf" in t]
        assert len(got) == n, (d, got)


def test_vector_and_scalar_count_of_the_group_loop():
    body = scan._body()
    valu = sum(1 for t in body if t.startswith("v_"))
    salu = event._count(body, "salu")
    print("group loop body: valu", valu, "salu", salu)
    assert L1_LOOP_VALU < L1_LOOP_VALU_PARENT == scan.L1_LOOP_VALU
    assert valu <= L1_LOOP_VALU, (valu, L1_LOOP_VALU, "parent", L1_LOOP_VALU_PARENT)
    assert salu <= L1_LOOP_SALU, (salu, L1_LOOP_SALU)
