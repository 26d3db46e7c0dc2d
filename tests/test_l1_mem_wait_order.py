"""The level-1 encode kernel's vector-memory waits and its long-match loops, held by the device listing of the build
(7bgzf_amd/csrc/hd_api.device.s), read the way test_l1_step_isa.py reads it.

s_waitcnt vmcnt(N) counts vector-memory operations in ISSUE order: a wait for a younger operation cannot pass before every
older one is back, whether the older one's result is wanted or not.  Two places of the kernel had an operation nobody needs
soon standing in front of one that is needed at once (hd_deflate_static.hpp, fill_piece and emit_tokens):
  * the refill asked for the NEXT piece -- an HBM miss, wanted 16 steps later -- and then issued the CRC's twenty table
    gathers: their first wait stood for the whole HBM round trip, at the head of every 16-step group;
  * the emit pass stored the staged dwords and then gathered its code table: the wait for the gather stood for the store's
    acknowledgement as well, in every pass.
Held here, in the plain and the PRIMED level-1 instantiation:
  (a) in the block that refills the ring ahead of the group loop, the global_load_dwordx4 of the next piece comes behind the
      last CRC-table global_load_dword;
  (b) no s_waitcnt vmcnt stands between that global_load_dwordx4 and the group loop's header;
  (c) the group loop body has exactly four global_load_dword (the four passes' table gathers), no global_store_dword stands
      between one of them and the first s_waitcnt vmcnt behind it -- and none between a store and the next gather either
      (walking round the back edge), so that nothing in the loop waits for a store;
  (d) the four long-match loops (depth 3, one per unrolled step) hold at most the scalar instructions this build reached."""
import re

import pytest

import test_l1_step_isa as isa

PLAIN = isa.PLAIN
PRIMED = "_ZN2hd16k_deflate_staticILi12ELi11ELb0ELi0ELb1EEEvNS_11DeflateArgsE"
L1_LONG_MATCH_SALU = 108          # the four loops together, s_* without waits, nops and branches (the parent commit's listing: 128)
L1_LONG_MATCH_SALU_PARENT = 128


def _kernel(sym):
    text = isa._listing()
    a = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
    b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[a:b]


def _op(line):
    return line.split(";")[0].strip()


def _is_vm_wait(t):
    return t.startswith("s_waitcnt") and "vmcnt" in t


def _refill_block(lines):
    """the lines between the header of the depth-1 loop around the group loop and the group loop's own header"""
    h = next(i for i, l in enumerate(lines) if "This Loop Header: Depth=2" in l)
    start = max(i for i in range(h) if re.match(r"^\.LBB\d+_\d+:", lines[i]))
    outer = max(i for i in range(start) if "Loop Header: Depth=1" in lines[i])
    return [_op(l) for l in lines[outer:start]]


@pytest.mark.parametrize("sym", [PLAIN, PRIMED], ids=["plain", "primed"])
def test_next_piece_is_requested_behind_the_crc_gathers(sym):
    blk = _refill_block(_kernel(sym))
    gathers = [i for i, t in enumerate(blk) if re.match(r"global_load_dword\s", t)]
    pieces = [i for i, t in enumerate(blk) if t.startswith("global_load_dwordx4")]
    assert len(gathers) == 20, len(gathers)                 # CrcLanes::fold: 4 + 16 table loads
    assert pieces, "no refill in front of the group loop"
    x4 = pieces[-1]
    assert x4 > gathers[-1], (x4, gathers[-1])              # (a)
    waits = [t for t in blk[x4:] if _is_vm_wait(t)]
    assert not waits, waits                                 # (b)
    # ... and the gathers are waited for in front of it: the request is the youngest operation when it goes out
    assert any(_is_vm_wait(t) and "vmcnt(0)" in t for t in blk[gathers[-1]:x4])


@pytest.mark.parametrize("sym", [PLAIN, PRIMED], ids=["plain", "primed"])
def test_no_pass_waits_for_its_store(sym):
    body = isa._instructions(isa._group_loop(_kernel(sym)))
    loads = [i for i, t in enumerate(body) if re.match(r"global_load_dword\s", t)]
    stores = [i for i, t in enumerate(body) if t.startswith("global_store")]
    assert len(loads) == 4, loads
    assert len(stores) == 4 and all(body[i].startswith("global_store_dword ") for i in stores), stores
    assert not any(t.startswith(("global_load", "buffer_", "flat_", "scratch_")) for i, t in enumerate(body) if i not in loads)
    for i in loads:
        k = i + 1
        while not _is_vm_wait(body[k]):
            assert not body[k].startswith("global_store"), (i, k, body[k])
            k += 1
    for i in stores:
        k = (i + 1) % len(body)
        while k not in loads:                                   # (the back edge: the loop's first step follows its last)
            assert not _is_vm_wait(body[k]), (i, k, body[k])
            k = (k + 1) % len(body)


def _blocks(lines):
    """[(label of the depth-3 loop the block belongs to, or None, [instructions])] of the basic blocks of `lines`"""
    out, cur = [], None
    for n, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.\d+:", l)
        if m:
            name = None
            member = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=3", l)
            if member:
                name = ".L" + member.group(1)
            elif m.group(1):
                k = n + 1                                   # a header's annotation runs on over the comment lines behind its label
                notes = [l]
                while k < len(lines) and lines[k].lstrip().startswith(";") and not lines[k].startswith("; %bb"):
                    notes.append(lines[k])
                    k += 1
                if any("This Inner Loop Header: Depth=3" in x for x in notes):
                    name = m.group(1)
            cur = []
            out.append((name, cur))
            continue
        t = _op(l)
        if cur is not None and t and not t.startswith(".") and not t.endswith(":"):
            cur.append(t)
    return out


def _long_match_salu(sym_lines):
    loops = {}
    for name, ins in _blocks(isa._group_loop(sym_lines)):
        if name:
            loops.setdefault(name, []).extend(ins)
    salu = {k: sum(1 for t in v if t.startswith("s_") and not t.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch")))
            for k, v in loops.items()}
    return loops, salu


def test_long_match_loops_scalar_count():
    loops, salu = _long_match_salu(_kernel(PLAIN))
    assert len(loops) == 4, list(loops)
    # each is the extension loop's home: one ds_read_u8 pair, one v_writelane_b32, the walk's v_readlane_b32
    for k, v in loops.items():
        assert sum(1 for t in v if t.startswith("ds_read_u8")) == 2, k
        assert sum(1 for t in v if t.startswith("v_writelane_b32")) == 1, k
    total = sum(salu.values())
    print("long-match loops, scalar instructions:", salu, total)
    assert L1_LONG_MATCH_SALU <= L1_LONG_MATCH_SALU_PARENT
    assert total <= L1_LONG_MATCH_SALU, (salu, L1_LONG_MATCH_SALU)
