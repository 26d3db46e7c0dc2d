"""The batch encoder with a preset dictionary -- hipdeflate_batch_deflate_dict_dev, hipdeflate_batch_deflate_dict and their
device.py / package forms -- against tests/dict_model.py: per block, the tokens read out of the device's member are the tokens
the CPU twin's one-block parse of (the dictionary's used tail || block) makes behind the seam.  Bit-exact, no tolerances.

Every member made here is held to the form first (encode()): zlib.decompressobj(-15, zdict=dictionary) returns the block with
eof set and nothing unused, crc32[b] is the block's alone, and the bytes around every slot's room are untouched.  No case
provokes a fault; every refusal is one the header defines.

Where the cases land (hd_deflate_wg.hpp parse_wg<..., WG_HIST_DICT>, k_dict_table; hd_api.hip batch_deflate_dev_impl):
  * dict_len 1024 / 1025 / 5000 / 32768 / 40000: used 1024, 1024 (one byte unused), 4096 (904 unused), the window, its tail;
  * the eight block lengths of one launch go both ways: with 32 KiB of history 32 KiB is the last block whose (history ||
    block) fits the ring of 64 pieces -- the table snapshot and the bulk load --, 33 KiB the first that replays, 64 KiB runs
    through the filler; with shorter histories 64 KiB is the only one that replays;
  * every launch is made twice, with the snapshot and with hipdeflate_test_dict_replay(1): equal bytes."""
import importlib
import os
import zlib

import numpy as np
import pytest

import dict_cases as dc
import dict_model as dm
import hdtest

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 0xa5


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def dev():
    return importlib.import_module("7bgzf_amd.device")


@pytest.fixture(autouse=True)
def no_stalls(pkg):
    yield
    assert pkg.lib().hipdeflate_stall_count() == 0


def to_dev(torch, blob, shift=0):
    """the bytes on the device, `shift` bytes behind a 16-byte boundary"""
    buf = torch.from_numpy(np.frombuffer(bytes(shift) + bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    return buf[shift:shift + len(blob)]


def i64(torch, v):
    return torch.from_numpy(np.asarray(v, dtype=np.int64)).cuda()


def i32(torch, v):
    return torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32)).cuda()


def launch(torch, dev, pkg, data, offs, lens, level, d, d_shift=0, slot=None, cap=None, plain=False):
    """one device call over blocks data[offs[i]:offs[i] + lens[i]] -> (members, crc32, status); the slots lie between guards and
    every slot's room ends GUARD bytes in front of the next slot"""
    n = len(offs)
    if slot is None:
        slot = int(pkg.lib().hipdeflate_bound(max(lens), level)) + GUARD
    cap = slot - GUARD if cap is None else cap
    assert slot % 16 == 0 and cap <= slot - GUARD
    buf = torch.full((GUARD + n * slot + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out_len, crc, status = (torch.full((n,), -3, dtype=torch.int32, device="cuda") for _ in range(3))
    src = data if torch.is_tensor(data) else to_dev(torch, data)
    in_off, in_len = i64(torch, offs), i32(torch, lens)    # (held here: a pointer into a tensor nobody holds is a pointer into free memory)
    if plain:
        rc = pkg.lib().hipdeflate_batch_deflate_dev(src.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, level,
                                                    pkg.FRAME_RAW, buf[GUARD:].data_ptr(), slot, cap, out_len.data_ptr(),
                                                    crc.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        pkg._check(rc, "hipdeflate_batch_deflate_dev")
    else:
        dd = to_dev(torch, d, d_shift) if len(d) else None
        dev.deflate_dict_call(src, in_off, in_len, level, dd, buf[GUARD:], slot, cap, out_len, crc, status)
    got = bytes(buf.cpu().numpy())
    assert got[:GUARD] == bytes([SENT]) * GUARD and got[GUARD + n * slot:] == bytes([SENT]) * GUARD
    olen, st = out_len.cpu().tolist(), status.cpu().tolist()
    members = []
    for i in range(n):
        room = got[GUARD + i * slot:GUARD + (i + 1) * slot]
        # (the device calls' rule, tests/test_gpu_encode_room.py: nothing changes at or past the room's last whole dword)
        edge = (cap + 3) & ~3
        assert room[edge:] == bytes([SENT]) * (slot - edge), i
        assert st[i] or 0 <= olen[i] <= cap
        members.append(room[:olen[i]] if st[i] == 0 else b"")
    return members, crc.cpu().numpy().view(np.uint32).tolist(), st


def check_form(data, offs, lens, d, members, crc, status):
    """what every member of this encoder is held to"""
    assert status == [0] * len(offs)
    for i, (o, n) in enumerate(zip(offs, lens)):
        block = data[o:o + n]
        z = zlib.decompressobj(-15, zdict=bytes(d)) if len(d) else zlib.decompressobj(-15)
        assert z.decompress(members[i]) == block and z.eof and z.unused_data == b"", i
        assert crc[i] == zlib.crc32(block), i


_made = {}


def encode(torch, dev, pkg, kind, dict_len, level, lens=dc.BLOCK_LENS, replay=False):
    """(offs, lens, members) of one launch over the shared blocks, held to the form; made once"""
    key = (kind, dict_len, level, tuple(lens), replay)
    if key not in _made:
        data, d = dc.master(kind), dc.dictionary(kind, dict_len)
        offs, lens = dc.blocks(kind, lens)
        try:
            pkg.lib().hipdeflate_test_dict_replay(1 if replay else 0)
            members, crc, st = launch(torch, dev, pkg, data, offs, lens, level, d)
        finally:
            pkg.lib().hipdeflate_test_dict_replay(0)
        check_form(data, offs, lens, d, members, crc, st)
        _made[key] = (offs, lens, members)
    return _made[key]


def check_tokens(kind, dict_len, level, o, n, member):
    """the member's tokens are the model's, and they rebuild the block behind the history"""
    d, block = dc.dictionary(kind, dict_len), dc.master(kind)[o:o + n]
    toks, out = dm.member_tokens(member, dm.history_of(d))
    assert out == block
    want = dm.expected_tokens(d, block, level)
    if toks != want:
        k = next((j for j, (a, b) in enumerate(zip(toks, want)) if a != b), min(len(toks), len(want)))
        raise AssertionError("%s block of %d bytes (level %d, dict_len %d): token %d is %r, the model's %r (%d / %d tokens)"
                             % (kind, n, level, dict_len, k, toks[k:k + 1], want[k:k + 1], len(toks), len(want)))
    return toks


# ---- token identity, the snapshot against the replay --------------------------------------------------------------------

@pytest.mark.parametrize("dict_len", dc.DICT_LENS)
@pytest.mark.parametrize("level", dc.ENC_LEVELS)
@pytest.mark.parametrize("kind", dc.KINDS)
def test_tokens_are_the_one_block_parse_behind_the_seam(torch, dev, pkg, kind, level, dict_len):
    offs, lens, members = encode(torch, dev, pkg, kind, dict_len, level)
    reaching = 0
    for o, n, m in zip(offs, lens, members):
        toks = check_tokens(kind, dict_len, level, o, n, m)
        reaching += dm.dict_cost(toks)[0]
    assert reaching > 0                                    # the dictionary is used
    # the table snapshot and the replay of the history in every block write the same bytes
    assert encode(torch, dev, pkg, kind, dict_len, level, replay=True)[2] == members
    if level == 6 and dict_len == 32768:                   # levels 7..9 are level 6
        assert encode(torch, dev, pkg, kind, dict_len, 9)[2] == members


# ---- where there is no dictionary to use ----------------------------------------------------------------------------------

@pytest.mark.parametrize("level,dict_len", [(6, 0), (6, 1), (6, 1023), (3, 1023), (0, 32768), (1, 32768), (2, 32768), (2, 1024)])
def test_plain_call_bytes_where_the_dictionary_is_not_used(torch, dev, pkg, level, dict_len):
    lens = (1, 258, 2048, 4101, 33 << 10)
    for kind in dc.KINDS:
        data = dc.master(kind)
        offs, lens = dc.blocks(kind, lens)
        got = launch(torch, dev, pkg, data, offs, lens, level, dc.dictionary(kind, dict_len))
        assert got == launch(torch, dev, pkg, data, offs, lens, level, b"", plain=True)
        check_form(data, offs, lens, b"", *got)


# ---- the distance edge, alignment, many blocks -------------------------------------------------------------------------------

@pytest.mark.parametrize("replay", [False, True])
def test_distance_edge(torch, dev, pkg, replay):
    """a random 32 KiB block whose dictionary is the same 32 KiB: matches at distance 32768 exactly, from position 0 on"""
    d = dc.master("random")[:32768]
    data = bytes(64) + d
    try:
        pkg.lib().hipdeflate_test_dict_replay(1 if replay else 0)
        members, crc, st = launch(torch, dev, pkg, data, [64], [32768], 6, d)
    finally:
        pkg.lib().hipdeflate_test_dict_replay(0)
    check_form(data, [64], [32768], d, members, crc, st)
    toks, out = dm.member_tokens(members[0], d)
    assert out == d and toks == dm.expected_tokens(d, d, 6)
    first = next(t for t in toks if t[1])
    assert first[2] == 32768 and first[0] < 64             # the first match names the dictionary's furthest bytes
    assert sum(ln for p, ln, v in toks if v == 32768 and ln) > 32768 * 9 // 10 and len(members[0]) <= 32768 // 16


@pytest.mark.parametrize("level", [3, 6])
def test_alignment_of_dictionary_and_blocks(torch, dev, pkg, level):
    kind, dict_len, lens = "text", 5000, (258, 2048, 4101, 33 << 10)
    offs, lens, members = encode(torch, dev, pkg, kind, dict_len, level, lens)
    data, d = dc.master(kind), dc.dictionary(kind, dict_len)
    for shift in (1, 7):
        assert launch(torch, dev, pkg, data, offs, lens, level, d, d_shift=shift)[0] == members
    # the same blocks at odd offsets of another buffer, three bytes between them
    packed, at = bytearray(b"\x11"), []
    for o, n in zip(offs, lens):
        at.append(len(packed))
        packed += data[o:o + n] + b"\x22" * 3
    assert [a & 15 for a in at] != [0] * len(at) and any(a & 1 for a in at)
    assert launch(torch, dev, pkg, bytes(packed), at, lens, level, d, d_shift=3)[0] == members


def test_more_blocks_than_cus_and_the_gain_on_text(torch, dev, pkg):
    kind, n, size = "text", 600, 2048
    data, d = dc.master(kind), dc.dictionary(kind, 32768)
    offs, lens = dc.blocks(kind, (size,) * n)
    src = to_dev(torch, data)
    members, crc, st = launch(torch, dev, pkg, src, offs, lens, 6, d)
    check_form(data, offs, lens, d, members, crc, st)
    for i in (0, 1, 255, 256, 599):
        check_tokens(kind, 32768, 6, offs[i], lens[i], members[i])
    without, _, st0 = launch(torch, dev, pkg, src, offs, lens, 6, b"", plain=True)
    assert st0 == [0] * n
    # (2 KiB of text against 32 KiB of the same text: tests/test_dict_model.py shows the model saves a tenth at least)
    assert sum(map(len, members)) < sum(map(len, without)) * 9 // 10
    try:
        pkg.lib().hipdeflate_test_dict_replay(1)
        assert launch(torch, dev, pkg, src, offs, lens, 6, d)[0] == members
    finally:
        pkg.lib().hipdeflate_test_dict_replay(0)


# ---- room, refusals, the host form ------------------------------------------------------------------------------------------

def test_room(torch, dev, pkg):
    """the plain call's rule: a room holds a block no longer than itself, and the member must fit it.  Noise the dictionary
    does not help is the block whose member is longer than it: in a room of the member's size it is written, in a room one
    byte smaller the status is 1"""
    d = dc.dictionary("text", 32768)
    data = dc.master("random")
    offs, lens = [16, 3000, 8000], [2048, 2048, 1000]
    members, crc, st = launch(torch, dev, pkg, data, offs, lens, 6, d)
    check_form(data, offs, lens, d, members, crc, st)
    need = max(map(len, members))
    assert 2048 < need <= 2048 + 5 + 5 and [len(m) for m in members] == [need, need, len(members[2])]
    exact = launch(torch, dev, pkg, data, offs, lens, 6, d, slot=4096, cap=need)
    assert exact[0] == members and exact[2] == [0, 0, 0]
    short = launch(torch, dev, pkg, data, offs, lens, 6, d, slot=4096, cap=need - 1)
    assert short[2] == [1, 1, 0] and short[0][2] == members[2]
    assert short == launch(torch, dev, pkg, data, offs, lens, 6, b"", slot=4096, cap=need - 1, plain=True)
    # a block longer than its slot is refused at these levels, as the plain call refuses it
    data = dc.master("text")
    offs, lens = dc.blocks("text", (2048, 8192))
    for plain in (False, True):
        got = launch(torch, dev, pkg, data, offs, lens, 6, d, slot=4096 + GUARD, cap=4096, plain=plain)
        assert got[2] == [0, 1]


def test_refusals(torch, dev, pkg):
    src = to_dev(torch, bytes(4096))
    d = to_dev(torch, bytes(2048))
    out = torch.zeros(8192 + 16, dtype=torch.uint8, device="cuda")
    off, ln = i64(torch, [0]), i32(torch, [4096])
    res = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3)]
    L, st = pkg.lib(), torch.cuda.current_stream().cuda_stream
    ok = lambda dict_ptr, dict_len, o, stride, out_len: L.hipdeflate_batch_deflate_dict_dev(
        src.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 6, dict_ptr, dict_len, o, stride, stride, out_len, res[1].data_ptr(),
        res[2].data_ptr(), st)
    assert ok(d.data_ptr(), 2048, out.data_ptr(), 8192, res[0].data_ptr()) == 0
    assert ok(None, 0, out.data_ptr(), 8192, res[0].data_ptr()) == 0
    for bad in ((None, 2048, out.data_ptr(), 8192, res[0].data_ptr()), (d.data_ptr(), 2048, out[8:].data_ptr(), 8192, res[0].data_ptr()),
                (d.data_ptr(), 2048, out.data_ptr(), 8200, res[0].data_ptr()), (d.data_ptr(), 2048, out.data_ptr(), 8192, None)):
        assert ok(*bad) == 101                             # HD_E_ARG
    torch.cuda.synchronize()


def test_host_form(torch, dev, pkg):
    for kind, level, dict_len in (("text", 6, 32768), ("fastq", 3, 5000), ("text", 1, 32768), ("text", 6, 1023)):
        offs, lens = dc.blocks(kind, (1, 2048, 4101, 33 << 10))
        members = launch(torch, dev, pkg, dc.master(kind), offs, lens, level, dc.dictionary(kind, dict_len))[0]
        got, crc, st = pkg.batch_deflate_dict(dc.master(kind), offs, lens, dc.dictionary(kind, dict_len), level)
        assert got == members and list(st) == [0] * len(offs)
        assert [int(c) for c in crc] == [zlib.crc32(dc.master(kind)[o:o + n]) for o, n in zip(offs, lens)]
    # device.deflate_dict: the same members in slots of the bound
    kind, lens = "text", (2048, 4101)
    offs, lens, members = encode(torch, dev, pkg, kind, 32768, 6, lens)
    slots, slot, out_len, crc, status = dev.deflate_dict(to_dev(torch, dc.master(kind)), i64(torch, offs), i32(torch, lens),
                                                         to_dev(torch, dc.dictionary(kind, 32768)), 6)
    raw = bytes(slots.cpu().numpy())
    assert [raw[i * slot:i * slot + n] for i, n in enumerate(out_len.cpu().tolist())] == members and status.cpu().tolist() == [0, 0]
