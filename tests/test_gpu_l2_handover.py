"""Level 2's hand-over between the split path and the fused kernel, on the MI355X (the arithmetic and the inputs:
l2_handover.py, held to the sources and to the twin by test_l2_handover.py on the CPU).

hd_deflate_dynamic.hpp launch_level2 codes a block by one of two codecs that must write the same bytes: parse into a
record in HBM + emit from it, or the fused kernel (its own parse) for a block longer than split_max = min(out_stride,
out_cap), for one whose tokens pass the record's cap_tok, and for all when split_max > 327680.  The twin knows neither,
so it is the one reference for every route.

  * A  the capacity line in one record: T - cap_tok = 0, 1, 2, 63, 64, 65 beside blocks of 0 and 63 bytes and planted ones;
  * B  cap_tok at the tokens stored by a DEFLATE block close and by the whole member, and one less: the overflow in
       step_boundary's own pass, on the pass right behind a close, on the last entry; the same inputs in a room < n;
  * C  the planted-edge corpus of encode_gen.py and two blocks of HD_SEG_LIMIT bytes through both codecs (rooms 327680
       and 327696), which must agree with the twin and with each other;
  * D  2 x 2560 + 40 blocks: the fused kernel's persistent wavefronts take blocks b, b + 2560, b + 5120 of other kinds;
  * E  66000 blocks: overflowing blocks on both sides of the 64512-block launch pair.

Every launch goes through hipdeflate_batch_deflate_dev into slots, a tail, out_len, crc32 and status pre-filled with
sentinels, so that a block neither codec took shows.  Every member: status 0, == the twin's member of the block framed
by encode_room.frame_member, CRC-32 == zlib.crc32, zlib inflates the payload back, nothing written past the room's last
whole dword, and the stall counter does not move.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import encode_room as er
import hdtest
import l2_handover as h

pytestmark = pytest.mark.gpu

GUARD, TAIL = 0xA5, 4096
UNSET = 0x5A5A5A5A                                   # out_len, crc32 and status before the launch


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def _blob(blocks, ragged=True):
    """one buffer: every block 16-byte aligned, but (ragged) every third start at an offset 1..15 mod 16"""
    blob, offs = bytearray(), []
    for i, b in enumerate(blocks):
        blob += bytes(-len(blob) % 16)
        if ragged and i % 3 == 0:
            blob += bytes(1 + (i * 7) % 15)
        offs.append(len(blob))
        blob += b
    blob += bytes(16)
    return np.frombuffer(bytes(blob), dtype=np.uint8), np.array(offs, dtype=np.int64), np.array([len(b) for b in blocks], dtype=np.int32)


def _launch(pkg, src, offs, lens, frame, stride, cap):
    """one level-2 launch of the device API -> (slots and tail, out_len, crc32, status) on the host"""
    import torch
    nb = len(offs)
    d_src, d_off, d_len = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (src, offs, lens))
    out = torch.full((nb * stride + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    olen, crc, st = (torch.full((nb,), UNSET, dtype=torch.int32, device="cuda") for _ in range(3))
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    rc = pkg.lib().hipdeflate_batch_deflate_dev(p(d_src), p(d_off), p(d_len), nb, h.LEVEL, frame, p(out), stride, cap,
                                                p(olen), p(crc), p(st), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), olen.cpu().numpy().view(np.uint32), crc.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _guards(where, nb, stride, cap, hout, hl):
    """nothing past the last whole dword of any room, nor past the last slot; no length beyond the room"""
    bad = []
    edge = (min(stride, cap) + 3) & ~3
    slots = hout[:nb * stride].reshape(nb, stride)
    if edge < stride:
        for i in np.nonzero((slots[:, edge:] != GUARD).any(axis=1))[0][:4]:
            bad.append((where, int(i), "wrote past its room"))
    if (hout[nb * stride:] != GUARD).any():
        bad.append((where, "wrote past the last slot"))
    for i in np.nonzero(hl > min(stride, cap))[0][:4]:
        bad.append((where, int(i), "out_len %#x" % int(hl[i])))
    return bad


def _check_block(where, d, frame, stride, cap, m_slot, olen, crc, st):
    """one block against the twin -> what is wrong, or None"""
    flush = frame == er.RAW_FLUSH
    want = h.model(d, flush).choose(er.payload_room(frame, stride, cap))
    assert want.fits, (where, "the plan put a member in a room that does not hold it")
    if int(st) != 0:
        return (where, "status", int(st))
    if int(olen) > min(stride, cap):
        return (where, "out_len", int(olen))
    m = bytes(m_slot[:int(olen)])
    if m != er.frame_member(frame, want.member, d):
        return (where, "member != twin", len(m), len(want.member))
    if int(crc) != zlib.crc32(d):
        return (where, "crc")
    hdr, trl = er.FRAME_BYTES[frame]
    if zlib.decompressobj(-15).decompress(m[hdr:len(m) - trl] + (b"\x03\x00" if flush else b"")) != d:
        return (where, "zlib does not give the block back")
    return None


def _run(pkg, where, names, blocks, frame, stride, cap, ragged=True):
    """one launch, every block checked -> (what is wrong, the members)"""
    src, offs, lens = _blob(blocks, ragged)
    if ragged:
        assert sum(1 for o in offs if o % 16) >= (len(blocks) + 2) // 3
    hout, hl, hc, hs = _launch(pkg, src, offs, lens, frame, stride, cap)
    nb = len(blocks)
    bad = _guards(where, nb, stride, cap, hout, hl)
    members = []
    for i, d in enumerate(blocks):
        slot = hout[i * stride:(i + 1) * stride]
        e = _check_block((where, names[i]), d, frame, stride, cap, slot, hl[i], hc[i], hs[i])
        if e:
            bad.append(e)
        members.append(bytes(slot[:min(int(hl[i]), stride)]))
    return bad, members


# timeouts: the kernels' share of every test is milliseconds.  What takes time is the first test's start of torch and the
# HIP runtime (about 13 s), the generators (encode_gen's corpus: 8 s) and the twin: 120 s leaves room for a slow core.

@pytest.mark.timeout(120)
@pytest.mark.parametrize("frame", (er.BGZF, er.RAW_FLUSH), ids=("bgzf", "raw_flush"))
def test_a_capacity_line_in_one_record(pkg, frame):
    stalls = pkg.lib().hipdeflate_stall_count()
    a = h.case_a()
    assert h.cap_tok(min(a.stride, a.cap)) == 1001
    bad, _ = _run(pkg, "A", list(a.blocks), list(a.blocks.values()), frame, a.stride, a.cap)
    assert not bad, bad[:12]
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(120)
@pytest.mark.parametrize("frame", (er.RAW, er.RAW_FLUSH), ids=("raw", "raw_flush"))
def test_b_overflow_around_a_close(pkg, frame):
    """one launch per case: the block between two small neighbours (a fitting one in front, an overflowing one behind), so
    that both kernels of the launch pair and the fused kernel have a block of their own beside it"""
    stalls = pkg.lib().hipdeflate_stall_count()
    front, behind = h.filler(700, 901), h.filler(40000, 902)
    bad = []
    cases = h.cases_b()
    assert len(cases) == 46
    for k, c in enumerate(cases):
        names, blocks = ["front", c.name, "behind"], [front, c.data, behind]
        if len(behind) > min(c.stride, c.cap):
            names, blocks = names[:2], blocks[:2]             # (the rooms below the blocks: the case and its small neighbour)
        e, _ = _run(pkg, c.name, names, blocks, frame, c.stride, c.cap, ragged=k % 2 == 0)
        bad += e
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(180)
def test_c_planted_corpus_through_both_codecs(pkg):
    stalls = pkg.lib().hipdeflate_stall_count()
    bl = h.blocks_c()
    names, blocks = list(bl), list(bl.values())
    bad = []
    for frame in (er.RAW, er.RAW_FLUSH):
        got = {}
        for room in (h.C_SPLIT_ROOM, h.C_FUSED_ROOM):
            for lo in range(0, len(blocks), h.C_LAUNCH):
                e, members = _run(pkg, "C room %d" % room, names[lo:lo + h.C_LAUNCH], blocks[lo:lo + h.C_LAUNCH], frame, room, room)
                bad += e
                got.setdefault(room, []).extend(members)
        for i, n in enumerate(names):
            if got[h.C_SPLIT_ROOM][i] != got[h.C_FUSED_ROOM][i]:
                bad.append((n, er.FRAME_NAMES[frame], "the two codecs wrote different members"))
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(120)
def test_d_fused_grid_stride(pkg):
    stalls = pkg.lib().hipdeflate_stall_count()
    data, kinds = h.blocks_d()
    assert len(data) == 2 * h.FUSED_SLOTS + 40
    names = ["%d %s" % (i, k) for i, k in enumerate(kinds)]
    bad, _ = _run(pkg, "D", names, data, er.RAW, h.up16(h.D_CAP), h.D_CAP)
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(180)
def test_e_handover_across_launch_pairs(pkg):
    stalls = pkg.lib().hipdeflate_stall_count()
    nb, bs, room = h.E_BLOCKS, h.E_BYTES, h.E_ROOM
    data = h.data_e()
    src = np.frombuffer(data + bytes(16), dtype=np.uint8)
    offs = np.arange(nb, dtype=np.int64) * bs
    lens = np.full(nb, bs, dtype=np.int32)
    hout, hl, hc, hs = _launch(pkg, src, offs, lens, er.RAW, room, room)
    bad = _guards("E", nb, room, room, hout, hl)
    assert not bad, bad[:12]
    assert not hs.any(), np.nonzero(hs)[0][:12]
    for i in range(nb):
        d = data[i * bs:(i + 1) * bs]
        if int(hc[i]) != zlib.crc32(d):
            bad.append((i, "crc"))
        elif zlib.decompressobj(-15).decompress(bytes(hout[i * room:i * room + int(hl[i])])) != d:
            bad.append((i, "zlib does not give the block back"))
    for i in h.e_checked():
        e = _check_block(("E", i), data[i * bs:(i + 1) * bs], er.RAW, room, room, hout[i * room:(i + 1) * room], hl[i], hc[i], hs[i])
        if e:
            bad.append(e)
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls
