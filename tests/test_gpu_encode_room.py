"""Every encode path held to its output room at each fit edge (the model: encode_room.py, pinned against the twin by
test_encode_room.py).

include/hipdeflate.h: member i goes to out + i*out_stride, at most min(out_stride, out_cap) bytes are written, status 1
= does not fit.  The room decides the stored fallback, the latency or the ordinary form, the BGZF clamp, the segment
slots per block and the segment rounds; here every one of those is run at the rooms where its answer changes, with
out_cap != out_stride, and the status, the member and the CRC are held to the model."""
import collections
import ctypes
import zlib

import numpy as np
import pytest

import encode_room as er
import hdtest
from test_encode_room import big_blocks, blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def up16(v):
    return (v + 15) & ~15


def _pack(datas):
    blob, offs, lens = bytearray(), [], []
    for i, d in enumerate(datas):
        blob += bytes((-len(blob) % 16) + (i % 3))         # every third start aligned, the others not
        offs.append(len(blob))
        lens.append(len(d))
        blob += d
    return np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8), np.array(offs, np.uint64), np.array(lens, np.uint32)


def batch(pkg, packed, level, frame, stride, cap):
    """hipdeflate_batch_deflate with its own stride and cap -> (members, crc, status)"""
    src, offs, lens = packed
    nb = len(offs)
    out = np.zeros(max(nb * stride, 1), dtype=np.uint8)
    olen, crc, st = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32), np.full(nb, -7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
    rc = pkg.lib().hipdeflate_batch_deflate(p(src), p(offs), p(lens), nb, level, frame, p(out), stride, cap,
                                            p(olen), p(crc), p(st))
    assert rc == 0, rc
    return [bytes(out[i * stride: i * stride + int(olen[i])]) for i in range(nb)], crc, st


_MODELS = {}


def model(data, level, flush):
    """one twin call per block, level and form: every room's expectation comes from it (cached by the block's bytes)"""
    k = (hdtest.sha(data), level, flush)
    if k not in _MODELS:
        _MODELS[k] = er.Block(data, level, flush)
    return _MODELS[k]


def check_launch(pkg, names, datas, models, level, frame, latency, stride, cap, packed=None, device=True):
    packed = packed if packed is not None else _pack(datas)
    members, crc, st = batch(pkg, packed, level, frame | (er.LATENCY if latency else 0), stride, cap)
    room = er.payload_room(frame, stride, cap)
    bad = []
    for i, (n, d, b) in enumerate(zip(names, datas, models)):
        want = b.choose(room, latency, device=device)
        if int(st[i]) != (0 if want.fits else 1):
            bad.append((n, "status", int(st[i]), want.kind, room, b.need, b.need_lat))
            continue
        if not want.fits:
            continue
        if members[i] != er.frame_member(frame, want.member, d):
            bad.append((n, "member", want.kind, room, len(members[i]), len(want.member)))
        if int(crc[i]) != zlib.crc32(d):
            bad.append((n, "crc", room))
    return bad


# every frame at levels 0, 1, 2, 3, 6; RAW / RAW_FLUSH at every level
CASES = [(f, lv) for f in (er.RAW, er.RAW_FLUSH, er.BGZF, er.MIGZ, er.ZLIB, er.GZIP) for lv in (0, 1, 2, 3, 6)] + \
        [(f, lv) for f in (er.RAW, er.RAW_FLUSH) for lv in (4, 5, 7, 8, 9)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("frame,level", CASES, ids=["%s-l%d" % (er.FRAME_NAMES[f], lv) for f, lv in CASES])
def test_batch_at_every_edge_room(pkg, frame, level):
    """one launch per distinct edge room, all blocks in it; stride = up16(room), cap = the room itself"""
    stalls = pkg.lib().hipdeflate_stall_count()
    flush = frame == er.RAW_FLUSH
    bl = dict(blocks())
    if frame in (er.RAW, er.RAW_FLUSH) and level <= 3:
        bl.update(big_blocks())
    names, datas = list(bl), list(bl.values())
    models = [model(d, level, flush) for d in datas]
    packed = _pack(datas)
    hdr, trl = er.FRAME_BYTES[frame]
    bad = []
    for latency in (False, True):
        rooms = sorted({r for b in models for r in b.edge_rooms(latency)})
        for room in rooms:
            total = room + hdr + trl
            if total <= 0 or (frame == er.BGZF and total > er.BGZF_MAX):
                continue                                    # (above the clamp: test_bgzf_rooms_above_the_clamp)
            bad += [(latency, total) + x for x in
                    check_launch(pkg, names, datas, models, level, frame, latency, up16(total), total, packed)]
    assert not bad, (_tally(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


def _tally(bad):
    """{(latency, what[, status got, form wanted]): count} of a test's mismatches"""
    return dict(collections.Counter((b[0], b[3]) + ((b[4], b[5]) if b[3] == "status" else ()) for b in bad))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", range(10))
def test_bgzf_rooms_above_the_clamp(pkg, level):
    """stride / cap above 65536: every BGZF member is held to 65536 bytes -- the 65505 / 65506-byte random edge of
    the stored form and the compressible blocks whose latency worst case crosses the clamp"""
    s = hdtest.synth()
    rnd = bytes(s.random_bytes(65506))
    bl = {"random_65505": rnd[:65505], "random_65506": rnd}
    for n in (65338, 65339, 65418, 65419, 65500, 65536):
        bl["zeros_%d" % n] = bytes(n)
    bl["fastq_65536"] = bytes(s.fastq_like(65536))
    names, datas = list(bl), list(bl.values())
    models = [model(d, level, False) for d in datas]
    packed = _pack(datas)
    stalls = pkg.lib().hipdeflate_stall_count()
    bad = []
    for latency in (False, True):
        for total in er.bgzf_clamp_rooms():
            for stride, cap in ((up16(total), total), (up16(total), 0xffffffff), (up16(total) + 65536, total)):
                bad += [(latency, stride, cap) + x for x in
                        check_launch(pkg, names, datas, models, level, er.BGZF, latency, stride, cap, packed)]
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", range(10))
def test_per_call_codecs_at_edge_rooms(pkg, level):
    """hip_deflate / hip_deflate_flush at every edge room, straddling the routes' thresholds (need_lat, need_st): the
    per-call codecs are the twin's latency forms at the caller's room"""
    stalls = pkg.lib().hipdeflate_stall_count()
    bad = []
    for name, d in blocks().items():
        for flush in (False, True):
            b = model(d, level, flush)
            for room in b.edge_rooms(latency=True):
                want = b.choose(room, latency=True)
                r, m = (pkg.hip_deflate_flush if flush else pkg.hip_deflate)(d, level, cap=room)
                if (r == 0) != want.fits or (want.fits and m != want.member):
                    bad.append((name, flush, room, r, want.kind, len(m), b.need, b.need_lat))
    assert not bad, bad[:12]
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- device API: slots with a guard behind them ----------------------------------------------------------------

GUARD = 0xA5
TAIL = 4096


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", [0, 1, 2, 3, 6])
def test_device_api_writes_nothing_past_its_room(pkg, level):
    """hipdeflate_batch_deflate_dev with cap % 4 in {0, 1, 2, 3} and stride = up16(cap) + 16..64: every slot and a
    4 KiB tail filled with 0xA5 beforehand; nothing may change at or past the room's last whole dword, nor past the
    last slot; status and member as the model says (levels >= 3: a block longer than min(stride, cap) is refused)"""
    import torch
    stalls = pkg.lib().hipdeflate_stall_count()
    bl = blocks()
    names, datas = list(bl), list(bl.values())
    packed = _pack(datas)
    src = torch.from_numpy(packed[0].copy()).cuda()
    off = torch.from_numpy(packed[1].astype(np.int64)).cuda()
    ln = torch.from_numpy(packed[2].astype(np.int32)).cuda()
    nb = len(names)
    bad, grazed = [], 0
    for frame in (er.RAW, er.RAW_FLUSH, er.BGZF, er.GZIP):
        flush = frame == er.RAW_FLUSH
        models = [model(d, level, flush) for d in datas]
        hdr, trl = er.FRAME_BYTES[frame]
        for latency in (False, True):
            # rooms at the fit edges, every residue mod 4 among them
            rooms = sorted({r + hdr + trl for b in models for r in b.edge_rooms(latency)[:4]} |
                           {1021 + hdr + trl, 4094 + hdr + trl, 40003 + hdr + trl})
            for j, cap in enumerate(rooms):
                if cap <= 0 or (frame == er.BGZF and cap > er.BGZF_MAX):
                    continue
                stride = up16(cap) + 16 * (1 + j % 4)
                out = torch.full((nb * stride + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
                olen = torch.zeros(nb, dtype=torch.int32, device="cuda")
                crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
                st = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
                rc = pkg.lib().hipdeflate_batch_deflate_dev(
                    ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(ln.data_ptr()), nb,
                    level, frame | (er.LATENCY if latency else 0), ctypes.c_void_p(out.data_ptr()), stride, cap,
                    ctypes.c_void_p(olen.data_ptr()), ctypes.c_void_p(crc.data_ptr()), ctypes.c_void_p(st.data_ptr()), None)
                assert rc == 0, rc
                torch.cuda.synchronize()
                h = out.cpu().numpy()
                hl, hs, hc = olen.cpu().numpy().view(np.uint32), st.cpu().numpy(), crc.cpu().numpy().view(np.uint32)
                room = er.payload_room(frame, stride, cap)
                edge = min(stride, cap)
                for i, (n, d, b) in enumerate(zip(names, datas, models)):
                    slot = h[i * stride:(i + 1) * stride]
                    touched = np.nonzero(slot[edge:] != GUARD)[0]
                    if len(touched):
                        last = edge + int(touched[-1])
                        if last >= (edge + 3) & ~3:
                            bad.append((n, frame, latency, cap, stride, "wrote byte %d of the slot" % last))
                        grazed += 1
                    want = b.choose(room, latency, device=True)
                    if level >= er.WG_LEVEL and len(d) > edge:
                        want = er.Choice(False, None, None)
                    if int(hs[i]) != (0 if want.fits else 1):
                        bad.append((n, frame, latency, cap, "status", int(hs[i]), want.kind))
                    elif want.fits and bytes(slot[:int(hl[i])]) != er.frame_member(frame, want.member, d):
                        bad.append((n, frame, latency, cap, "member", want.kind))
                    elif want.fits and int(hc[i]) != zlib.crc32(d):
                        bad.append((n, frame, latency, cap, "crc"))
                if (h[nb * stride:] != GUARD).any():
                    bad.append((frame, latency, cap, "wrote past the last slot"))
    print("members that wrote into the room's last partial dword:", grazed)
    assert not bad, bad[:12]
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- segment rounds ----------------------------------------------------------------------------------------------

def _distinct_blocks(nb, n, seed=7):
    """nb blocks of n bytes of FASTQ-like data, no two neighbours alike (windows of a 6 MB sample)"""
    s = hdtest.synth()
    base = np.asarray(s.fastq_like(6 << 20), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, len(base) - n, nb)
    return np.concatenate([base[a:a + n] for a in starts])


def _seg_slots(slot, seg):
    """hd_segment.hpp seg_slots_per_block: the segment slots per block of a launch whose room is `slot`"""
    full = er.stored_size(seg) + 5
    return slot // full + (1 if slot % full >= 11 else 0)


def _deflate_dev(pkg, data, off, ln, level, frame, stride, cap):
    """hipdeflate_batch_deflate_dev on torch tensors -> (slots, out_len, crc32, status); unlike the host batch call, which
    shrinks its device slot to hipdeflate_bound(longest block), the device call codes in the caller's slot"""
    import torch
    nb = off.numel()
    out = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    olen = torch.zeros(nb, dtype=torch.int32, device="cuda")
    crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    st = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    rc = pkg.lib().hipdeflate_batch_deflate_dev(vp(data), vp(off), vp(ln), nb, level, frame, vp(out), stride, cap,
                                                vp(olen), vp(crc), vp(st), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, olen, crc, st


def _inflate_back(pkg, out, stride, olen, crc, data, off, ln, hdr=0, trl=0):
    """every member inflated on the device: the input back byte for byte, the decoder's CRC-32 = the encoder's"""
    import importlib
    import torch
    dev = importlib.import_module("7bgzf_amd.device")
    nb = off.numel()
    back = torch.empty_like(data)
    b_len = torch.zeros(nb, dtype=torch.int32, device="cuda")
    b_crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    b_st = torch.ones(nb, dtype=torch.int32, device="cuda")
    in_off = torch.arange(nb, dtype=torch.int64, device="cuda") * stride + hdr
    dev.device_inflate(out, in_off, (olen - hdr - trl).to(torch.int32), back, off, ln, b_len, b_crc, b_st)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(b_st)) == 0
    assert torch.equal(b_len, ln) and torch.equal(back, data) and torch.equal(b_crc, crc)


def _latency_rounds(pkg, level, nb, slot, rb_expected, S_expected):
    """nb blocks of 0xff00 in latency form, slot = out_stride = out_cap: every member inflated back and its CRC-32
    against zlib's, the twin on the members at the rounds' edges"""
    import torch
    n, lat = 0xff00, er.LAT_SEG[level]
    assert er.seg_worst(n, lat, False) <= slot
    S = _seg_slots(slot, lat)
    assert S == S_expected and 65536 // S == rb_expected and nb > rb_expected
    stalls = pkg.lib().hipdeflate_stall_count()
    host = _distinct_blocks(nb, n)
    data = torch.from_numpy(host).cuda()
    off = torch.arange(nb, dtype=torch.int64, device="cuda") * n
    ln = torch.full((nb,), n, dtype=torch.int32, device="cuda")
    out, olen, crc, st = _deflate_dev(pkg, data, off, ln, level, er.RAW | er.LATENCY, slot, slot)
    assert int(torch.count_nonzero(st)) == 0
    _inflate_back(pkg, out, slot, olen, crc, data, off, ln)
    hc = crc.cpu().numpy().view(np.uint32)
    assert [i for i in range(nb) if int(hc[i]) != zlib.crc32(host[i * n:(i + 1) * n])] == []
    sizes = olen.cpu().numpy()
    for i in sorted({0, rb_expected - 1, rb_expected, nb - 1}):
        m = out[i * slot: i * slot + int(sizes[i])].cpu().numpy().tobytes()
        assert hdtest.codec_twin(host[i * n:(i + 1) * n].tobytes(), level, cap=slot) == (0, m), i
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(600)
def test_latency_segment_rounds_level1(pkg):
    """3856 blocks of 0xff00 in 65536-byte slots: S = 17 slots per block, 3855 blocks per round -- two rounds of
    k_seg_finish"""
    _latency_rounds(pkg, 1, 3856, 65536, 3855, 17)


@pytest.mark.timeout(600)
def test_latency_segment_rounds_level2(pkg):
    """7282 blocks of 0xff00 at level 2 in 65536-byte slots: S = 9, 7281 blocks per round -- two rounds"""
    _latency_rounds(pkg, 2, 7282, 65536, 7281, 9)


@pytest.mark.timeout(600)
def test_latency_stitch_path_over_two_rounds(pkg):
    """257 blocks of 0xff00 in 1 MiB slots at level 1: S = 257 > 64 slots per block, so k_seg_stitch + k_compact
    instead of k_seg_finish, and 255 blocks per round -- two rounds"""
    _latency_rounds(pkg, 1, 257, 1 << 20, 255, 257)


@pytest.mark.timeout(900)
def test_throughput_segment_rounds_on_the_device_api(pkg):
    """level 1 MiGz, 3856 blocks of 1 MiB in hipdeflate_bound(1 MiB, 1) slots: 17 segment slots per block, two rounds
    (about 12 GB of HBM).  Checked by device inflate + torch.equal and CRC, and the twin at the rounds' edges"""
    import torch
    stalls = pkg.lib().hipdeflate_stall_count()
    nb, n = 3856, 1 << 20
    stride = int(pkg.lib().hipdeflate_bound(n, 1))
    S = _seg_slots(stride, er.SEG_BYTES)
    rb = 65536 // S
    assert S == 17 and rb == 3855
    tile = torch.from_numpy(np.asarray(hdtest.synth().fastq_like(64 << 20), dtype=np.uint8)).cuda()
    data = tile.repeat(nb * n // tile.numel() + 1)[:nb * n]
    del tile
    off = torch.arange(nb, dtype=torch.int64, device="cuda") * n
    ln = torch.full((nb,), n, dtype=torch.int32, device="cuda")
    out, olen, crc, st = _deflate_dev(pkg, data, off, ln, 1, er.MIGZ, stride, stride)
    assert int(torch.count_nonzero(st)) == 0
    hdr, trl = er.FRAME_BYTES[er.MIGZ]
    _inflate_back(pkg, out, stride, olen, crc, data, off, ln, hdr, trl)
    sizes = olen.cpu().numpy()
    for i in (0, rb - 1, rb, nb - 1):
        m = out[i * stride: i * stride + int(sizes[i])].cpu().numpy().tobytes()
        d = data[i * n:(i + 1) * n].cpu().numpy().tobytes()
        r, twin = hdtest.oracle_twin(d, 1, cap=stride - hdr - trl)
        assert r == 0 and m == er.frame_member(er.MIGZ, twin, d), i
    assert pkg.lib().hipdeflate_stall_count() == stalls
