"""The PER-BLOCK schedule of levels 3..9 on the MI355X, at every launch shape and cut: HD_FRAME_LATENCY with no block longer
than 64 KiB -- k_stage_in, k_parse_wg shared by 4 or 2 workgroups (hd_deflate_wg.hpp), k_emit_wg (hd_emit_wg.hpp) -- on the
blocks of tests/wg_block_gen.py, whose point test_wg_block_gen.py pins on the CPU.  It is what an unset BGZF_METHOD, hip_deflate,
hip_deflate_flush and every hipdeflate_lat_* context run.

Expected values are exact everywhere: the member's payload == hdtest.codec_twin(block, level, cap = the payload's room)
(RAW_FLUSH: codec_twin_flush), CRC-32 == zlib.crc32, status 0, zlib inflates the payload to the block; where the twin says
"does not fit", status 1 and out_len 0.  A payload must also be the same bytes in every launch that wrote it, whatever the
number of sharers.  The stall counter does not move.

Which paths a test runs follows from launch_wg's arithmetic (a sub-batch of n blocks: wg_split = 4 for n <= 64, 2 for
n <= 128, else 1; wg_split > 1 stages the blocks and parses from the staged copies) and from the members' DEFLATE block
counts (k_emit_wg: four to a round; `cuts` holds members of 4, 5, 6, 7, 8 and 10):
  * launch shapes (a)       wg_split 4 (1, 2, 63, 64 blocks), 2 (65, 127, 128), 1 unstaged (129, 300); emit rounds 1..3;
                            with a 65537-byte block in the launch: the throughput kernels;
  * sub-batches (b)         130 + 130 + 40: unstaged, unstaged, staged x 4 over one scratch area; 100 x 3: staged x 2;
                            64 x 4 + 44: staged x 4; emit rounds 1..3;
  * device API (c)          k_stage_in's unaligned loads at wg_split 4 (64 blocks) and 2 (65), unstaged unaligned parse
                            (129); the same launches at out_cap 65552: the throughput kernels;
  * verdict (d)             "does not fit" reached in emit round 2 and at the member's last byte, wg_split 4 (hip_deflate)
                            and 2 (65 blocks);
  * latency contexts (e)    staged from pinned memory at wg_split 4 and 2, unstaged (129, 160), a small run behind a
                            large one; a context of 65537-byte blocks: the throughput kernels.
"""
import ctypes
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import encode_room as er
import hdtest
import wg_block_gen as wg

pytestmark = pytest.mark.gpu

LEVELS = (3, 4, 5, 6)
SLOT = 65536
FRAMES = (er.RAW, er.RAW_FLUSH, er.BGZF, er.MIGZ, er.GZIP, er.ZLIB)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 300)
GUARD, TAIL = 0xA5, 4096


def wg_split(n):
    """hd_deflate_wg.hpp launch_wg, a.lat: the workgroups that share a block's parse in a sub-batch of n blocks"""
    return 4 if n <= 64 else 2 if n <= 128 else 1


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


class Pool:
    """the blocks by name, the twin of each (block, level, form, room) computed once, and every payload a launch wrote"""

    def __init__(self):
        self.names = [c.name for c in wg.cached_corpus()]
        self.data = {c.name: c.data for c in wg.cached_corpus()}
        self.data["text_65537"] = bytes(hdtest.synth().text_like(65537, seed=31))
        self.perm = [self.names[i] for i in np.random.default_rng(5).permutation(len(self.names))]
        self.twins = {}
        self.wrote = {}                                # (name, level, flush) -> the payload, from the first launch that wrote it

    def deal(self, start, n):
        """n blocks from the whole pool by the fixed permutation, from position `start` on"""
        return [self.perm[(start + i) % len(self.perm)] for i in range(n)]

    def _one(self, key):
        name, level, flush, room = key
        return (hdtest.codec_twin_flush if flush else hdtest.codec_twin)(self.data[name], level, cap=room)

    def want(self, keys):
        missing = sorted({k for k in keys if k not in self.twins})
        if missing:
            hdtest.oracle()
            with ThreadPoolExecutor(16) as ex:
                for k, v in zip(missing, ex.map(self._one, missing)):
                    self.twins[k] = v

    def check(self, where, names, level, frame, stride, cap, members, crc, st):
        """every member of a launch against the twin at the launch's room -> the list of what is wrong"""
        flush = frame == er.RAW_FLUSH
        room = er.payload_room(frame, stride, cap)
        hdr, trl = er.FRAME_BYTES[frame]
        self.want([(n, level, flush, room) for n in names])
        bad = []
        for i, n in enumerate(names):
            d, m = self.data[n], members[i]
            r, twin = self.twins[(n, level, flush, room)]
            if r != 0:
                if int(st[i]) != 1 or len(m) != 0:
                    bad.append((where, n, "the twin says it does not fit", int(st[i]), len(m)))
                continue
            payload = m[hdr:len(m) - trl]
            if int(st[i]) != 0:
                bad.append((where, n, "status", int(st[i])))
            elif payload != twin:
                bad.append((where, n, "payload != twin", len(payload), len(twin)))
            elif (int(crc[i]) & 0xffffffff) != zlib.crc32(d):
                bad.append((where, n, "crc"))
            elif zlib.decompressobj(-15).decompress(payload + (b"\x03\x00" if flush else b"")) != d:
                bad.append((where, n, "zlib does not give the block back"))
            elif m != er.frame_member(frame, twin, d) or not _frame_fields_ok(frame, m, d):
                bad.append((where, n, "frame", er.FRAME_NAMES[frame]))
            elif self.wrote.setdefault((n, level, flush), payload) != payload:
                bad.append((where, n, "another launch wrote other bytes"))
        return bad


def _frame_fields_ok(frame, m, d):
    """the frame's size field and trailer, read from the member itself"""
    u32 = lambda b: int.from_bytes(b, "little")        # noqa: E731
    if frame in (er.BGZF, er.MIGZ, er.GZIP) and (u32(m[-8:-4]) != zlib.crc32(d) or u32(m[-4:]) != len(d)):
        return False
    if frame == er.BGZF:
        return u32(m[16:18]) == len(m) - 1 and len(m) <= 65536
    if frame == er.MIGZ:
        return u32(m[16:20]) == len(m) - 20 - 8
    if frame == er.ZLIB:
        return int.from_bytes(m[-4:], "big") == zlib.adler32(d) and (m[0] * 256 + m[1]) % 31 == 0
    return True


@pytest.fixture(scope="module")
def pool():
    return Pool()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _blob(blocks, ragged=False):
    """one buffer: every block 16-byte aligned, or (ragged) every third start at an offset 1..15 mod 16"""
    blob, offs = bytearray(), []
    for i, b in enumerate(blocks):
        blob += bytes(-len(blob) % 16)
        if ragged and i % 3 == 0:
            blob += bytes(1 + (i * 7) % 15)
        offs.append(len(blob))
        blob += b
    blob += bytes(16)
    return np.frombuffer(bytes(blob), dtype=np.uint8), np.array(offs, dtype=np.uint64), np.array([len(b) for b in blocks], dtype=np.uint32)


def _host(pkg, blocks, level, frame, stride=SLOT, cap=SLOT):
    """hipdeflate_batch_deflate -> (members, crc, status)"""
    src, offs, lens = _blob(blocks)
    nb = len(blocks)
    out = np.zeros(nb * stride, dtype=np.uint8)
    olen, crc, st = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32), np.full(nb, -7, dtype=np.int32)
    rc = pkg.lib().hipdeflate_batch_deflate(_vp(src), _vp(offs), _vp(lens), nb, level, frame, _vp(out), stride, cap,
                                            _vp(olen), _vp(crc), _vp(st))
    assert rc == 0, rc
    return [bytes(out[i * stride:i * stride + int(olen[i])]) for i in range(nb)], crc, st


# ---- (a) launch shapes, host API ---------------------------------------------------------------------------------------
# timeouts: measured on an MI355X machine with 16 CPUs, the module takes 19 s: 13 s are the first test that brings up
# torch and the HIP runtime, 2 s the generator, every other test 0.05 .. 0.45 s.  The part that does not depend on the
# kernels is the twins of the pool -- 2,016 calls for the host-API tests, 37 s on ONE thread -- and the generator (6 s), so
# 120 s per test leaves room for a machine that gives the twins a single slow core and for the runtime's start.

@pytest.mark.timeout(120)
@pytest.mark.parametrize("level", LEVELS)
def test_every_launch_shape_writes_the_twin(pkg, pool, level):
    stalls = pkg.lib().hipdeflate_stall_count()
    bad, start = [], 7 * level
    met = {n: set() for n in pool.names}               # the sharer counts each block met in a non-flush launch
    for k, count in enumerate(COUNTS):
        frame = FRAMES[(k + LEVELS.index(level)) % len(FRAMES)]
        names = pool.deal(start, count)
        start += count
        members, crc, st = _host(pkg, [pool.data[n] for n in names], level, frame | er.LATENCY)
        bad += pool.check("%d blocks" % count, names, level, frame, SLOT, SLOT, members, crc, st)
        if frame != er.RAW_FLUSH:
            for n in names:
                met[n].add(wg_split(count))
    assert all(s == {4, 2, 1} for s in met.values()), "the dealing no longer brings every block to every split"
    # one block longer than 64 KiB: the whole launch goes to the throughput kernels, and the other 64 members stay as they are
    names = pool.deal(start, 64)
    names.insert(33, "text_65537")
    members, crc, st = _host(pkg, [pool.data[n] for n in names], level, er.RAW | er.LATENCY)
    bad += pool.check("64 blocks and one of 65537 bytes", names, level, er.RAW, SLOT, SLOT, members, crc, st)
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(120)
def test_level_9_takes_level_6s_path(pkg, pool):
    stalls = pkg.lib().hipdeflate_stall_count()
    names = pool.deal(11, 65)
    members, crc, st = _host(pkg, [pool.data[n] for n in names], 9, er.BGZF | er.LATENCY)
    bad = pool.check("level 9", names, 9, er.BGZF, SLOT, SLOT, members, crc, st)
    pool.want([(n, 6, False, SLOT - 26) for n in names])
    for i, n in enumerate(names):
        if st[i] == 0 and members[i][18:-8] != pool.twins[(n, 6, False, SLOT - 26)][1]:
            bad.append((n, "level 9 != level 6"))
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- (b) several sub-batches -------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
@pytest.mark.parametrize("level", (3, 6))
def test_sub_batches_of_every_kind_over_one_scratch_area(pkg, pool, level):
    """hipdeflate_test_beside caps the sub-batch: 300 blocks as 130 + 130 + 40 (unstaged, unstaged, staged with four sharers:
    the staging area behind records sized for 130), 100 + 100 + 100 (two sharers) and 64 x 4 + 44 (four)"""
    stalls = pkg.lib().hipdeflate_stall_count()
    bad = []
    try:
        for sub_cap in (130, 100, 64):
            pkg.lib().hipdeflate_test_beside(3, sub_cap)
            names = pool.deal(sub_cap, 300)
            members, crc, st = _host(pkg, [pool.data[n] for n in names], level, er.RAW | er.LATENCY)
            bad += pool.check("sub-batches of %d" % sub_cap, names, level, er.RAW, SLOT, SLOT, members, crc, st)
    finally:
        pkg.lib().hipdeflate_test_beside(3, 0)
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- (c) device API, unaligned -----------------------------------------------------------------------------------------

def _dev(pkg, torch, src, off, ln, level, frame, stride, cap):
    """hipdeflate_batch_deflate_dev into slots and a tail filled with GUARD -> (the slots and tail on the host, out_len, crc, status)"""
    nb = off.numel()
    out = torch.full((nb * stride + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    olen = torch.zeros(nb, dtype=torch.int32, device="cuda")
    crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    st = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    rc = pkg.lib().hipdeflate_batch_deflate_dev(p(src), p(off), p(ln), nb, level, frame, p(out), stride, cap, p(olen), p(crc), p(st), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), olen.cpu().numpy().view(np.uint32), crc.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _dev_check(pool, where, names, level, stride, cap, h, hl, hc, hs):
    nb = len(names)
    members = [bytes(h[i * stride:i * stride + int(hl[i])]) for i in range(nb)]
    bad = pool.check(where, names, level, er.RAW, stride, cap, members, hc, hs)
    edge = min(stride, cap)                            # (a multiple of 4 here: its last whole dword ends at it)
    for i, n in enumerate(names):
        if (h[i * stride + edge:(i + 1) * stride] != GUARD).any():
            bad.append((where, n, "wrote past its room"))
    if (h[nb * stride:] != GUARD).any():
        bad.append((where, "wrote past the last slot"))
    return bad


@pytest.mark.timeout(120)
@pytest.mark.parametrize("level", (3, 6))
def test_device_api_unaligned_blocks_in_both_schedules(pkg, pool, level):
    import torch
    stalls = pkg.lib().hipdeflate_stall_count()
    bad = []
    for count in (64, 65, 129):
        names = pool.deal(3 * count, count)
        src, offs, lens = _blob([pool.data[n] for n in names], ragged=True)
        assert sum(1 for o in offs if o % 16) >= count // 3
        d_src = torch.from_numpy(src.copy()).cuda()
        d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
        d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
        # out_cap 65536: no block can be longer than 64 KiB, the per-block schedule; out_cap 65552: the throughput kernels
        for stride, cap in ((65552, 65536), (65552, 65552)):
            h, hl, hc, hs = _dev(pkg, torch, d_src, d_off, d_len, level, er.RAW | er.LATENCY, stride, cap)
            bad += _dev_check(pool, "%d blocks, cap %d" % (count, cap), names, level, stride, cap, h, hl, hc, hs)
    # a block longer than its slot is refused, and its neighbours do not notice
    names = pool.deal(40, 7)
    names.insert(3, "text_65537")
    src, offs, lens = _blob([pool.data[n] for n in names], ragged=True)
    h, hl, hc, hs = _dev(pkg, torch, torch.from_numpy(src.copy()).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(),
                         torch.from_numpy(lens.astype(np.int32)).cuda(), level, er.RAW | er.LATENCY, 65552, 65536)
    assert int(hs[3]) != 0 and int(hl[3]) == 0, (int(hs[3]), int(hl[3]))
    keep = [i for i in range(len(names)) if i != 3]
    members = [bytes(h[i * 65552:i * 65552 + int(hl[i])]) for i in keep]
    bad += pool.check("beside a refused block", [names[i] for i in keep], level, er.RAW, 65552, 65536, members, hc[keep], hs[keep])
    if (h[len(names) * 65552:] != GUARD).any():
        bad.append("wrote past the last slot")
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- (d) the verdict in round two --------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
@pytest.mark.parametrize("level", (3, 6))
def test_the_verdict_of_a_seven_block_member(pkg, pool, level):
    """a member of 7 DEFLATE blocks in a room of exactly its length, one byte less, and one byte less than its fifth block
    needs (k_emit_wg finds out in its second round): status and bytes are the twin's"""
    import deflate_tokens
    stalls = pkg.lib().hipdeflate_stall_count()
    block = pool.data["cut7"]
    r, whole = hdtest.codec_twin(block, level)
    blocks = deflate_tokens.read(whole, expand=False).blocks
    assert r == 0 and len(blocks) == 7
    rooms = (len(whole), len(whole) - 1, (blocks[4].end_bit + 7) // 8 - 1)
    others = [n for n in pool.deal(9, 65) if n != "cut7"][:64]
    bad = []
    for room in rooms:
        r, twin = hdtest.codec_twin(block, level, cap=room)
        print("level %d, room %d of %d: the twin answers %d" % (level, room, len(whole), r))
        assert (r == 0) == (room == len(whole))
        got = pkg.hip_deflate(block, level, cap=room)
        if got != ((0, twin) if r == 0 else (1, b"")):
            bad.append(("hip_deflate", room, got[0], len(got[1])))
        names = others[:20] + ["cut7"] + others[20:]
        members, crc, st = _host(pkg, [pool.data[n] for n in names], level, er.RAW | er.LATENCY, stride=SLOT, cap=room)
        bad += pool.check("65 blocks, out_cap %d" % room, names, level, er.RAW, SLOT, room, members, crc, st)
        if (int(st[20]), members[20]) != ((0, twin) if r == 0 else (1, b"")):
            bad.append(("batch", room, int(st[20]), len(members[20])))
    assert not bad, (len(bad), bad[:12])
    assert pkg.lib().hipdeflate_stall_count() == stalls


# ---- (e) latency contexts ----------------------------------------------------------------------------------------------

def _lat_run(pkg, c, blocks):
    L = pkg.lib()
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    for i, b in enumerate(blocks):
        if b:
            ctypes.memmove(L.hipdeflate_lat_input(c, i), b, len(b))
    assert L.hipdeflate_lat_run(c, _vp(lens), len(blocks)) == 0
    members, crcs, sts = [], [], []
    for i in range(len(blocks)):
        n, crc, st = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int32()
        p = L.hipdeflate_lat_output(c, i, ctypes.byref(n), ctypes.byref(crc), ctypes.byref(st))
        members.append(ctypes.string_at(p, n.value))
        crcs.append(crc.value)
        sts.append(st.value)
    return members, crcs, sts


@pytest.mark.timeout(120)
@pytest.mark.parametrize("level", (3, 6))
def test_latency_context_runs_of_every_shape(pkg, pool, level):
    L = pkg.lib()
    stalls = L.hipdeflate_stall_count()
    bad, start = [], 5 * level
    c = L.hipdeflate_lat_open(level, er.BGZF | er.LATENCY, 160, 65536)
    big = L.hipdeflate_lat_open(level, er.BGZF | er.LATENCY, 160, 65537)       # blocks that may be longer than 64 KiB: the throughput kernels
    assert c and big
    try:
        assert L.hipdeflate_lat_input(c, 160) is None and L.hipdeflate_lat_input(c, 159)
        for count in (1, 64, 65, 128, 129, 160, 3):
            names = pool.deal(start, count)
            start += count
            members, crc, st = _lat_run(pkg, c, [pool.data[n] for n in names])
            bad += pool.check("run of %d" % count, names, level, er.BGZF, SLOT, SLOT, members, crc, st)
            if count in (64, 160, 3):
                m2, crc2, st2 = _lat_run(pkg, big, [pool.data[n] for n in names])
                bad += pool.check("run of %d, throughput kernels" % count, names, level, er.BGZF, SLOT, SLOT, m2, crc2, st2)
                if m2 != members:
                    bad.append(("run of %d" % count, "the two contexts wrote different members"))
    finally:
        L.hipdeflate_lat_close(c)
        L.hipdeflate_lat_close(big)
    assert not bad, (len(bad), bad[:12])
    assert L.hipdeflate_stall_count() == stalls
