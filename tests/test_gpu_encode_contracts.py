"""The encoder's stated rules on the KERNELS' members (the CPU side: test_encode_contracts.py).

The planted corpus (encode_gen.py) and corpus_small go through every device entry point that writes raw DEFLATE:
batch_deflate at levels 0..9 in HD_FRAME_RAW and HD_FRAME_RAW_FLUSH, each with and without HD_FRAME_LATENCY;
hip_deflate / hip_deflate_flush from 1, 2 and 4 threads at once, so that latency launches carry several blocks;
and one run through the device-resident path (device.DeviceDeflate) for its slot layout.  Every member must be
clean under encode_contracts.check, equal to the twin, and come back whole through zlib and the oracle.
"""
import threading
import zlib

import numpy as np
import pytest

import encode_contracts as ec
import encode_gen
import hdtest

pytestmark = pytest.mark.gpu

TWIN = {"plain": hdtest.oracle_twin, "flush": hdtest.oracle_twin_flush,
        "lat": hdtest.codec_twin, "lat_flush": hdtest.codec_twin_flush}


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def inputs():
    out = [(c.family + "/" + c.name, c.data) for c in encode_gen.cached_corpus()]
    out += [("small/" + k, v) for k, v in hdtest.corpus_small().items()]
    return out


def _pack(inputs):
    """one blob, every third start unaligned"""
    blob, offs, lens = bytearray(), [], []
    for i, (_, d) in enumerate(inputs):
        blob += bytes((i * 7) % 16 if i % 3 == 0 else -len(blob) % 16)
        offs.append(len(blob))
        lens.append(len(d))
        blob += d
    return bytes(blob), offs, lens


def _verify(items):
    """items: (name, member, data, level, form, room) -> asserts member == twin, zlib and the oracle give the input
    back, and no rule is broken"""
    for name, m, d, level, form, room in items:
        r, twin = TWIN[form](d, level, cap=room)
        assert r == 0 and m == twin, (name, level, form, len(m), len(twin))
        flush = form.endswith("flush")
        back = zlib.decompressobj(-15).decompress(m + (b"\x03\x00" if flush else b""))
        assert back == d, (name, level, form)
        r, back = (hdtest.oracle_inflate_flushed if flush else hdtest.oracle_inflate)(m, len(d))
        assert r == 0 and back == d, (name, level, form)
    bad, edges = ec.check_many(items, nproc=4)
    assert not bad, bad[:10]
    return edges


@pytest.mark.timeout(900)
@pytest.mark.parametrize("level", range(10))
def test_batch_members_meet_every_rule(pkg, inputs, level):
    stalls = pkg.lib().hipdeflate_stall_count()
    blob, offs, lens = _pack(inputs)
    slot = int(pkg.lib().hipdeflate_bound(max(lens), level))
    items = []
    for frame, form in ((pkg.FRAME_RAW, "plain"), (pkg.FRAME_RAW_FLUSH, "flush"),
                        (pkg.FRAME_RAW | pkg.FRAME_LATENCY, "lat"), (pkg.FRAME_RAW_FLUSH | pkg.FRAME_LATENCY, "lat_flush")):
        members, crc, st = pkg.batch_deflate(blob, offs, lens, level, frame, slot=slot)
        for i, (name, d) in enumerate(inputs):
            assert st[i] == 0, (name, level, form)
            assert int(crc[i]) == zlib.crc32(d), name
            items.append((name, members[i], d, level, form, slot))
    _verify(items)
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(600)
@pytest.mark.parametrize("threads", [1, 2, 4])
def test_per_block_codecs_from_threads_meet_every_rule(pkg, inputs, threads):
    """hip_deflate / hip_deflate_flush (the latency form) called from `threads` threads at once"""
    stalls = pkg.lib().hipdeflate_stall_count()
    blocks = [(n, d) for n, d in inputs if len(d) <= 0xff00][:48]
    work = [(n, d, lv, fl) for n, d in blocks for lv in (1, 2, 6) for fl in (False, True)]
    got, errs = {}, []

    def run(k):
        try:
            for j in range(k, len(work), threads):
                n, d, lv, fl = work[j]
                got[j] = (pkg.hip_deflate_flush if fl else pkg.hip_deflate)(d, lv, cap=len(d) + len(d) // 2 + 64)
        except Exception as e:                        # (re-raised below, in the test's thread)
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    items = []
    for j, (n, d, lv, fl) in enumerate(work):
        r, m = got[j]
        assert r == 0, (n, lv, fl)
        items.append((n, m, d, lv, "lat_flush" if fl else "lat", len(d) + len(d) // 2 + 64))
    _verify(items)
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(600)
def test_device_resident_members_meet_every_rule(pkg, inputs):
    """device.DeviceDeflate: BGZF members in 64 KiB slots of HBM; the payloads obey the rules and equal the twin"""
    import importlib
    import torch
    dev = importlib.import_module("7bgzf_amd.device")
    stalls = pkg.lib().hipdeflate_stall_count()
    blocks = [(n, d) for n, d in inputs if 0 < len(d) <= 0xff00]
    blob, offs, lens = _pack(blocks)
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    items = []
    for level in (1, 2, 6):
        enc = dev.DeviceDeflate(len(blocks))
        enc.run(data, off, ln, level=level, frame=pkg.FRAME_BGZF)
        torch.cuda.synchronize()
        assert int(enc.status.abs().sum()) == 0
        slots = enc.slots.cpu().numpy()
        sizes = enc.out_len.cpu().numpy().view(np.uint32)
        for i, (n, d) in enumerate(blocks):
            m = bytes(slots[i * enc.slot: i * enc.slot + int(sizes[i])])
            assert int.from_bytes(m[-4:], "little") == len(d) and int.from_bytes(m[-8:-4], "little") == zlib.crc32(d), n
            items.append((n, m[18:-8], d, level, "plain", 65536 - 26))
    _verify(items)
    assert pkg.lib().hipdeflate_stall_count() == stalls
