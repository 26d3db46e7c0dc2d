"""hipdeflate_batch_inflate_size* and hipdeflate_batch_inflate_framed* on the MI355X against the model
(tests/framed_model.py, held to the reference's wrapper decoders by tests/test_framed_model.py) on every member of
tests/framed_gen.py: status, sizes, bytes consumed, check values, the bytes, and the bytes around them."""
import base64
import ctypes
import importlib
import json
import os
import time
import zlib

import numpy as np
import pytest

import deflate_gen as dg
import framed_gen
import framed_model as M
import hdtest

pytestmark = pytest.mark.gpu

FRAMES = [M.RAW, M.ZLIB, M.GZIP]
SENTINEL = 0xa5
PAD = 48                              # bytes between two members' rooms that nobody may write


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def dev():
    return importlib.import_module("7bgzf_amd.device")


@pytest.fixture(scope="module")
def members():
    return framed_gen.members()


@pytest.fixture(scope="module")
def sizes(members):
    """the model's size pass, once, for every test: member name -> (status, out_size, in_used)"""
    return {id(m): M.size(m.data, m.frame) for m in members}


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_size(dev, ms, frame):
    import torch
    blob, off, ln = framed_gen.pack(ms)
    n = len(ms)
    osz, used, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.inflate_size_call(_t(blob), _t(off), _t(ln), frame, osz, used, st)
    torch.cuda.synchronize()
    return _u32(osz), _u32(used), st.cpu().numpy()


def run_framed(dev, ms, frame, caps, want_check=True, want_used=True):
    """-> (out_len, check, in_used, status, out bytes, out_off): room i is out[out_off[i]:out_off[i] + caps[i]], PAD sentinel bytes behind it"""
    import torch
    blob, off, ln = framed_gen.pack(ms)
    n = len(ms)
    caps = np.asarray(caps, dtype=np.uint32)
    ooff = np.zeros(n, dtype=np.uint64)
    step = caps.astype(np.uint64) + PAD
    if n:
        ooff[1:] = np.cumsum(step[:-1])
    total = int(step.sum()) + PAD
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    olen, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    chk = torch.full((n,), -7, dtype=torch.int32, device="cuda") if want_check else None
    used = torch.full((n,), -7, dtype=torch.int32, device="cuda") if want_used else None
    dev.inflate_framed_call(_t(blob), _t(off), _t(ln), frame, out, _t(ooff), _t(caps), olen, chk, used, st)
    torch.cuda.synchronize()
    return (_u32(olen), _u32(chk) if want_check else None, _u32(used) if want_used else None, st.cpu().numpy(),
            out.cpu().numpy(), ooff)


def check_framed(ms, caps, res, want):
    """res of run_framed against want[i] = model.framed(member i, cap i); every byte outside the decoded members'
    [out_off, out_off + out_len) still holds the sentinel, but for the room of a member that failed"""
    olen, chk, used, st, out, ooff = res
    bad = []
    untouched = np.ones(len(out), dtype=bool)
    for i, m in enumerate(ms):
        w = want[i]
        got = (int(st[i]), int(olen[i]), int(used[i]) if used is not None else w[2], int(chk[i]) if chk is not None else w[3])
        if got != w[:4]:
            bad.append((m.name, int(caps[i]), got, w[:4]))
            continue
        o = int(ooff[i])
        if w[0] == 0:
            if out[o:o + w[1]].tobytes() != w[4]:
                bad.append((m.name, int(caps[i]), "bytes"))
            untouched[o:o + w[1]] = False
        else:
            untouched[o:o + int(caps[i])] = False            # the decoded prefix of a member that fails, inside its room
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:8])
    assert np.all(out[untouched] == SENTINEL), "bytes outside the members were written"


@pytest.mark.parametrize("frame", FRAMES)
def test_size_pass_against_the_model_on_every_member(pkg, dev, members, sizes, frame):
    ms = [m for m in members if m.frame == frame]
    osz, used, st = run_size(dev, ms, frame)
    bad = [(m.name, (int(st[i]), int(osz[i]), int(used[i])), sizes[id(m)]) for i, m in enumerate(ms)
           if (int(st[i]), int(osz[i]), int(used[i])) != sizes[id(m)]]
    assert len(ms) > 700 and not bad, "%d mismatches, first: %s" % (len(bad), bad[:8])
    assert pkg.lib().hipdeflate_stall_count() == 0


def test_size_pass_against_the_full_decoder_on_the_golden_vectors(pkg, dev):
    import torch
    vects = json.load(open(os.path.join(hdtest.GOLDEN, "inflate_std_vects.json")))
    muts = json.load(open(os.path.join(hdtest.GOLDEN, "mutants.json")))
    zs = [base64.b64decode(v["data"]) for v in vects] + [base64.b64decode(m["stream"]) for m in muts]
    assert len(vects) == 151 and len(muts) >= 100
    ms = [framed_gen.Member("golden%d" % i, M.RAW, z) for i, z in enumerate(zs)]
    osz, used, st = run_size(dev, ms, M.RAW)
    blob, off, ln = framed_gen.pack(ms)
    n, room = len(ms), 1 << 18                             # ample: one vector puts out more than 64 KiB before its fault, none this much
    caps = np.full(n, room, dtype=np.uint32)
    ooff = np.arange(n, dtype=np.uint64) * room
    out = torch.empty(n * room, dtype=torch.uint8, device="cuda")
    olen, crc, fst = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.device_inflate(_t(blob), _t(off), _t(ln), out, _t(ooff), _t(caps), olen, crc, fst)
    torch.cuda.synchronize()
    fst, olen = fst.cpu().numpy(), _u32(olen)
    assert not np.any(fst == 3)
    bad = [(i, int(st[i]), int(fst[i]), int(osz[i]), int(olen[i])) for i in range(n) if st[i] != fst[i] or osz[i] != olen[i]]
    assert not bad, bad[:8]
    assert np.all(st[:151] != 0) and np.sum(st == 0) > 50


def _amplifier(n):
    """a dynamic block of one literal, n matches (258, 1) coded in two bits each, one literal: 2 + 258 n bytes from n / 4 bytes.
    Built from the stream for 64 + n % 4 matches by repeating one byte of its token run."""
    n0 = 64 + n % 4
    lit = [0] * 286
    lit[285], lit[256], lit[65], lit[66] = 1, 2, 3, 3
    dl = [0] * 30
    dl[0] = 1

    def build(k):
        return dg.encode([dg.Block("dynamic", tokens=[65] + [(258, 1)] * k + [66], lit_lens=lit, dist_lens=dl, final=True)])
    a, b = build(n0), build(n0 + 4)
    # the token run is the longest run of one byte value (four tokens a byte): q lies inside it
    best, start = (0, 0), 0
    for i in range(1, len(a) + 1):
        if i == len(a) or a[i] != a[start]:
            best = max(best, (i - start, start))
            start = i
    q = best[1] + best[0] // 2
    assert best[0] >= 12 and len(b) == len(a) + 1 and a[:q] + a[q:q + 1] + a[q:] == b
    return a[:q] + a[q:q + 1] * ((n - n0) // 4) + a[q:]


def test_amplifier_is_what_it_says():
    """the splice against zlib where the output is small (CPU work, here because the GPU test below rests on it)"""
    for n in (64, 65, 66, 67, 100, 4001):
        z = _amplifier(n)
        out = zlib.decompress(z, -15)
        assert len(out) == 2 + 258 * n and out == b"A" * (1 + 258 * n) + b"B"
        assert M.size(z, M.RAW) == (0, len(out), len(z))


def test_size_pass_at_the_edge_of_32_bits(pkg, dev):
    """1032 : 1 -- about 4.1 MiB of stream just below 2^32 bytes of output, and at or above it; and 1 GiB"""
    n_below = ((1 << 32) - 1 - 2) // 258                   # 2 + 258 n <= 2^32 - 1
    cases = [(n_below, (0, 2 + 258 * n_below)), (n_below + 1, (3, 0)), ((1 << 30) // 258, (0, 2 + 258 * ((1 << 30) // 258)))]
    assert 2 + 258 * (n_below + 1) >= 1 << 32
    zs = [_amplifier(n) for n, _ in cases]
    for frame in FRAMES:
        ms = []
        for z, (n, w) in zip(zs, cases):
            plain_len = 2 + 258 * n
            if frame == M.RAW:
                ms.append(framed_gen.Member("amp%d" % n, frame, z))
            elif frame == M.ZLIB:
                ms.append(framed_gen.Member("amp%d" % n, frame, framed_gen.zlib_header() + z + b"\1\2\3\4"))   # (the Adler-32 is not examined)
            else:
                ms.append(framed_gen.Member("amp%d" % n, frame, framed_gen.gzip_header() + z + b"\1\2\3\4" +
                                            (plain_len & 0xffffffff).to_bytes(4, "little")))
        t0 = time.perf_counter()
        osz, used, st = run_size(dev, ms, frame)
        print("frame %d: size pass over %d tokens in %.3f s (copies included)" % (frame, sum(n for n, _ in cases), time.perf_counter() - t0))
        hdr = {M.RAW: 0, M.ZLIB: 2, M.GZIP: 10}[frame]
        for i, (n, w) in enumerate(cases):
            want_used = hdr + len(zs[i]) + M.FOOTER[frame] if w[0] == 0 else 0
            assert (int(st[i]), int(osz[i]), int(used[i])) == (w[0], w[1], want_used), (frame, n)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("room", ["exact", "minus1", "ample"])
def test_framed_decode_against_the_model_on_every_member(pkg, dev, members, sizes, frame, room):
    ms = [m for m in members if m.frame == frame]
    caps = []
    for m in ms:
        st, sz, _ = sizes[id(m)]
        if room == "exact":
            caps.append(sz if st == 0 else 65536)
        elif room == "minus1":
            caps.append(sz - 1 if st == 0 and sz else 100)
        else:
            caps.append(sz + 777 if st == 0 else 70000)
    want = [M.framed(m.data, m.frame, c) for m, c in zip(ms, caps)]
    if room == "minus1":
        assert sum(1 for w in want if w[0] == 3) > 400
    else:
        assert sum(1 for w in want if w[0] == 0) > 400
    for m, w in zip(ms, want):
        if w[0] == 0 and m.plain is not None:
            assert w[4] == m.plain
    check_framed(ms, caps, run_framed(dev, ms, frame, caps), want)
    assert pkg.lib().hipdeflate_stall_count() == 0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 5000])
def test_launch_shapes_valid_and_invalid_interleaved(pkg, dev, members, sizes, n):
    for frame in FRAMES:
        small = [m for m in members if m.frame == frame and len(m.data) < 3000 and sizes[id(m)][1] < 20000]
        good = [m for m in small if sizes[id(m)][0] == 0]
        poor = [m for m in small if sizes[id(m)][0] != 0]
        assert len(good) > 50 and len(poor) > 20
        ms = [(good if i % 2 == 0 else poor)[(i * 7 + n) % len(good if i % 2 == 0 else poor)] for i in range(n)]
        osz, used, st = run_size(dev, ms, frame)
        for i, m in enumerate(ms):
            assert (int(st[i]), int(osz[i]), int(used[i])) == sizes[id(m)], (frame, i, m.name)
        caps = [sizes[id(m)][1] if sizes[id(m)][0] == 0 else 512 for m in ms]
        cache = {}
        for m, c in zip(ms, caps):
            if id(m) not in cache:
                cache[id(m)] = M.framed(m.data, m.frame, c)
        want = [cache[id(m)] for m in ms]
        check_framed(ms, caps, run_framed(dev, ms, frame, caps), want)
        if n in (2, 65):
            check_framed(ms, caps, run_framed(dev, ms, frame, caps, want_check=False), want)
            check_framed(ms, caps, run_framed(dev, ms, frame, caps, want_used=False), want)
            check_framed(ms, caps, run_framed(dev, ms, frame, caps, want_check=False, want_used=False), want)


def test_no_members_is_no_work(pkg, dev):
    import torch
    L = pkg.lib()
    a = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    b, c, d = a.clone(), a.clone(), a.clone()
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for frame in FRAMES:
        assert L.hipdeflate_batch_inflate_size_dev(None, None, None, 0, frame, a.data_ptr(), b.data_ptr(), c.data_ptr(), s) == 0
        assert L.hipdeflate_batch_inflate_framed_dev(None, None, None, 0, frame, out.data_ptr(), None, None, a.data_ptr(), b.data_ptr(),
                                                     c.data_ptr(), d.data_ptr(), s) == 0
        z = np.zeros(1, dtype=np.uint32)
        p = z.ctypes.data_as(ctypes.c_void_p)
        assert L.hipdeflate_batch_inflate_size(None, None, None, 0, frame, p, p, p) == 0
        assert L.hipdeflate_batch_inflate_framed(None, None, None, 0, frame, None, None, None, p, None, None, p) == 0
    torch.cuda.synchronize()
    for t in (a, b, c, d):
        assert bool((t == -7).all())
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("frame", FRAMES)
def test_in_used_of_the_first_member_finds_the_second(pkg, dev, frame):
    import torch
    (m1, d1), (m2, d2) = framed_gen.pairs()[frame]
    both = m1 + m2
    blob = _t(np.frombuffer(bytes(5) + both + bytes(16), dtype=np.uint8))
    off = torch.tensor([5], dtype=torch.int64, device="cuda")
    ln = torch.tensor([len(both)], dtype=torch.int32, device="cuda")
    osz, used, st = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.inflate_size_call(blob, off, ln, frame, osz, used, st)
    assert (int(st[0]), int(osz[0]), int(used[0])) == (0, len(d1), len(m1))
    off2, ln2 = off + used.to(torch.int64), ln - used                     # the walk: on the device, by the caller
    dev.inflate_size_call(blob, off2, ln2, frame, osz, used, st)
    assert (int(st[0]), int(osz[0]), int(used[0])) == (0, len(d2), len(m2))
    out = torch.zeros(len(d2), dtype=torch.uint8, device="cuda")
    olen, chk = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    dev.inflate_framed_call(blob, off2, ln2, frame, out, torch.zeros(1, dtype=torch.int64, device="cuda"), osz, olen, chk, used, st)
    assert int(st[0]) == 0 and out.cpu().numpy().tobytes() == d2 and int(used[0]) == len(m2)
    assert int(_u32(chk)[0]) == (zlib.adler32(d2) if frame == M.ZLIB else zlib.crc32(d2))


def test_python_inflate_members_and_the_host_form(pkg, dev):
    import torch
    s = hdtest.synth()
    rng = np.random.default_rng(31)
    text, fq = bytes(s.text_like(400000, seed=41)), bytes(s.fastq_like(400000, seed=42))
    plains = []
    for i in range(300):
        n = int(rng.choice([0, 1, 100, 1023, 1024, 1025, 5000, 65535, 65536, 70001]))
        o = int(rng.integers(0, 300000))
        plains.append((text if i % 2 else fq)[o:o + n])
    for frame, wbits in ((M.ZLIB, 15), (M.GZIP, 31)):
        ms = []
        for i, p in enumerate(plains):
            c = zlib.compressobj(1 + i % 9, zlib.DEFLATED, wbits)
            ms.append(framed_gen.Member("m%d" % i, frame, c.compress(p) + c.flush(), p))
        blob, off, ln = framed_gen.pack(ms)
        out, out_off, out_len, status = dev.inflate_members(_t(blob), _t(off), _t(ln), frame)
        assert bool((status == 0).all()) and out.numel() == sum(len(p) for p in plains)
        o, oo, ol = out.cpu().numpy(), out_off.cpu().numpy(), _u32(out_len)
        for i, p in enumerate(plains):
            assert int(ol[i]) == len(p) and o[int(oo[i]):int(oo[i]) + len(p)].tobytes() == p, (frame, i)
        outs, chk, used, st = pkg.batch_inflate_framed([m.data for m in ms], [len(p) for p in plains], frame)
        osz, used2, st2 = pkg.batch_inflate_size([m.data for m in ms], frame)
        for i, p in enumerate(plains):
            assert st[i] == 0 and outs[i] == p and used[i] == len(ms[i].data) == used2[i] and st2[i] == 0 and osz[i] == len(p), (frame, i)
            assert int(chk[i]) == (zlib.adler32(p) if frame == M.ZLIB else zlib.crc32(p))
    assert pkg.lib().hipdeflate_stall_count() == 0


def test_arguments(pkg, dev):
    import torch
    L = pkg.lib()
    z = zlib.compress(b"hello hello hello")
    blob = _t(np.frombuffer(z + bytes(16), dtype=np.uint8))
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    ln = torch.tensor([len(z)], dtype=torch.int32, device="cuda")
    a, b, c, d = (torch.full((1,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    cap = torch.tensor([64], dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    hz = np.frombuffer(z, dtype=np.uint8)
    hoff, hln, hcap = np.zeros(1, dtype=np.uint64), np.array([len(z)], dtype=np.uint32), np.array([64], dtype=np.uint32)
    hres = [np.zeros(1, dtype=np.uint32) for _ in range(4)]
    hout = np.zeros(64, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for frame in (pkg.FRAME_BGZF, pkg.FRAME_MIGZ, pkg.FRAME_RAW_FLUSH, pkg.FRAME_ZLIB | pkg.FRAME_LATENCY, pkg.FRAME_LATENCY, 6, -1):
        assert L.hipdeflate_batch_inflate_size_dev(blob.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, frame, a.data_ptr(), b.data_ptr(),
                                                   c.data_ptr(), s) == pkg.HD_E_ARG
        assert L.hipdeflate_batch_inflate_framed_dev(blob.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, frame, out.data_ptr(),
                                                     off.data_ptr(), cap.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(),
                                                     d.data_ptr(), s) == pkg.HD_E_ARG
        assert L.hipdeflate_batch_inflate_size(p(hz), p(hoff), p(hln), 1, frame, p(hres[0]), p(hres[1]), p(hres[2])) == pkg.HD_E_ARG
        assert L.hipdeflate_batch_inflate_framed(p(hz), p(hoff), p(hln), 1, frame, p(hout), p(hoff), p(hcap), p(hres[0]), p(hres[1]),
                                                 p(hres[2]), p(hres[3])) == pkg.HD_E_ARG
    torch.cuda.synchronize()
    assert all(int(t[0]) == -7 for t in (a, b, c, d))
    # a member of HD_INFLATE_MAX_IN bytes: refused whole, no byte of it is read (the buffer holds a few dozen)
    big = torch.tensor([M.MAX_IN], dtype=torch.int32, device="cuda")
    hbig = np.array([M.MAX_IN], dtype=np.uint32)
    for frame in FRAMES:
        dev.inflate_size_call(blob, off, big, frame, a, b, c)
        assert (int(c[0]), int(a[0]), int(b[0])) == (1, 0, 0), frame
        dev.inflate_framed_call(blob, off, big, frame, out, off, cap, a, b, c, d)
        assert (int(d[0]), int(a[0]), int(b[0]), int(c[0])) == (1, 0, 0, 0), frame
        assert L.hipdeflate_batch_inflate_size(p(hz), p(hoff), p(hbig), 1, frame, p(hres[0]), p(hres[1]), p(hres[2])) == pkg.HD_E_ARG
        assert L.hipdeflate_batch_inflate_framed(p(hz), p(hoff), p(hbig), 1, frame, p(hout), p(hoff), p(hcap), p(hres[0]), p(hres[1]),
                                                 p(hres[2]), p(hres[3])) == pkg.HD_E_ARG
    # and the member itself, to see that the arrays above are in order
    dev.inflate_framed_call(blob, off, ln, M.ZLIB, out, off, cap, a, b, c, d)
    assert (int(d[0]), int(a[0]), int(c[0])) == (0, 17, len(z)) and out[:17].cpu().numpy().tobytes() == b"hello hello hello"
