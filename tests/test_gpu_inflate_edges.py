"""The hand-built DEFLATE corpus (tests/deflate_gen.py) through every decode entry point on the MI355X: exact
status equality with the verdict the family states (pinned to the oracle and libdeflate by
tests/test_deflate_gen.py), output bytes equal to the token lists' bytes, CRC-32 equal to zlib.crc32.

Where the families land in the kernels (hd_inflate.hpp unless said otherwise):
  * match_matrix -- distances 1725 / 1726 (ring) against 1727 and beyond (HBM): the near/far split of the scalar
    copy (INF_NEAR) and of the windows (inr / hbm masks); sources and destinations placed across the 2 KiB ring
    wrap and across 1 KiB piece edges by the output phases; lengths <= 8 and 9..16 go to the lane-group passes
    of 8 and 16 when a window takes them (the 0 / 2 / 37 / 300 literals in front vary where the window starts);
    lengths > 64 and overlapping ones to the general copies.
  * code_shapes -- litlen codewords of 10..15 bits and offset codewords of 9..15 bits miss the 9- / 8-bit
    direct tables: the bit-serial slow path (K_SLOW), in runs at the start, middle and end of a block, with the
    window falling back to the scalar loop around them; in the latency kernel they are the runs of long
    codewords between spec windows.
  * amplify -- 258 output bytes per 2 input bits: windows cut by the output budget (WIN_OUT_BUDGET) long before
    the input runs out, the ring wrapped many times per window's worth of input.
  * blocks / chunk -- stored blocks at every bit alignment, empty blocks, hundreds of 5-token blocks: the
    header and end-of-block paths; the chunk forms are the flushed entry points' streams.
  * faults / cap_minus1 -- every verdict rule, once each.

The latency kernel (hip_inflate, hip_inflate_flush) gives up after INF_LAT_SPINS with HD_BAD_DATA: a valid
stream that comes back non-zero is a failure here, never something to tolerate."""
import importlib
import os
import threading
import zlib

import numpy as np
import pytest

import deflate_gen as dg
import hdtest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def cases():
    return dg.cached_corpus()


def _want(c, flushed):
    return c.code_flushed if flushed else c.code


def _mismatches(cs, outs, crc, st, flushed):
    bad = []
    for i, c in enumerate(cs):
        w = _want(c, flushed)
        if int(st[i]) != w:
            bad.append((c.name, "status", int(st[i]), w))
        elif w == 0:
            if outs[i] != c.expected:
                bad.append((c.name, "bytes", len(outs[i]), len(c.expected)))
            elif crc is not None and (int(crc[i]) & 0xffffffff) != zlib.crc32(c.expected):
                bad.append((c.name, "crc"))
    return bad


def _report(bad):
    return "%d mismatches, first: %s" % (len(bad), bad[:12])


@pytest.mark.timeout(300)
def test_batch_inflate_whole_corpus_one_launch(pkg, cases):
    outs, crc, st = pkg.batch_inflate([c.stream for c in cases], [c.cap for c in cases])
    bad = _mismatches(cases, outs, crc, st, False)
    assert not bad, _report(bad)


@pytest.mark.timeout(300)
def test_batch_inflate_one_launch_per_family(pkg, cases):
    bad = []
    for fam in sorted({c.family for c in cases}):
        cs = [c for c in cases if c.family == fam]
        outs, crc, st = pkg.batch_inflate([c.stream for c in cs], [c.cap for c in cs])
        bad += _mismatches(cs, outs, crc, st, False)
    # 1, 3 and 5 small members, with and without the caller's crc array: the host table's columns at odd counts (the
    # crc column is the last one back, hd_tables.hpp DecTable), and a caller that wants no crc gets none written
    small = [c for c in cases if c.code == dg.OK and 0 < len(c.expected) and len(c.stream) <= 300 and c.cap <= 300]
    assert len(small) >= 9
    for k, count in enumerate((1, 3, 5)):
        cs = small[k * 2:k * 2 + count]
        for want_crc in (True, False):
            outs, crc, st = pkg.batch_inflate([c.stream for c in cs], [c.cap for c in cs], want_crc=want_crc)
            bad += _mismatches(cs, outs, crc if want_crc else None, st, False)
            assert want_crc or not crc.any()
    assert not bad, _report(bad)


@pytest.mark.timeout(300)
def test_batch_inflate_flushed(pkg, cases):
    """every stream through the flushed batch entry point: the chunk forms decode there, the rest as before"""
    outs, crc, st = pkg.batch_inflate([c.stream for c in cases], [c.cap for c in cases], flushed=True)
    bad = _mismatches(cases, outs, crc, st, True)
    assert not bad, _report(bad)
    assert sum(1 for c in cases if c.chunk and c.code_flushed == dg.OK) >= 50


def _call(pkg, c):
    f = pkg.hip_inflate_flush if c.chunk else pkg.hip_inflate
    return f(c.stream, c.cap)


def _check_call(c, r, out):
    w = _want(c, c.chunk)
    if r != w:
        return (c.name, "status", r, w)
    if w == 0 and out != c.expected:
        return (c.name, "bytes", len(out), len(c.expected))
    return None


@pytest.mark.timeout(600)
def test_hip_inflate_lone_calls(pkg, cases):
    """one call at a time (the chunk forms through hip_inflate_flush), and the chunk forms through hip_inflate
    too, where they must be refused"""
    bad = []
    for c in cases:
        e = _check_call(c, *_call(pkg, c))
        if e:
            bad.append(e)
    for c in cases:
        if c.chunk:
            r, _ = pkg.hip_inflate(c.stream, c.cap)
            if r != c.code:
                bad.append((c.name, "plain", r, c.code))
    assert not bad, _report(bad)


@pytest.mark.timeout(600)
def test_hip_inflate_from_16_threads(pkg, cases):
    bad, lock = [], threading.Lock()

    def work(k):
        for c in cases[k::16]:
            e = _check_call(c, *_call(pkg, c))
            if e:
                with lock:
                    bad.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, _report(bad)


@pytest.mark.timeout(300)
def test_device_inflate_odd_offsets(pkg, cases):
    """the device-resident entry point with every stream and every output at an odd offset of one buffer; the
    bytes between the outputs must stay as they were"""
    import torch
    dev = importlib.import_module("7bgzf_amd.device")
    rng = np.random.default_rng(5)
    ioff, ooff, pos, opos = [], [], 0, 0
    for c in cases:
        pos += int(rng.integers(0, 8)) * 2 + 1
        ioff.append(pos)
        pos += len(c.stream)
        opos += int(rng.integers(0, 8)) * 2 + 1
        ooff.append(opos)
        opos += c.cap
    opos += 17
    src = np.zeros(pos + 64, dtype=np.uint8)
    for c, o in zip(cases, ioff):
        src[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    comp = torch.from_numpy(src).cuda()
    out = torch.full((opos,), 0xa5, dtype=torch.uint8, device="cuda")
    nb = len(cases)
    in_off = torch.tensor(ioff, dtype=torch.int64, device="cuda")
    in_len = torch.tensor([len(c.stream) for c in cases], dtype=torch.int32, device="cuda")
    out_off = torch.tensor(ooff, dtype=torch.int64, device="cuda")
    out_cap = torch.tensor([c.cap for c in cases], dtype=torch.int32, device="cuda")
    out_len = torch.zeros(nb, dtype=torch.int32, device="cuda")
    crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    st = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    dev.device_inflate(comp, in_off, in_len, out, out_off, out_cap, out_len, crc, st)
    torch.cuda.synchronize()
    host, stv = out.cpu().numpy(), st.cpu().numpy()
    olen, crcv = out_len.cpu().numpy(), crc.cpu().numpy()
    outs = [bytes(host[o:o + int(olen[i])]) if stv[i] == 0 else b"" for i, o in enumerate(ooff)]
    bad = _mismatches(cases, outs, crcv, stv, False)
    assert not bad, _report(bad)
    guard = np.ones(opos, dtype=bool)
    for c, o in zip(cases, ooff):
        guard[o:o + c.cap] = False
    assert np.all(host[guard] == 0xa5), "bytes written outside the output slots"


@pytest.mark.timeout(300)
def test_unpipe_bgzf_members_of_generated_streams(pkg, cases):
    """BGZF members whose payloads are the corpus's valid streams, through the streaming decoder"""
    members, want = [], []
    for c in cases:
        if c.code != dg.OK or len(c.expected) > 0xff00 or len(c.stream) + 26 > 65536:
            continue
        body = c.stream + zlib.crc32(c.expected).to_bytes(4, "little") + len(c.expected).to_bytes(4, "little")
        hdr = bytes.fromhex("1f8b08040000000000ff060042430200") + (len(body) + 18 - 1).to_bytes(2, "little")
        members.append(hdr + body)
        want.append(c.expected)
    assert len(members) > 200
    r, out = pkg.unpipe_decompress(b"".join(members) + pkg.BGZF_EOF)
    assert r == 0 and out == b"".join(want)
