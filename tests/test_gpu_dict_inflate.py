"""The batch decoder with a preset dictionary -- hipdeflate_batch_inflate_dict_dev, hipdeflate_batch_inflate_dict and their
device.py / package forms -- against tests/dict_model.py: bytes, out_len, check, in_used and status of every member are the
model's, which tests/test_dict_model.py holds to Python's zlib.  No case provokes a fault; every refusal is one the header
defines.  Every launch's output lies between guard bytes, and no byte outside a member's room is written.

Where the cases land (hd_inflate.hpp inflate_stream<..., InflateDictArgs>, hd_frame.hpp k_dict_open):
  * streams zlib wrote with zdict at levels 0 (stored), 1, 6, 9 and Z_FIXED (static), raw and in the zlib wrapper;
    dictionaries of 1 .. 40000 bytes (32767: one short of the window; 40000: only the last 32768 count); blocks of 10 bytes
    (the scalar loop alone), 3000 (windows, sources in the ring and in the dictionary) and 64 KiB (flushed output as source);
  * hand-built streams with one match at each edge of the source logic, as the stream's last token (the scalar loop) and with
    300 literals behind it (the window decode): tests/dict_cases.py hand_cases;
  * the encoder's own members; 600 members in one launch."""
import importlib
import os
import zlib

import numpy as np
import pytest

import dict_cases as dc
import dict_model as dm
import hdtest

pytestmark = pytest.mark.gpu

RAW, ZLIB = dm.RAW, dm.ZLIB
GUARD, SENT = 64, 0xa5


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    assert (p.FRAME_RAW, p.FRAME_ZLIB) == (RAW, ZLIB)
    return p


@pytest.fixture(scope="module")
def torch():
    return importlib.import_module("torch")


@pytest.fixture(scope="module")
def dev():
    return importlib.import_module("7bgzf_amd.device")


def to_dev(torch, blob, shift=0):
    buf = torch.from_numpy(np.frombuffer(bytes(shift) + bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    return buf[shift:shift + len(blob)]


def i64(torch, v):
    return torch.from_numpy(np.asarray(v, dtype=np.int64)).cuda()


def i32(torch, v):
    return torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32)).cuda()


def decode(torch, dev, members, caps, d, frame, d_shift=0, gap=3, framed=False, results=True):
    """one device call over `members`, packed `gap` bytes apart behind one odd byte, rooms GUARD bytes apart between guards
    -> [(status, out_len, in_used, check, output)]; framed: hipdeflate_batch_inflate_framed_dev instead (no dictionary)"""
    blob, ioff = bytearray(b"\x33"), []
    for m in members:
        ioff.append(len(blob))
        blob += bytes(m) + b"\x44" * gap
    ooff, o = [], GUARD
    for c in caps:
        ooff.append(o)
        o += c + GUARD
    n = len(members)
    out = torch.full((o + 16,), SENT, dtype=torch.uint8, device="cuda")
    out_len, check, used, status = (torch.full((n,), -3, dtype=torch.int32, device="cuda") for _ in range(4))
    args = (to_dev(torch, blob), i64(torch, ioff), i32(torch, [len(m) for m in members]), frame)
    rest = (out, i64(torch, ooff), i32(torch, caps), out_len, check if results else None, used if results else None, status)
    if framed:
        dev.inflate_framed_call(*args, *rest)
    else:
        dev.inflate_dict_call(*args, to_dev(torch, d, d_shift) if len(d) else None, *rest)
    raw = bytes(out.cpu().numpy())
    st, ln = status.cpu().tolist(), out_len.cpu().numpy().view(np.uint32).tolist()
    chk, us = check.cpu().numpy().view(np.uint32).tolist(), used.cpu().numpy().view(np.uint32).tolist()
    got, at = [], 0
    for i in range(n):
        assert raw[at:ooff[i]] == bytes([SENT]) * (ooff[i] - at), "bytes in front of room %d were written" % i
        at = ooff[i] + caps[i]
        assert ln[i] <= caps[i]
        # (a member that fails may leave its decoded prefix inside its room: only what a good member made is compared)
        if st[i] == 0:
            assert raw[ooff[i] + ln[i]:at] == bytes([SENT]) * (caps[i] - ln[i]), "room %d was written behind out_len" % i
        got.append((st[i], ln[i], us[i] if results else None, chk[i] if results else None, raw[ooff[i]:ooff[i] + ln[i]] if st[i] == 0 else b""))
    assert raw[at:] == bytes([SENT]) * (len(raw) - at)
    return got


def model(members, caps, d, frame, results=True):
    want = [dm.member(m, frame, d, c) for m, c in zip(members, caps)]
    return want if results else [(s, n, None, None, o) for s, n, _, _, o in want]


def same(got, want, names=None):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "member %s: (status, out_len, in_used, check) %r, the model's %r%s" % (
            names[i] if names else i, g[:4], w[:4], "" if g[4] == w[4] else "; the bytes differ")
    assert len(got) == len(want)


# ---- streams zlib wrote ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dict_len", dc.DEC_DICT_LENS)
@pytest.mark.parametrize("wbits", [-15, 15])
@pytest.mark.parametrize("kind", dc.KINDS)
def test_streams_zlib_wrote_with_a_dictionary(torch, dev, kind, dict_len, wbits):
    frame = RAW if wbits < 0 else ZLIB
    d = dc.dictionary(kind, dict_len)
    members, caps = [], []
    for n in dc.DEC_BLOCK_LENS:
        data = dc.master(kind)[dc.AT:dc.AT + n]
        for level, strategy in [(lv, 0) for lv in dc.DEC_LEVELS] + [(6, zlib.Z_FIXED)]:
            members.append(dc.zlib_member(data, d, level, wbits, strategy))
            caps.append(n)
    want = model(members, caps, d, frame)
    assert all(w[0] == 0 and w[2] == len(m) for w, m in zip(want, members))
    same(decode(torch, dev, members, caps, d, frame), want)
    # without check and in_used; the dictionary at odd addresses; one byte of room too few (status 3)
    same(decode(torch, dev, members, caps, d, frame, d_shift=1, results=False), model(members, caps, d, frame, results=False))
    tight = [c - 1 for c in caps]
    want = model(members, tight, d, frame)
    assert all(w[0] == 3 for w in want)
    same(decode(torch, dev, members, tight, d, frame, d_shift=7), want)


# ---- hand-built streams: every edge of the source logic --------------------------------------------------------------------

@pytest.mark.parametrize("dict_len", dc.DEC_DICT_LENS)
def test_hand_built_streams(torch, dev, dict_len):
    d = dc.dictionary("text", dict_len)
    cases = dc.hand_cases("text", dict_len)
    names, members = [c[0] for c in cases], [c[1] for c in cases]
    caps = [len(c[2]) if c[2] is not None else 4096 for c in cases]
    want = model(members, caps, d, RAW)
    for c, w in zip(cases, want):                          # (the model's answers are the hand-made ones)
        assert (w[0], w[4]) == ((0, c[2]) if c[2] is not None else (1, b"")), c[0]
    same(decode(torch, dev, members, caps, d, RAW), want, names)
    # a member whose output ends one byte past out_cap
    good = [(c, k) for c, k in zip(cases, caps) if c[2] is not None]
    tight = [k - 1 for _, k in good]
    want = model([c[1] for c, _ in good], tight, d, RAW)
    assert all(w[0] == 3 for w in want)
    same(decode(torch, dev, [c[1] for c, _ in good], tight, d, RAW), want, [c[0] for c, _ in good])
    # the same streams in the zlib wrapper, naming the dictionary
    framed = [dm.zlib_header(d) + c[1] + zlib.adler32(c[2] or b"").to_bytes(4, "big") for c in cases]
    want = model(framed, caps, d, ZLIB)
    assert [w[0] for w in want] == [0 if c[2] is not None else 1 for c in cases]
    same(decode(torch, dev, framed, caps, d, ZLIB), want, names)


def test_distance_32768_at_position_0(torch, dev):
    import deflate_gen as dg
    d = dc.dictionary("fastq", 32768)
    raws = [dg.encode([dg.Block(kind, tokens=[(258, 32768), (3, 32768)] + list(b"tail" * n), final=True)])
            for kind in ("static", "dynamic") for n in (0, 100)]
    want = model(raws, [4096] * 4, d, RAW)
    assert all(w[0] == 0 and w[4][:261] == d[:261] for w in want)
    same(decode(torch, dev, raws, [4096] * 4, d, RAW), want)
    # ... and one byte further with a dictionary one byte shorter: in front of the data
    same(decode(torch, dev, raws, [4096] * 4, d[1:], RAW), [(1, 0, 0, 0, b"")] * 4)
    # ... while a longer dictionary's last 32768 bytes are the ones named
    longer = dc.dictionary("fastq", 40000)
    assert longer[-32768:] == d
    same(decode(torch, dev, raws, [4096] * 4, longer, RAW), want)


# ---- the zlib frame ----------------------------------------------------------------------------------------------------------

def test_zlib_frame_rules(torch, dev):
    d = dc.dictionary("fastq", 5000)
    data = dc.master("fastq")[dc.AT:dc.AT + 3000]
    m = dc.zlib_member(data, d, 6, 15)
    plain = zlib.compress(data, 6)
    raw = dc.zlib_member(data, d, 6, -15)
    members = [m, m + b"behind", plain, m[:-1] + bytes([m[-1] ^ 1]), m[:2], m[:3], m[:5], m[:6], m[:9],
               bytes([m[0], m[1] ^ 1]) + m[2:],                              # FCHECK
               plain[:2] + raw + zlib.adler32(data).to_bytes(4, "big"),      # needs the dictionary, does not name it
               m[:2] + bytes(4) + m[6:]]                                     # DICTID 0
    caps = [3000] * len(members)
    want = model(members, caps, d, ZLIB)
    assert [w[0] for w in want] == [0, 0, 0] + [1] * 9
    assert want[0][2] == len(m) and want[1][2] == len(m) and want[2][2] == len(plain) and want[0][3] == zlib.adler32(data)
    same(decode(torch, dev, members, caps, d, ZLIB), want)
    # another dictionary, the same one a byte shorter: the wrong DICTID -- only the member that does not name it decodes
    for other in (dc.dictionary("text", 5000), d[1:]):
        want = model(members, caps, other, ZLIB)
        assert [w[0] for w in want] == [1, 1, 0] + [1] * 9
        same(decode(torch, dev, members, caps, other, ZLIB), want)


def test_without_a_dictionary_it_is_the_framed_call(torch, dev):
    data = [dc.master(k)[dc.AT:dc.AT + n] for k in dc.KINDS for n in (0, 10, 3000, 40000)]
    d = dc.dictionary("text", 5000)
    for frame, wbits in ((RAW, -15), (ZLIB, 15)):
        members = [dc.zlib_member(x, b"", 6, wbits) for x in data]
        members += [members[2][:-3], members[3][:40], b"", b"\x07"]          # cut short; block type 3
        members += [dc.zlib_member(data[2], d, 6, wbits)]                    # written with a dictionary nobody gives
        caps = [len(x) for x in data] + [3000, 40000, 16, 16, 3000]
        got = decode(torch, dev, members, caps, b"", frame)
        want = model(members, caps, b"", frame)
        assert [w[0] for w in want][:8] == [0] * 8 and want[-1][0] == 1
        same(got, want)
        if frame == ZLIB:
            # (the framed call refuses FDICT in the header, this call where no dictionary was given: both status 1)
            assert members[-1][1] & 0x20
        assert decode(torch, dev, members, caps, b"", frame, framed=True) == got


# ---- the encoder's own members, many members, the host form -------------------------------------------------------------------

def test_the_encoders_own_members(torch, dev, pkg):
    for kind, dict_len, level in (("text", 32768, 6), ("fastq", 5000, 3), ("text", 40000, 4)):
        d = dc.dictionary(kind, dict_len)
        offs, lens = dc.blocks(kind)
        members, crc, st = pkg.batch_deflate_dict(dc.master(kind), offs, lens, d, level)
        assert list(st) == [0] * len(offs)
        want = model(members, lens, d, RAW)
        assert [(w[0], w[4]) for w in want] == [(0, dc.master(kind)[o:o + n]) for o, n in zip(offs, lens)]
        assert [w[3] for w in want] == [int(c) for c in crc]
        same(decode(torch, dev, members, lens, d, RAW), want)


def test_600_members_in_one_launch(torch, dev):
    n, size = 600, 2048
    d = dc.dictionary("text", 32768)
    offs, lens = dc.blocks("text", (size,) * n)
    blocks = [dc.master("text")[o:o + size] for o in offs]
    for frame, wbits in ((RAW, -15), (ZLIB, 15)):
        members = [dc.zlib_member(b, d, 6, wbits) for b in blocks]
        members[17] = members[17][:-5]                     # one bad member among them (cut short: the model says how it fails)
        got = decode(torch, dev, members, lens, d, frame, gap=0)
        assert got[17][0] != 0
        for i, (g, b, m) in enumerate(zip(got, blocks, members)):
            if i != 17:
                assert g == (0, size, len(m), zlib.adler32(b) if frame == ZLIB else zlib.crc32(b), b), i
        same([got[i] for i in (0, 17, 599)], model([members[i] for i in (0, 17, 599)], [size] * 3, d, frame))


def test_host_form_and_device_wrapper(torch, dev, pkg):
    d = dc.dictionary("fastq", 40000)
    data = [dc.master("fastq")[dc.AT + 7 * i:dc.AT + 7 * i + n] for i, n in enumerate((10, 3000, 64 << 10, 0))]
    for frame, wbits in ((RAW, -15), (ZLIB, 15)):
        members = [dc.zlib_member(x, d, 9, wbits) for x in data] + [b"\x07"]
        caps = [len(x) for x in data] + [16]
        want = model(members, caps, d, frame)
        outs, chk, used, st = pkg.batch_inflate_dict(members, caps, d, frame)
        assert [(int(s), len(o), int(u), int(c), o) for s, o, u, c in zip(st, outs, used, chk)] == want
        # device.inflate_dict: rooms of its own
        blob, ioff = b"".join(members), np.cumsum([0] + [len(m) for m in members[:-1]])
        out, out_off, out_len, status = dev.inflate_dict(to_dev(torch, blob), i64(torch, ioff), i32(torch, [len(m) for m in members]),
                                                         to_dev(torch, d), frame, out_cap=i32(torch, caps))
        raw, oo = bytes(out.cpu().numpy()), out_off.cpu().tolist()
        assert status.cpu().tolist() == [w[0] for w in want]
        assert [raw[o:o + n] for o, n in zip(oo, out_len.cpu().tolist())] == [w[4] for w in want]
    with pytest.raises(pkg.HipDeflateError, match="101"):
        pkg.batch_inflate_dict([b"\x03\x00"], [16], d, pkg.FRAME_GZIP)


def test_refusals(torch, dev, pkg):
    src, d = to_dev(torch, b"\x03\x00"), to_dev(torch, bytes(64))
    off, ln, cap = i64(torch, [0]), i32(torch, [2]), i32(torch, [16])
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    r = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(4)]
    L, st = pkg.lib(), torch.cuda.current_stream().cuda_stream
    call = lambda frame, dp, dn, out_len, status: L.hipdeflate_batch_inflate_dict_dev(
        src.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, frame, dp, dn, out.data_ptr(), off.data_ptr(), cap.data_ptr(), out_len,
        r[1].data_ptr(), r[2].data_ptr(), status, st)
    assert call(RAW, d.data_ptr(), 64, r[0].data_ptr(), r[3].data_ptr()) == 0
    assert call(RAW, None, 0, r[0].data_ptr(), r[3].data_ptr()) == 0
    for bad in ((pkg.FRAME_GZIP, d.data_ptr(), 64, r[0].data_ptr(), r[3].data_ptr()), (pkg.FRAME_BGZF, d.data_ptr(), 64, r[0].data_ptr(), r[3].data_ptr()),
                (RAW | pkg.FRAME_LATENCY, d.data_ptr(), 64, r[0].data_ptr(), r[3].data_ptr()), (RAW, None, 64, r[0].data_ptr(), r[3].data_ptr()),
                (RAW, d.data_ptr(), 64, None, r[3].data_ptr()), (ZLIB, d.data_ptr(), 64, r[0].data_ptr(), None)):
        assert call(*bad) == 101                           # HD_E_ARG
    torch.cuda.synchronize()
    assert (r[3].item(), r[0].item()) == (0, 0)
