"""tests/dict_model.py held to Python's zlib, without a GPU: the model the device tests compare against decodes what zlib
writes with a preset dictionary, refuses what zlib refuses, knows the wrapper's FDICT / DICTID rules -- and on the encode cases
of tests/test_gpu_dict_deflate.py no token crosses the seam and the dictionary pays."""
import zlib

import pytest

import deflate_gen as dg
import dict_cases as dc
import dict_model as dm


def zlib_inflate(raw, d, wbits=-15):
    o = zlib.decompressobj(wbits, zdict=bytes(d)) if len(d) else zlib.decompressobj(wbits)
    out = o.decompress(bytes(raw))
    assert o.eof
    return out, o.unused_data


def test_used_of():
    assert [dm.used_of(n) for n in (0, 1, 1023, 1024, 1025, 5000, 32767, 32768, 40000)] == [0, 0, 0, 1024, 1024, 4096, 31744, 32768, 32768]
    d = dc.dictionary("text", 5000)
    assert dm.history_of(d) == d[-4096:] and dm.history_of(d[:1023]) == b""


@pytest.mark.parametrize("dict_len", dc.DEC_DICT_LENS)
@pytest.mark.parametrize("wbits", [-15, 15])
def test_model_decodes_what_zlib_writes(dict_len, wbits):
    d = dc.dictionary("text", dict_len)
    frame = dm.RAW if wbits < 0 else dm.ZLIB
    for kind in dc.KINDS:
        for n in dc.DEC_BLOCK_LENS:
            data = dc.master(kind)[dc.AT:dc.AT + n]
            for level, strategy in [(lv, 0) for lv in dc.DEC_LEVELS] + [(6, zlib.Z_FIXED)]:
                m = dc.zlib_member(data, d, level, wbits, strategy)
                assert dm.member(m, frame, d, n) == (0, n, len(m), zlib.adler32(data) if wbits > 0 else zlib.crc32(data), data)
                assert dm.member(m, frame, d, n - 1)[0] == dm.INSUFFICIENT_SPACE
                assert dm.member(m + b"xyz", frame, d, n)[2] == len(m)            # bytes behind the member are allowed


def test_zlib_header_rules():
    d = dc.dictionary("fastq", 5000)
    data = dc.master("fastq")[dc.AT:dc.AT + 3000]
    m = dc.zlib_member(data, d, 6, 15)
    hdr = (m[0] << 8) | m[1]
    assert hdr % 31 == 0 and (m[1] >> 5) & 1 and int.from_bytes(m[2:6], "big") == zlib.adler32(d)
    assert m[:6] == dm.zlib_header(d)
    assert dm.open_zlib(m, d) == (6, True)
    # wrong DICTID: another dictionary, the same one a byte shorter, none at all
    for other in (dc.dictionary("text", 5000), d[1:], b""):
        assert dm.member(m, dm.ZLIB, other, 3000) == (1, 0, 0, 0, b"")
        if len(other):
            with pytest.raises(zlib.error):
                zlib_inflate(m, other, 15)
    # a header cut inside DICTID, or with no room for the trailer behind it
    for n in (2, 3, 5, 6, 9):
        assert dm.member(m[:n], dm.ZLIB, d, 3000)[0] == 1
    # FDICT clear: decoded without the dictionary, whatever was given
    plain = zlib.compress(data, 6)
    assert not (plain[1] >> 5) & 1
    assert dm.member(plain, dm.ZLIB, d, 3000) == (0, 3000, len(plain), zlib.adler32(data), data)
    # ... so a stream that needs the dictionary fails without the bit: the raw member in a plain wrapper
    raw = dc.zlib_member(data, d, 6, -15)
    bare = plain[:2] + raw + zlib.adler32(data).to_bytes(4, "big")
    assert dm.member(bare, dm.ZLIB, d, 3000)[0] == 1
    # wrong Adler-32
    bad = m[:-1] + bytes([m[-1] ^ 1])
    assert dm.member(bad, dm.ZLIB, d, 3000) == (1, 0, 0, 0, b"")
    with pytest.raises(zlib.error):
        zlib_inflate(bad, d, 15)


@pytest.mark.parametrize("dict_len", dc.DEC_DICT_LENS)
def test_hand_built_streams_are_zlibs_verdicts(dict_len):
    d = dc.dictionary("text", dict_len)
    seen = set()
    for name, raw, want in dc.hand_cases("text", dict_len):
        st, out, bits = dm.inflate(raw, d, 1 << 17)
        if want is None:
            assert st == 1, name
            with pytest.raises(zlib.error):
                zlib_inflate(raw, d)
        else:
            assert (st, out, (bits + 7) // 8) == (0, want, len(raw)), name
            assert zlib_inflate(raw, d) == (want, b""), name
            assert dm.inflate(raw, d, len(want) - 1)[0] == dm.INSUFFICIENT_SPACE, name
        seen.add(name.rsplit("_tail", 1)[0])
    must = {"first_at_D", "overlap_seam", "far_first_byte", "far_straddle", "far_group_straddle", "far_group8_straddle",
            "far_load_straddle", "near_straddle", "stored_static"}
    assert must | ({"first_past_D"} if dict_len < 32768 else set()) <= seen      # (no distance names byte 32769)


def test_distance_one_past_the_dictionary():
    """the model's verdict equals zlib.error, at the first token and after output, for a dictionary shorter than the window"""
    for dict_len in (100, 32767):
        d = dc.dictionary("text", dict_len)
        for head in ((0, 50) if dict_len == 100 else (0,)):        # (a distance is at most 32768)
            for over in (0, 1):
                toks = list(d[:head]) + [(20, head + dict_len + over)]
                raw = dg.encode([dg.Block("static", tokens=toks, final=True)])
                st, out, _ = dm.inflate(raw, d, 4096)
                if over:
                    assert st == 1
                    with pytest.raises(zlib.error):
                        zlib_inflate(raw, d)
                else:
                    assert st == 0 and zlib_inflate(raw, d) == (out, b"")
    # a 40000-byte dictionary: only its last 32768 bytes can be named
    d = dc.dictionary("text", 40000)
    raw = dg.encode([dg.Block("static", tokens=[(20, 32768)], final=True)])
    assert dm.inflate(raw, d, 64)[:2] == (0, d[-32768:][:20])
    assert zlib_inflate(raw, d)[0] == d[-32768:][:20]


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("dict_len", dc.DICT_LENS)
def test_encode_cases_no_token_crosses_the_seam_and_zlib_reads_them(kind, dict_len):
    d = dc.dictionary(kind, dict_len)
    offs, lens = dc.blocks(kind)
    for o, n in zip(offs, lens):
        block = dc.master(kind)[o:o + n]
        for level in dc.ENC_LEVELS:
            assert dm.straddlers(d, block, level) == []
            toks = dm.expected_tokens(d, block, level)
            assert sum(max(ln, 1) for _, ln, _ in toks) == n
            assert all(v <= p + dm.used_of(dict_len) for p, ln, v in toks if ln)
            # the tokens rebuild the block behind the history
            hist = dm.history_of(d)
            out = bytearray(hist)
            for p, ln, v in toks:
                if ln == 0:
                    out.append(v)
                else:
                    for _ in range(ln):
                        out.append(out[-v])
            assert bytes(out[len(hist):]) == block


def test_the_dictionary_pays_on_text():
    """the condition the device's gain test rests on: 2 KiB text blocks against 32 KiB of the same text in front of them --
    the dictionary form's tokens are fewer, and a member made of them is smaller than the twin's plain member"""
    d = dc.dictionary("text", 32768)
    offs, lens = dc.blocks("text", (2048,) * 8)
    with_d = without = 0
    for o, n in zip(offs, lens):
        block = dc.master("text")[o:o + n]
        toks = dm.expected_tokens(d, block, 6)
        assert dm.dict_cost(toks)[0] > 0
        # the member of those tokens as a writer with optimal codes for them would make it
        member = dg.encode([dg.Block("dynamic", tokens=[v if ln == 0 else (ln, v) for _, ln, v in toks], final=True)])
        assert dm.member_tokens(member, dm.history_of(d)) == (toks, block)
        with_d += len(member)
        without += dm.plain_size(block, 6)
    assert with_d < without * 9 // 10, (with_d, without)
