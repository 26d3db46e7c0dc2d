"""The model of the preset-dictionary calls (hipdeflate_batch_deflate_dict*, hipdeflate_batch_inflate_dict*).

ENCODE, levels 3..9.  Every block of a call is parsed with the LAST used = min(32768, dict_len) & ~1023 bytes of the dictionary
as its history, and its tokens are those a ONE-BLOCK parse of (history || block) makes behind the seam.  The one-block parse
is the CPU twin's (oracle/hd_deflate_twin.c through hdtest.oracle_twin), read back with the plain-Python token reader
(deflate_tokens.read), as tests/stream_encode_carry_model.py does for the stream whose chunks carry the window.

DECODE.  A member starts with the dictionary's last D = min(32768, dict_len) bytes as its window: what it answers is what the
oracle's inflate answers for (a stored block of those bytes || the member) with the lead stripped.  The zlib wrapper's rules
with FDICT and DICTID are restated from RFC 1950 and lib/zlib/inflate.c:810-822, 1298-1329 (paths relative to the reference).

Nothing here knows the kernels; tests/test_dict_model.py holds the model to Python's zlib.

  used_of(dict_len)                        the history's length on the encode side
  expected_tokens(dictionary, block, lv)   the block's tokens in block coordinates: (pos, length, value) triples, value a
                                           literal's byte (length 0) or a match's distance, up to used_of() in front of 0
  straddlers(dictionary, block, lv)        tokens of that parse that start in front of the seam and end behind it (none)
  plain_size(block, lv)                    the bytes of the twin's member for the block alone
  member_tokens(raw, history)              the tokens of a member that ends in a final block, and the bytes they make
  inflate(raw, dictionary, cap)            (status, output, bits of `raw` used) of a raw member
  member(m, frame, dictionary, cap)        (status, out_len, in_used, check, output) of the decode call for one member
  zlib_header(dictionary, level_bits=2)    the six header bytes of a zlib member that names the dictionary
"""
import zlib

import deflate_tokens
import framed_model
import hdtest

WINDOW = 32768          # include/hipdeflate_params.h HD_WG_WINDOW
PIECE = 1024            # ... HD_WG_CUT
RAW, ZLIB = framed_model.RAW, framed_model.ZLIB
OK, BAD_DATA, INSUFFICIENT_SPACE = framed_model.OK, framed_model.BAD_DATA, framed_model.INSUFFICIENT_SPACE


def used_of(dict_len):
    return min(WINDOW, dict_len) & ~(PIECE - 1)


def history_of(dictionary):
    """the bytes of the dictionary the encoder parses a block with"""
    used = used_of(len(dictionary))
    return bytes(dictionary[len(dictionary) - used:]) if used else b""


_parse = {}


def _one_block(dictionary, block, level):
    """every token of the twin's one-block parse of (history || block), positions from the history's first byte"""
    hist = history_of(dictionary)
    both = hist + bytes(block)
    key = (hdtest.sha(both), len(hist), level)
    if key not in _parse:
        r, coded = hdtest.oracle_twin(both, level)
        assert r == 0
        st = deflate_tokens.read(coded)
        assert st.out == both
        _parse[key] = [t for b in st.blocks for t in b.tokens()]
    return _parse[key], len(hist)


def straddlers(dictionary, block, level):
    toks, used = _one_block(dictionary, block, level)
    return [(p, ln, v) for p, ln, v in toks if p < used < p + max(ln, 1)]


def expected_tokens(dictionary, block, level):
    toks, used = _one_block(dictionary, block, level)
    return [(p - used, ln, v) for p, ln, v in toks if p >= used]


def plain_size(block, level):
    r, coded = hdtest.oracle_twin(bytes(block), level)
    assert r == 0
    return len(coded)


def stored_lead(history):
    """`history` as one stored, non-final block: what puts it into a reader's window"""
    assert len(history) <= 0xffff
    if not history:
        return b""
    return bytes([0]) + len(history).to_bytes(2, "little") + (len(history) ^ 0xffff).to_bytes(2, "little") + bytes(history)


def member_tokens(raw, history=b""):
    """the tokens of one member's DEFLATE bytes (blocks up to and including the final one) and the bytes they make with
    `history` in front.  The reader refuses a distance past what it has produced, so the history is given to it as a
    stored block in front."""
    st = deflate_tokens.read(stored_lead(history) + bytes(raw))
    h = len(history)
    blocks = st.blocks[1:] if history else st.blocks
    assert blocks and blocks[-1].final, "a member ends in a final block"
    assert (st.end_bit + 7) // 8 == st.nbytes, "nothing behind the final block"
    toks = [(p - h, ln, v) for b in blocks for (p, ln, v) in b.tokens()]
    return toks, st.out[h:]


def dict_cost(toks):
    """matches that reach in front of the block: (count, bytes they cover)"""
    reach = [(p, ln, v) for p, ln, v in toks if ln and v > p]
    return len(reach), sum(ln for _, ln, _ in reach)


# ---- decode -------------------------------------------------------------------------------------------------------------

def window_of(dictionary):
    return bytes(dictionary[max(0, len(dictionary) - WINDOW):])


def inflate(raw, dictionary, cap):
    """-> (status, output, bits of `raw` consumed): a raw member whose window starts out as the dictionary's last 32 KiB"""
    lead = stored_lead(window_of(dictionary))
    d = len(lead) - 5 if lead else 0
    r, out, bits = framed_model.oracle_inflate_bits(lead + bytes(raw), cap + d)
    if r:
        return r, b"", 0
    return OK, out[d:], bits - 8 * len(lead)


def zlib_header(dictionary, cmf=0x78, level_bits=2):
    """CMF, FLG with FDICT and a valid FCHECK, DICTID big-endian"""
    flg = (level_bits << 6) | 0x20
    flg += 31 - ((cmf << 8) | flg) % 31
    return bytes([cmf, flg]) + zlib.adler32(bytes(dictionary)).to_bytes(4, "big")


def open_zlib(m, dictionary):
    """-> (offset of the DEFLATE payload, whether the member names the dictionary), or None where the rules refuse it"""
    n = len(m)
    if n < 6:
        return None
    hdr = (m[0] << 8) | m[1]
    if hdr % 31 or ((hdr >> 8) & 15) != 8 or (hdr >> 12) > 7:
        return None
    if not (hdr >> 5) & 1:
        return 2, False
    # FDICT: DICTID and the trailer behind it; the dictionary is the one given, whole -- and one must have been given
    if n < 10 or not len(dictionary):
        return None
    if int.from_bytes(m[2:6], "big") != zlib.adler32(bytes(dictionary)):
        return None
    return 6, True


def member(m, frame, dictionary, cap):
    """-> (status, out_len, in_used, check, output): hipdeflate_batch_inflate_dict* for one member and `cap` bytes of room"""
    m = bytes(m)
    fail = lambda code: (code, 0, 0, 0, b"")
    if len(m) >= framed_model.MAX_IN:
        return fail(BAD_DATA)
    if frame == RAW:
        pos, foot, named = 0, 0, True
    else:
        assert frame == ZLIB
        opened = open_zlib(m, dictionary)
        if opened is None:
            return fail(BAD_DATA)
        (pos, named), foot = opened, 4
    r, out, bits = inflate(m[pos:len(m) - foot], dictionary if named else b"", cap)
    if r:
        return fail(r)
    used = (bits + 7) // 8
    if frame == ZLIB:
        check = zlib.adler32(out)
        if int.from_bytes(m[pos + used:pos + used + 4], "big") != check:
            return fail(BAD_DATA)
    else:
        check = zlib.crc32(out)
    return OK, len(out), pos + used + foot, check, out
