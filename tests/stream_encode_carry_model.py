"""The model of the stream encoder whose chunks carry the window (hipdeflate_stream_deflate_carry_dev, levels 3..9).

Chunk i, which starts at input byte s = i * chunk_bytes, is parsed with prime(i) = min(32768, s) & ~1023 bytes in front of
it as its history, and its tokens are those a ONE-BLOCK parse of (history || chunk) makes behind the seam.  The one-block
parse is the CPU twin's (oracle/hd_deflate_twin.c through hdtest.oracle_twin), read back with the plain-Python token reader
(deflate_tokens.read): nothing here knows the kernel.

  prime_of(i, chunk_bytes)                   the history's length
  expected_tokens(data, i, chunk_bytes, lv)  chunk i's tokens in chunk coordinates: (pos, length, value) triples, value a
                                             literal's byte (length 0) or a match's distance -- which may reach up to
                                             prime_of(i) bytes in front of position 0
  straddlers(data, i, chunk_bytes, lv)       the tokens of that parse that start in front of the seam and end behind it
                                             (none, for the model to stand: the seam is a piece boundary, and no match
                                             crosses one)
  replay(history, tokens)                    the bytes the tokens make with `history` in front of them
  stream_tokens(raw)                         the tokens of a chunk's bytes as they stand in a stream (positions from 0)
"""
import deflate_tokens
import hdtest

WINDOW = 32768          # include/hipdeflate_params.h HD_WG_WINDOW
PIECE = 1024            # ... HD_WG_CUT


def prime_of(i, chunk_bytes):
    s = i * chunk_bytes
    return min(WINDOW, s) & ~(PIECE - 1)


def span(data, i, chunk_bytes):
    """-> (s, prime, n): chunk i's start, its history's length and its own"""
    s = i * chunk_bytes
    assert 0 <= s < len(data) or (s == 0 and not data)
    return s, prime_of(i, chunk_bytes), min(chunk_bytes, len(data) - s)


_parse = {}


def _one_block(data, i, chunk_bytes, level):
    """every token of the twin's one-block parse of (history || chunk i), positions from the history's first byte"""
    s, prime, n = span(data, i, chunk_bytes)
    both = bytes(data[s - prime:s + n])
    key = (hdtest.sha(both), level)
    if key not in _parse:
        r, coded = hdtest.oracle_twin(both, level)
        assert r == 0
        st = deflate_tokens.read(coded)
        assert st.out == both
        _parse[key] = [t for b in st.blocks for t in b.tokens()]
    return _parse[key], prime


def straddlers(data, i, chunk_bytes, level):
    toks, prime = _one_block(data, i, chunk_bytes, level)
    return [(p, ln, v) for p, ln, v in toks if p < prime < p + max(ln, 1)]


def expected_tokens(data, i, chunk_bytes, level):
    toks, prime = _one_block(data, i, chunk_bytes, level)
    return [(p - prime, ln, v) for p, ln, v in toks if p >= prime]


def replay(history, tokens):
    out = bytearray(history)
    base = len(out)
    for p, ln, v in tokens:
        assert p == len(out) - base, (p, len(out) - base)
        if ln == 0:
            out.append(v)
        else:
            assert 1 <= v <= len(out), (p, ln, v)
            for _ in range(ln):
                out.append(out[-v])
    return bytes(out[base:])


def stream_tokens(raw, history=b""):
    """the tokens of one chunk's DEFLATE bytes (blocks up to and including the empty stored block of its flush), and the
    bytes they make with `history` in front.  The reader refuses a distance past what it has produced, so the history is
    given to it as a stored block in front."""
    assert len(history) <= 0xffff
    lead = b""
    if history:
        lead = bytes([0]) + len(history).to_bytes(2, "little") + (len(history) ^ 0xffff).to_bytes(2, "little") + bytes(history)
    st = deflate_tokens.read(lead + bytes(raw), stop_at_final=False)
    h = len(history)
    blocks = st.blocks[1:] if history else st.blocks
    assert blocks and blocks[-1].sync_flush, "a chunk ends in the empty stored block"
    toks = [(p - h, ln, v) for b in blocks for (p, ln, v) in b.tokens()]
    return toks, st.out[h:]
