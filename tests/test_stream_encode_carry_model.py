"""The model of the stream encoder whose chunks carry the window (tests/stream_encode_carry_model.py), held on the CPU to what
the GPU tests take from it: the seam is clean in the twin's one-block parse, the expected tokens of every chunk rebuild the
input with the bytes in front as history, and prime_of is right at its edges."""
import pytest

import hdtest
import stream_encode_carry_model as cm

N = 160 << 10


def data_of(kind):
    s = hdtest.synth()
    return bytes(s.text_like(N, seed=11) if kind == "text" else s.fastq_like(N, seed=12))


@pytest.mark.parametrize("s,want", [(0, 0), (1008, 0), (1024, 1024), (1040, 1024), (32767, 31744), (32768, 32768), (32784, 32768),
                                    ((1 << 32) + 16, 32768), ((1 << 40) + 1008, 32768)])
def test_prime_of_at_its_edges(s, want):
    assert cm.prime_of(1, s) == want
    assert cm.prime_of(s // 16, 16) == want                # the same start reached with the smallest chunk
    assert want % 1024 == 0 and want <= min(s, 32768) and (s - want) % 16 == s % 16


def test_prime_of_chunk_zero_and_growth():
    for chunk in (16, 1040, 16384, 49152, 65536, 64 << 20):
        assert cm.prime_of(0, chunk) == 0
        primes = [cm.prime_of(i, chunk) for i in range(0, 40)]
        assert primes == sorted(primes) and primes[-1] <= 32768
    assert [cm.prime_of(i, 1040) for i in (1, 2, 3, 31, 32, 33)] == [1024, 2048, 3072, 31744, 32768, 32768]
    assert [cm.prime_of(i, 16384) for i in (1, 2, 3)] == [16384, 32768, 32768]


@pytest.mark.parametrize("kind", ["text", "fastq"])
@pytest.mark.parametrize("level", [3, 6])
@pytest.mark.parametrize("chunk", [16384, 65536])
def test_seam_is_clean_and_tokens_rebuild_the_input(kind, level, chunk):
    data = data_of(kind)
    nchunks = (len(data) + chunk - 1) // chunk
    reached = 0
    for i in range(nchunks):
        s, prime, n = cm.span(data, i, chunk)
        assert cm.straddlers(data, i, chunk, level) == []
        toks = cm.expected_tokens(data, i, chunk, level)
        assert toks[0][0] == 0 and all(v <= p + prime for p, ln, v in toks if ln)
        assert cm.replay(data[s - prime:s], toks) == data[s:s + n]
        reached += sum(1 for p, ln, v in toks if ln and v > p)
    assert reached > nchunks                               # ... and the history is used: matches that reach over the seam


def test_chunk_zero_is_the_twins_own_parse():
    data = data_of("text")[:40000]
    r, coded = hdtest.oracle_twin(data[:16384], 6)
    assert r == 0
    import deflate_tokens
    own = [t for b in deflate_tokens.read(coded).blocks for t in b.tokens()]
    assert cm.expected_tokens(data, 0, 16384, 6) == own


def test_stream_tokens_reads_a_chunk_behind_its_history():
    """the reader the GPU tests use on the device's chunks, on a chunk built by hand: a static block with one literal and a
    match that reaches 3 bytes in front of the chunk, then the flush marker"""
    import deflate_gen as g
    raw = g.encode([g.Block("static", [ord("x"), (3, 4)])], chunk=True)
    assert raw[-4:] == b"\x00\x00\xff\xff"
    toks, out = cm.stream_tokens(raw, history=b"abc")
    assert toks == [(0, 0, ord("x")), (1, 3, 4)] and out == b"xabc"
