"""The four DEFLATE decoders of the device against EACH OTHER, on the hand-built streams of tests/deflate_gen.py.

The latency decoder and the size pass share the code that reads a stream -- bit reader, block headers, the speculative
decode of a window and its walk (7bgzf_amd/csrc/hd_inflate_common.hpp).  The throughput decoder keeps its OWN COPY of
every one of those pieces (its speed and its register budget: DESIGN.md 4.3c), and all three keep their own copy of the
scalar path's token decode.  The other tests hold each decoder to the oracle separately; this one is the only thing that
holds the copies to the shared code and to one another, stream by stream:

    k_inflate          the batch decode                        (status, bytes out)
    k_inflate_framed   the framed decode, raw frame            (status, bytes out, bytes consumed)
    k_inflate_lat      hip_inflate, one lone call per stream   (status, bytes out)
    k_inflate_size     the size pass, raw frame                (status, size, bytes consumed)

The streams are every member, valid and invalid, of the families built around the edges of that shared code: the header
edges (code_shapes: every shape of code and of its run-length coding; blocks: stored blocks at every bit alignment, empty
and tiny blocks, a header behind a 258-byte match; faults: every reject rule once) and the token edges (match_matrix:
lengths and distances at every boundary, a distance of exactly the bytes out and one more; libdeflate_only: the symbols
286 / 287 / 30 / 31).  Every decoder must give every stream the same status; where that is OK, the same output size --
the generator's -- and, from the two that report it, the same bytes consumed: the whole stream.
(The piece decoders of the stream indexes, k_inflate_piece and k_carry_piece, and the carry decoder k_carry_decode are held to
the same streams in tests/test_gpu_carry_rows.py, through models that tests/test_index_models_vs_oracle.py pins to the oracle.)

The size pass takes no room.  A stream that the others refuse for the room alone (cap_over_on_*: HD_INSUFFICIENT_SPACE one
byte short) it must size as OK, at exactly one byte more than that room -- the same finding from the other side."""
import os

import pytest

import deflate_gen as dg
import hdtest

pytestmark = pytest.mark.gpu

HEADER_EDGE = ("code_shapes", "blocks", "faults")
TOKEN_EDGE = ("match_matrix", "libdeflate_only")


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.mark.timeout(120)
def test_four_decoders_agree_on_header_and_token_edges(pkg):
    cases = [c for c in dg.cached_corpus() if c.family in HEADER_EDGE + TOKEN_EDGE]
    assert len(cases) >= 500 and {c.family for c in cases} == set(HEADER_EDGE + TOKEN_EDGE)
    assert sum(1 for c in cases if c.code != dg.OK) >= 60
    streams, caps = [c.stream for c in cases], [c.cap for c in cases]
    outs_b, _, st_b = pkg.batch_inflate(streams, caps)
    outs_f, _, used_f, st_f = pkg.batch_inflate_framed(streams, caps, pkg.FRAME_RAW)
    size_s, used_s, st_s = pkg.batch_inflate_size(streams, pkg.FRAME_RAW)
    bad = []
    for i, c in enumerate(cases):
        st_l, out_l = pkg.hip_inflate(c.stream, c.cap)
        got = {"batch": int(st_b[i]), "framed": int(st_f[i]), "lat": int(st_l), "size": int(st_s[i])}
        want = dict.fromkeys(got, c.code)
        if c.code == dg.INSUFFICIENT_SPACE:
            want["size"] = dg.OK                   # no room to run out of: the size is the answer (checked below)
        if got != want:
            bad.append((c.name, "status", got, c.code))
            continue
        if c.code == dg.INSUFFICIENT_SPACE:
            if int(size_s[i]) != c.cap + 1:
                bad.append((c.name, "size of a stream one byte over its room", int(size_s[i]), c.cap + 1))
            continue
        if c.code != dg.OK:
            continue
        sizes = {"batch": len(outs_b[i]), "framed": len(outs_f[i]), "lat": len(out_l), "size": int(size_s[i])}
        if set(sizes.values()) != {len(c.expected)}:
            bad.append((c.name, "bytes out", sizes, len(c.expected)))
        if not (int(used_f[i]) == int(used_s[i]) == len(c.stream)):
            bad.append((c.name, "bytes consumed", int(used_f[i]), int(used_s[i]), len(c.stream)))
    assert not bad, "%d disagreements, first: %s" % (len(bad), bad[:12])
