"""The hand-built DEFLATE corpus (tests/deflate_gen.py) pinned on the CPU: every valid stream inflates with zlib
to the token lists' bytes, the oracle gives every stream the verdict its family states (the exact code: each
invalid stream breaks one rule), libdeflate (oracle/_ref/libref.so) agrees on code and bytes, and the corpus
reaches the edges it is built for.  These check the generator and the oracle; tests/test_gpu_inflate_edges.py
puts the same corpus through the kernels."""
import zlib

import pytest

import deflate_gen as dg
import hdtest


@pytest.fixture(scope="module")
def cases():
    return dg.cached_corpus()


def _report(bad):
    return "%d mismatches, first: %s" % (len(bad), bad[:12])


def test_corpus_is_deterministic_and_sized(cases):
    names = [c.name for c in cases]
    assert len(names) == len(set(names)), "case names must be unique"
    assert 800 <= len(cases) <= 5000
    again = dg.corpus()
    assert [(c.name, c.stream, c.cap, c.code) for c in again] == [(c.name, c.stream, c.cap, c.code) for c in cases]


def test_valid_streams_inflate_with_zlib(cases):
    bad, n = [], 0
    for c in cases:
        if c.code_flushed != dg.OK or not c.zlib:
            continue
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(c.stream)
        except zlib.error as e:
            bad.append((c.name, str(e)))
            continue
        n += 1
        if out != c.expected:
            bad.append((c.name, "bytes"))
        elif c.chunk == d.eof or d.unused_data:
            bad.append((c.name, "end of stream"))
    assert not bad, _report(bad)
    assert n > 500


def test_libdeflate_only_forms_are_rejected_by_zlib(cases):
    """the forms zlib refuses and libdeflate decodes really are such forms"""
    only = [c for c in cases if not c.zlib and c.code == dg.OK]
    assert len(only) >= 8
    for c in only:
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(c.stream)


def test_oracle_verdicts_and_bytes(cases):
    bad = []
    for c in cases:
        r, out = hdtest.oracle_inflate(c.stream, c.cap)
        if r != c.code or (r == 0 and out != c.expected):
            bad.append((c.name, "plain", r, c.code))
        r, out = hdtest.oracle_inflate_flushed(c.stream, c.cap)
        if r != c.code_flushed or (r == 0 and out != c.expected):
            bad.append((c.name, "flushed", r, c.code_flushed))
    assert not bad, _report(bad)


@pytest.mark.ref
def test_libdeflate_agrees(cases):
    ref = hdtest.ref()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so not built")
    bad = []
    for c in cases:
        r, out = hdtest.call_dec(ref.libdeflate_inflate, c.stream, c.cap)
        if r != c.code or (r == 0 and out != c.expected):
            bad.append((c.name, c.family, r, c.code))
    assert not bad, _report(bad)


# what the corpus must keep reaching (counted from the token lists and code lengths as they were written):
# a later edit of the generator must not drop a family quietly
COVERAGE = {
    "dist_1726": 100, "dist_1727": 100,            # both sides of INF_NEAR
    "near_src_wraps_ring": 1000,                    # a ring source across the 2 KiB wrap
    "dst_wraps_ring": 1000,
    "far_src_crosses_piece": 500,                   # an HBM source across a 1 KiB piece edge
    "far": 2000, "near": 2000,
    "len_le8": 1000, "len_9_16": 1000,              # the lane groups of 8 and 16
    "overlap_le16": 500,
    "dist_eq_out": 100,
    "lit_code_gt9": 1000,                           # the slow bit-serial path (litlen table is 9 bits)
    "dist_code_gt8": 200,                           # ... and the 8-bit offset table
    "eob_15bit": 6, "eob_len15_defined": 6,
    "amp_1bit_285": 10000,
    "repeat_crosses_boundary_16": 1, "repeat_crosses_boundary_17": 1, "repeat_crosses_boundary_18": 1,
    "hlit_257": 2, "hlit_286": 10, "hlit_288": 2, "hdist_1": 10, "hdist_30": 10, "hdist_32": 2,
    "hclen_19": 5, "rle_plain": 10, "rle_split": 2,
    "litlen_286_287": 4, "offset_30_31": 4,
    "stored_empty": 5, "stored_65535": 16,
    **{"stored_align_%d" % k: 16 for k in range(8)},
    "chunk_form": 50,
}


def test_coverage(cases):
    tot = {}
    for c in cases:
        for k, v in c.stats.items():
            tot[k] = tot.get(k, 0) + v
    short = {k: (tot.get(k, 0), m) for k, m in COVERAGE.items() if tot.get(k, 0) < m}
    assert not short, short
    fams = {c.family for c in cases}
    for f in ("match_matrix", "code_shapes", "amplify", "blocks", "libdeflate_only", "faults", "cap_minus1", "chunk",
              "chunk_match_matrix", "chunk_code_shapes", "chunk_blocks", "chunk_amplify"):
        assert f in fams, f
    faults = {c.name for c in cases if c.family == "faults"}
    for f in ("btype3", "stored_nlen", "stored_len_past_input_50", "rep16_first", "repeat_overrun_16",
              "repeat_overrun_17", "repeat_overrun_18", "litlen_oversubscribed", "litlen_incomplete",
              "offset_incomplete_1_2", "precode_oversubscribed", "eob_len0", "dist_past_out_d1726",
              "dist_past_out_d32768", "cap_over_on_literal", "cap_over_on_match", "cap_over_on_stored", "empty_input"):
        assert f in faults, f
    assert sum(1 for c in cases if c.name.startswith("cut_in_")) >= 6
    # every valid stream with output also appears with one byte less room
    valid = [c for c in cases if c.code_flushed == dg.OK and c.expected]
    assert sum(1 for c in cases if c.family == "cap_minus1") == len(valid)
