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


# ---- the second corpus: the latency kernel's geometry (deflate_gen.lat_corpus; tests/test_gpu_inflate_lat_ring.py
# puts it through the kernels) ---------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lat_cases():
    return dg.cached_lat_corpus()


def test_lat_corpus_is_deterministic_and_within_budget(lat_cases):
    """the budget: at most 400 cases, 64 MiB of expected output, no output past 1 MiB but the cases that are
    1 MiB + 1 on purpose; generated in a few seconds (two to nine on the machines tried: the bound leaves room for
    a loaded one and still fails a filler made of literal tokens)"""
    import time
    names = [c.name for c in lat_cases]
    assert len(names) == len(set(names)), "case names must be unique"
    assert 100 <= len(lat_cases) <= 400
    t0 = time.monotonic()
    again = dg.lat_corpus()
    dt = time.monotonic() - t0
    print("lat_corpus(): %.1f s" % dt)
    assert dt < 15
    assert [(c.name, c.stream, c.cap, c.code) for c in again] == [(c.name, c.stream, c.cap, c.code) for c in lat_cases]
    assert sum(len(c.expected) for c in lat_cases) <= 64 << 20
    over = sorted(c.name for c in lat_cases if max(len(c.expected), c.cap) > dg.LAT_MAX_OUT)
    assert over == ["lat_size_1048577_fill", "lat_size_1048577_stored_text"], over
    assert all(len(c.expected) == dg.LAT_MAX_OUT + 1 for c in lat_cases if c.name in over)
    assert not set(names) & {c.name for c in dg.cached_corpus()}


def test_lat_valid_streams_inflate_with_zlib(lat_cases):
    bad, n = [], 0
    for c in lat_cases:
        if c.code_flushed != dg.OK:
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
    assert n >= 140


def test_lat_oracle_verdicts_and_bytes(lat_cases):
    bad = []
    for c in lat_cases:
        r, out = hdtest.oracle_inflate(c.stream, c.cap)
        if r != c.code or (r == 0 and out != c.expected):
            bad.append((c.name, "plain", r, c.code))
        r, out = hdtest.oracle_inflate_flushed(c.stream, c.cap)
        if r != c.code_flushed or (r == 0 and out != c.expected):
            bad.append((c.name, "flushed", r, c.code_flushed))
    assert not bad, _report(bad)


@pytest.mark.ref
def test_lat_libdeflate_agrees(lat_cases):
    ref = hdtest.ref()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so not built")
    bad = []
    for c in lat_cases:
        r, out = hdtest.call_dec(ref.libdeflate_inflate, c.stream, c.cap)
        if r != c.code or (r == 0 and out != c.expected):
            bad.append((c.name, c.family, r, c.code))
    assert not bad, _report(bad)


def test_stored_lead_parser():
    a, b = bytes(range(200)), bytes(70000)
    assert dg.stored_lead(zlib.compress(a, 0)[2:-4]) == 200
    assert dg.stored_lead(zlib.compress(b, 0)[2:-4]) == 70000
    assert dg.stored_lead(zlib.compress(b, 6)[2:-4]) == 0
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    s = c.compress(a) + c.flush(zlib.Z_FULL_FLUSH)
    c6 = zlib.compressobj(6, zlib.DEFLATED, -15)
    assert dg.stored_lead(s) == 200 and dg.stored_lead(s + c6.compress(b) + c6.flush()) == 200
    # the hand-built streams: the stored blocks in front of the first Huffman block, from the block lists
    for c in dg.cached_lat_corpus():
        if c.blocks and not c.chunk:
            want = 0
            for blk in c.blocks:
                if blk.kind != "stored":
                    break
                want += len(blk.data)
            assert dg.stored_lead(c.stream) == want, c.name


LAT_COVERAGE = {
    "lat_dst_wraps_ring": 300,                      # a match's destination across a multiple of 64 KiB
    "lat_src_wraps_ring": 300,                      # ... its source
    "lat_stored_wraps_ring": 3,
    "lat_inflight_ge_64k": 30,                      # a block of literals behind stored records of a ring's worth and more
    "lat_inflight_32k_64k": 8,
    "lat_out_gt_64k": 100,
    "lat_out_1mib": 4,
    "lit_code_gt9": 100,                            # the scalar path's records across the wrap
    "amp_1bit_285": 794,
    "stored_65535": 60,
    "chunk_form": 3,
    **{"lat_wrap_" + k: 25 for k in ("dA", "dB", "d0", "d1", "sA", "sB", "s0", "s1")},
    **{"lat_wrap_m%d" % m: 35 for m in (1, 2, 15)},
}


def test_lat_coverage(lat_cases):
    tot = {}
    for c in lat_cases:
        for k, v in c.stats.items():
            tot[k] = tot.get(k, 0) + v
    short = {k: (tot.get(k, 0), m) for k, m in LAT_COVERAGE.items() if tot.get(k, 0) < m}
    assert not short, short
    # every (length, distance) with its destination across the wrap at both phases that span it, and once more
    pairs = {k: tot.get("lat_wrap_pair_%d_%d" % k, 0) for k in ((ln, d) for ln in dg.MATCH_LENGTHS for d in dg.LAT_WRAP_DISTS)}
    assert min(pairs.values()) >= 2, {k: v for k, v in pairs.items() if v < 2}
    assert tot["lat_wrap_dA"] == tot["lat_wrap_dB"] == len(pairs)
    fams = {c.family for c in lat_cases}
    for f in ("lat_wrap", "lat_lead", "lat_sizes", "cap_minus1", "chunk_lat_wrap", "chunk_lat_lead", "chunk_lat_sizes"):
        assert f in fams, f
    sizes = {len(c.expected) for c in lat_cases if c.family == "lat_sizes"}
    assert sizes == set(dg.LAT_SIZES)
    assert all(sum(1 for c in lat_cases if c.family == "lat_sizes" and len(c.expected) == n) == 2 for n in sizes)
    lead = {c.name for c in lat_cases if c.family == "lat_lead"}
    for kind in ("static", "dynamic"):
        for f in ["lat_lead_one_%d_at_%d" % (L, b) for L in (32768, 57344, 61440, 65535) for b in (0, 1000, 40000, 65613)] + \
                 ["lat_lead_%dx16383" % k for k in (4, 5, 9, 12)] + ["lat_lead_%dx65535" % k for k in (2, 3, 15)] + \
                 ["lat_lead_alternating_x6", "lat_lead_match_first"]:
            assert f + "_" + kind in lead, f
    # every valid case with output also appears with one byte less room
    valid = [c for c in lat_cases if c.code_flushed == dg.OK and c.expected]
    assert sum(1 for c in lat_cases if c.family == "cap_minus1") == len(valid)
