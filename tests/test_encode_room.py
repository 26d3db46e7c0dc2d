"""The twin against the room model (encode_room.py), at every edge room of blocks planted at the fit edges.

This pins the twin's room rules before the GPU tests hold the kernels to them (test_gpu_encode_room.py), so the
GPU expectations are not the twin's word alone: every verdict and every member here is the model's, and the twin
(plain, flush, and the per-block codecs' latency forms, levels 0..9) must agree with it byte for byte."""
import pytest

import encode_room as er
import hdtest


def blocks():
    """name -> data: the families, the tiny blocks and the lengths at the segment, clamp and stored edges"""
    s = hdtest.synth()
    fq, tx, rnd = bytes(s.fastq_like(0x10000)), bytes(s.text_like(0x10000)), bytes(s.random_bytes(0x10000))
    out = {
        "empty": b"", "one": b"a", "two": b"ab", "three": b"abc",
        "text_5000": tx[:5000], "fastq_20000": fq[:20000], "random_3000": rnd[:3000],
        "mixed_30000": fq[:10000] + rnd[:10000] + bytes(5000) + tx[:5000],
        "zeros_ff00": bytes(0xff00),
    }
    for lv in (1, 2):
        n = er.LAT_SEG[lv]
        out["text_lat%d-1" % lv] = tx[:n - 1]
        out["text_lat%d" % lv] = tx[:n]
        out["fastq_lat%d+1" % lv] = fq[:n + 1]
    out["fastq_ff00"] = fq[:0xff00]
    out["zeros_65339"] = bytes(65339)
    out["random_65505"] = rnd[:65505]
    out["zeros_65536"] = bytes(65536)
    return out


def big_blocks():
    s = hdtest.synth()
    fq = bytes(s.fastq_like(er.SEG_LIMIT + 1))
    # (zeros: a whole-coded member would fit any room near HD_SEG_LIMIT -- only the segmented form may take the block)
    return {"fastq_seglimit": fq[:er.SEG_LIMIT], "fastq_seglimit+1": fq, "zeros_seglimit+1": bytes(er.SEG_LIMIT + 1)}


FORMS = [(False, False), (True, False), (False, True), (True, True)]       # (flush, latency)


def _twin(flush, latency):
    if latency:
        return hdtest.codec_twin_flush if flush else hdtest.codec_twin
    return hdtest.oracle_twin_flush if flush else hdtest.oracle_twin


def _agree(name, data, level, flush, latency):
    b = er.Block(data, level, flush)
    for room in b.edge_rooms(latency):
        want = b.choose(room, latency)
        r, got = _twin(flush, latency)(data, level, cap=room)
        assert (r == 0) == want.fits, (name, level, flush, latency, room, b.need, b.need_lat, len(got))
        if want.fits:
            assert got == want.member, (name, level, flush, latency, room, want.kind, len(got), len(want.member))
    return b


@pytest.mark.parametrize("level", range(10))
def test_twin_agrees_with_the_room_model(level):
    for name, data in blocks().items():
        for flush, latency in FORMS:
            _agree(name, data, level, flush, latency)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_twin_agrees_with_the_room_model_past_the_segment_limit(level):
    for name, data in big_blocks().items():
        for flush, latency in FORMS:
            _agree(name, data, level, flush, latency)


def test_flush_reserve_is_five_bytes():
    """the flush form keeps 5 bytes free for a suffix that takes 4 or 5: a member that would end exactly at the room
    is refused (level 1, b"abc": 9 bytes, but room 10)"""
    r, m = hdtest.oracle_twin_flush(b"abc", 1, cap=64)
    assert r == 0 and len(m) == 9
    assert hdtest.oracle_twin_flush(b"abc", 1, cap=9)[0] != 0
    assert hdtest.oracle_twin_flush(b"abc", 1, cap=10) == (0, m)
    assert er.Block(b"abc", 1, True).need == 10


def test_bgzf_latency_default_slot_falls_back():
    """the BGZF clamp puts the latency worst case above 65536 for every level-1 block of 65339..65536 bytes: the
    per-block codecs give the ordinary member there, however compressible the block is"""
    n = 65536
    assert er.seg_worst(n, er.LAT_SEG[1], False) + 26 > er.BGZF_MAX
    assert er.seg_worst(65338, er.LAT_SEG[1], False) + 26 <= er.BGZF_MAX
    assert er.seg_worst(65339, er.LAT_SEG[1], False) + 26 > er.BGZF_MAX
    assert er.seg_worst(65418, er.LAT_SEG[2], False) + 26 <= er.BGZF_MAX < er.seg_worst(65419, er.LAT_SEG[2], False) + 26
    r, m = hdtest.codec_twin(bytes(n), 1, cap=er.BGZF_MAX - 26)
    assert r == 0 and m == hdtest.oracle_twin(bytes(n), 1)[1]
    rnd = bytes(hdtest.synth().random_bytes(65506))
    assert er.stored_size(65505) + 26 == er.BGZF_MAX
    for lv in (1, 2):
        assert hdtest.codec_twin(rnd[:65505], lv, cap=er.BGZF_MAX - 26)[0] == 0
        assert hdtest.codec_twin(rnd, lv, cap=er.BGZF_MAX - 26)[0] != 0
