"""The two plain-Python index models (stream_index_model.index, stream_carry_model.index_carry) held to the oracle
(hdo_inflate, which test_deflate_gen.py pins to libdeflate) on every stream of the hand-built corpus but the cap_minus1
family, each taken as a one-row FRAME_RAW stream.  "Does not decode: bad data" has one meaning in this library, the
oracle's; the device index is held to these models (test_gpu_carry_rows.py), so the models are held to it here.

  * the oracle decodes the stream (OK, or INSUFFICIENT_SPACE in the room the case states): status 0, out_bytes the
    generator's size, end_offset the stream's length, a row per flush point the block list holds -- but the full-flush
    model answers 1 where a row behind an inner flush point reaches over its own start (named from the token lists);
  * the chunk form: status 2 at the end of the stream, the rows in front of it sum to the generator's size;
  * the oracle says BAD_DATA: status 1 or 2, never 0, and 2 exactly where the fault is that the input ran out -- a fixed
    list, which the family builder's intent gives."""
import pytest

import deflate_gen as dg
import hdtest
import stream_carry_model as cm
import stream_index_model as m

RAW = m.FRAME_RAW
BIG = 1 << 21

# the faults that are the input running out: what _Bits.over says at the element that failed
RAN_OUT = ("cut_in_stored_", "cut_in_static_", "cut_in_dynamic_", "stored_len_past_input_0", "stored_len_past_input_50",
           "stored_len_past_input_99", "stored_header_cut", "eob_len0", "empty_input")
# the ten the models once got wrong, with the oracle's verdict
ONCE_WRONG = {"litlen_incomplete": dg.BAD_DATA, "litlen_single_2bit": dg.BAD_DATA, "offset_incomplete_1_2": dg.BAD_DATA,
              "offset_single_2bit": dg.BAD_DATA, "offset_incomplete_two_2bit": dg.BAD_DATA,
              "static_lit286_off0": dg.OK, "static_lit287_off5": dg.OK, "static_lit285_off30": dg.OK,
              "static_lit257_off31": dg.OK, "static_lit286_off31": dg.OK}


def ran_out(name):
    return any(name == p or (p.endswith("_") and name.startswith(p)) for p in RAN_OUT)


def rows_of(blocks, chunk=False):
    """from the block list: (the rows' sizes as its flush points cut it, whether a row behind the first reaches over its
    own start).  An empty stored block that is not final is a flush point wherever it stands: it ends on a byte.  (The
    chunk form writes every block as non-final.)"""
    sizes, n, over = [], 0, False
    for b in blocks:
        if b.kind == "stored":
            if not b.data and (chunk or not b.final):
                sizes.append(n)
                n = 0
            n += len(b.data)
            continue
        for t in b.tokens:
            if isinstance(t, int):
                n += 1
            else:
                over = over or (bool(sizes) and t[1] > n)
                n += t[0]
    return sizes + [n], over


@pytest.fixture(scope="module")
def cases():
    return [c for c in dg.cached_corpus() if c.family != "cap_minus1"]


@pytest.fixture(scope="module")
def answers(cases):
    """per case: the oracle's (code, size) in a large room, the full-flush model's answer, the carry model's"""
    out = {}
    for c in cases:
        r, b = hdtest.oracle_inflate(c.stream, BIG)
        rf, bf = hdtest.oracle_inflate_flushed(c.stream, BIG)
        out[c.name] = ((r, len(b)), (rf, len(bf)), m.index(c.stream, RAW), cm.index_carry(c.stream, RAW))
    return out


def test_the_oracle_in_a_large_room_is_the_generator(cases, answers):
    for c in cases:
        (r, n), (rf, nf) = answers[c.name][:2]
        assert r == (dg.OK if c.code == dg.INSUFFICIENT_SPACE else c.code), c.name
        assert rf == (dg.OK if c.code_flushed == dg.INSUFFICIENT_SPACE else c.code_flushed), c.name
        if c.code == dg.OK:
            assert n == len(c.expected), c.name
        if c.code == dg.INSUFFICIENT_SPACE:
            assert n == c.cap + 1, c.name                    # (cap_over_on_*: one byte over the room)
        if c.chunk:
            assert nf == len(c.expected), c.name


def test_streams_the_oracle_decodes(cases, answers):
    n = nreach = 0
    for c in cases:
        (r, size), _, x, y = answers[c.name]
        if c.chunk or r != dg.OK:
            continue
        n += 1
        sizes, over = rows_of(c.blocks) if c.blocks else ([size], False)
        assert sum(sizes) == size, c.name
        want = {"nchunks": len(sizes), "out_bytes": size, "end_offset": len(c.stream), "status": 0}
        got = {k: y[0][k] for k in want}
        assert got == want, (c.name, "carry")
        assert y[3] == sizes and y[2] and sum(y[2]) == len(c.stream), c.name
        if over:
            nreach += 1
            assert x[0]["status"] == 1 and max(y[5][1:]) > 0, (c.name, "a row reaches over its start")
            continue
        assert {k: x[0][k] for k in want} == want, (c.name, "full flush")
        assert list(x[1:]) == list(y[1:5]) and y[5] == [0] * len(sizes), c.name
    assert n >= 380
    print("streams the oracle decodes: %d, of them with a row that reaches over its start: %d" % (n, nreach))


def test_chunk_forms(cases, answers):
    n = 0
    for c in cases:
        if not c.chunk:
            continue
        n += 1
        _, (rf, size), x, y = answers[c.name]
        assert rf == dg.OK and size == len(c.expected), c.name
        sizes, over = rows_of(c.blocks, True)                  # (the marker encode() puts behind the list ends the last row)
        want = {"nchunks": len(sizes), "out_bytes": size, "end_offset": len(c.stream), "status": 2}
        assert {k: y[0][k] for k in want} == want and y[3] == sizes, (c.name, "carry")
        if over:
            assert x[0]["status"] == 1, c.name
            continue
        assert {k: x[0][k] for k in want} == want and x[3] == sizes, (c.name, "full flush")
    assert n >= 50


def test_streams_the_oracle_refuses(cases, answers):
    seen = set()
    for c in cases:
        (r, _), _, x, y = answers[c.name]
        if c.chunk or r == dg.OK:
            continue
        assert r == dg.BAD_DATA, c.name
        want = 2 if ran_out(c.name) else 1
        assert (x[0]["status"], y[0]["status"]) == (want, want), c.name
        assert x[0] == y[0] and list(x[1:]) == list(y[1:5]), c.name          # (rows in front of the fault: dist_past_out_d1)
        seen.add(c.name)
    # every name of the fixed list is a case, and so are the families the list's prefixes stand for
    assert {"stored_len_past_input_0", "stored_len_past_input_50", "stored_len_past_input_99", "stored_header_cut",
            "eob_len0", "empty_input"} <= seen
    for p in ("cut_in_stored_", "cut_in_static_", "cut_in_dynamic_"):
        assert sum(1 for s in seen if s.startswith(p)) == 2, p
    past = [s for s in seen if s.startswith("dist_past_out_")]
    assert len(past) == len(dg.MATCH_DISTS) and not any(ran_out(s) for s in past)     # status 1: the carry model's reach rule on row 0


def test_the_ten_by_name(cases, answers):
    by = {c.name: c for c in cases}
    for name, code in ONCE_WRONG.items():
        (r, size), _, x, y = answers[name]
        assert r == code, name
        if code == dg.OK:
            assert not by[name].zlib and size == len(by[name].expected) and x[0]["status"] == y[0]["status"] == 0, name
            assert x[0]["out_bytes"] == y[0]["out_bytes"] == size
        else:
            assert x[0]["status"] == y[0]["status"] == 1, name
