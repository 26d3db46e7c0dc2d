"""The per-call decoder (hip_inflate, hip_inflate_flush: k_inflate_lat, hd_inflate_lat.hpp) past its 64 KiB LDS
ring, on the MI355X: the second hand-built corpus (deflate_gen.lat_corpus, pinned on the CPU by
tests/test_deflate_gen.py) and streams real encoders make of [random | text | random | text].  Exact status and
exact bytes, no tolerance, no case left out.

What the families reach in that kernel:
  * lat_wrap -- ring indices across the 64 KiB wrap: a window's lane-group and general copies, the scalar path's
    literal and match records, a stored block, the budget-cut windows of a 200 KiB run.  Match filler only: no
    large record is in flight, so a failure here is a failure of the wrap.
  * lat_lead -- the sort wavefront stores a window's literals into the ring ahead of the back wavefront.  Behind
    stored blocks the records between the two stand for more output than the ring's spare 32 KiB; the sort has
    to wait for the back (hd_inflate_lat.hpp, "the lead") or its literals land on bytes the back has not
    flushed, has not copied from, or has not written yet.
  * lat_sizes -- outputs around 64 KiB, 128 KiB and 1 MiB, the largest room the latency kernel takes; one byte
    more goes alone through the batch kernel.
The batch entry point (k_inflate: a 2 KiB ring with far paths, no sort wavefront) decodes the same streams as the
control: it tells a wrong stream from a wrong kernel.

The latency kernel gives up a wait between its wavefronts after INF_LAT_SPINS with HD_BAD_DATA: a valid stream
that comes back non-zero is a failure."""
import os
import threading
import zlib

import numpy as np
import pytest

import deflate_gen as dg
import hdtest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


@pytest.fixture(scope="module")
def cases():
    return dg.cached_lat_corpus()


def _first_diff(a, b):
    n = min(len(a), len(b))
    x = np.frombuffer(a, dtype=np.uint8, count=n) != np.frombuffer(b, dtype=np.uint8, count=n)
    return int(np.argmax(x)) if x.any() else n


def _check(name, want, expected, r, out):
    if r != want:
        return (name, "status", r, want)
    if want == 0 and out != expected:
        return (name, "bytes", "first differing offset %d" % _first_diff(out, expected), len(out), len(expected))
    return None


def _report(bad):
    return "%d mismatches: %s" % (len(bad), bad)     # (all of them: which cases fail together is the finding)


def _batch(pkg, cs, flushed):
    outs, crc, st = pkg.batch_inflate([c.stream for c in cs], [c.cap for c in cs], flushed=flushed)
    bad = []
    for i, c in enumerate(cs):
        w = c.code_flushed if flushed else c.code
        e = _check(c.name, w, c.expected, int(st[i]), outs[i])
        if not e and w == 0 and (int(crc[i]) & 0xffffffff) != zlib.crc32(c.expected):
            e = (c.name, "crc")
        if e:
            bad.append(e)
    return bad


@pytest.mark.timeout(300)
def test_control_batch_inflate_one_launch(pkg, cases):
    """the control: the whole corpus through the batch kernel in one launch, and again through the flushed entry
    point, where the chunk forms decode"""
    bad = _batch(pkg, cases, False) + _batch(pkg, cases, True)
    assert not bad, _report(bad)
    assert sum(1 for c in cases if c.chunk and c.code_flushed == dg.OK) >= 3


def _call(pkg, c):
    f = pkg.hip_inflate_flush if c.chunk else pkg.hip_inflate
    return _check(c.name, c.code_flushed if c.chunk else c.code, c.expected, *f(c.stream, c.cap))


@pytest.mark.timeout(300)
def test_hip_inflate_lone_calls(pkg, cases):
    """one call at a time (the chunk forms through hip_inflate_flush), and the chunk forms through hip_inflate
    too, where they must be refused"""
    bad = [e for e in (_call(pkg, c) for c in cases) if e]
    for c in cases:
        if c.chunk:
            r, _ = pkg.hip_inflate(c.stream, c.cap)
            if r != c.code:
                bad.append((c.name, "plain", r, c.code))
    assert not bad, _report(bad)


@pytest.mark.timeout(300)
def test_hip_inflate_from_16_threads(pkg, cases):
    """the same from 16 threads, cases[k::16] each: calls of every size share batches (a batch's arena admits four
    1 MiB callers)"""
    bad, lock = [], threading.Lock()

    def work(k):
        for c in cases[k::16]:
            e = _call(pkg, c)
            if not e and c.chunk:
                r, _ = pkg.hip_inflate(c.stream, c.cap)
                e = (c.name, "plain", r, c.code) if r != c.code else None
            if e:
                with lock:
                    bad.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, _report(bad)


@pytest.mark.timeout(300)
def test_room_around_the_largest_call(pkg, cases):
    """lat_sizes with seven bytes of room to spare (the same bytes) and one byte short (3); the 1 MiB case is the
    last the latency kernel takes, 1 MiB + 1 goes alone"""
    sized = [c for c in cases if c.family == "lat_sizes"]
    assert {len(c.expected) for c in sized} >= {dg.LAT_MAX_OUT, dg.LAT_MAX_OUT + 1} and len(sized) == 18
    bad = []
    for c in sized:
        n = len(c.expected)
        for cap, want in ((n, dg.OK), (n + 7, dg.OK), (n - 1, dg.INSUFFICIENT_SPACE)):
            e = _check("%s cap %d" % (c.name, cap), want, c.expected, *pkg.hip_inflate(c.stream, cap))
            if e:
                bad.append(e)
    assert not bad, _report(bad)


# ---- real encoders, made on the spot ----------------------------------------------------------------------------


def _mixed(rnd):
    s = hdtest.synth()
    rng = np.random.default_rng(rnd)
    parts = []
    for k in range(2):
        parts.append(rng.integers(0, 256, rnd, dtype=np.uint8).tobytes())
        parts.append(bytes(s.text_like(300000, seed=70 + k)))
    return b"".join(parts)[:dg.LAT_MAX_OUT]


@pytest.fixture(scope="module")
def encoded(pkg):
    """[(name, flushed, stream, input)]: zlib 0 / 1 / 6 / 9 raw, zlib 6 full-flushed every 100,000 bytes (no final
    block: the flushed entry point's form), our own levels 1 and 6 as one FRAME_RAW member of batch_deflate"""
    jobs = []
    for rnd in (60 << 10, 200 << 10):
        data = _mixed(rnd)
        assert rnd + 300000 < len(data) <= dg.LAT_MAX_OUT
        for level in (0, 1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            z = c.compress(data) + c.flush()
            # what keeps the case what it claims to be: the stream opens with stored blocks -- of more than the
            # ring where the random bytes are that many; where they are 60 KiB, of more than the ring's spare
            # half (zlib ends a block when its buffer of 16 Ki symbols is full, not where the random bytes end:
            # the last block of them is shared with the text and is not stored)
            lead = dg.stored_lead(z)
            print("zlib %d, %d random bytes: stored lead %d" % (level, rnd, lead))
            assert lead > (dg.LAT_RING if rnd > dg.LAT_RING or level == 0 else dg.LAT_RING // 2), (level, rnd, lead)
            jobs.append(("zlib%d_r%d" % (level, rnd), False, z, data))
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = b"".join(c.compress(data[o:o + 100000]) + c.flush(zlib.Z_FULL_FLUSH) for o in range(0, len(data), 100000))
        assert z.endswith(b"\x00\x00\xff\xff")
        lead = dg.stored_lead(z)
        print("zlib 6 full-flushed, %d random bytes: stored lead %d" % (rnd, lead))
        assert lead > (dg.LAT_RING if rnd > dg.LAT_RING else dg.LAT_RING // 2), (rnd, lead)
        jobs.append(("zlib6_fullflush_r%d" % rnd, True, z, data))
        for level in (1, 6):
            members, _, st = pkg.batch_deflate(data, [0], [len(data)], level, pkg.FRAME_RAW)
            assert int(st[0]) == 0, (level, int(st[0]))
            assert zlib.decompressobj(-15).decompress(members[0]) == data
            jobs.append(("own%d_r%d" % (level, rnd), False, members[0], data))
    return jobs


def _decode(pkg, job):
    name, flushed, z, data = job
    f = pkg.hip_inflate_flush if flushed else pkg.hip_inflate
    return _check(name, dg.OK, data, *f(z, len(data)))


@pytest.mark.timeout(300)
def test_real_encoders_lone_and_8_threads(pkg, encoded):
    """each stream lone, then all of them from 8 threads at once, against the input and against the batch kernel's
    decode of the same stream"""
    bad = []
    for flushed in (False, True):
        js = [j for j in encoded if j[1] == flushed]
        outs, _, st = pkg.batch_inflate([j[2] for j in js], [len(j[3]) for j in js], flushed=flushed)
        bad += [e for e in (_check(j[0] + " (batch)", dg.OK, j[3], int(st[i]), outs[i]) for i, j in enumerate(js)) if e]
    bad += [e for e in (_decode(pkg, j) for j in encoded) if e]
    lock = threading.Lock()

    def work(k):
        for j in (encoded * 2)[k::8]:
            e = _decode(pkg, j)
            if e:
                with lock:
                    bad.append((e[0] + " (8 threads)",) + e[1:])

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, _report(bad)
