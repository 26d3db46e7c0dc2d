"""The streaming encoder and decoder (hipdeflate_pipe_*, hipdeflate_unpipe_*) driven call by call, the way a caller
that does `n = read(0, buf, cap); submit(n)` drives them -- not through the convenience loops pipe_compress /
unpipe_decompress.  tests/pipe_model.py says which blocks a batch consists of, what a result must hold and when
input() may be called; every single-threaded driver here asks it before each input(), so no test can block.

Expected bytes always come from outside the pipe: pkg.batch_deflate on the model's block table in the same frame,
level and slot (itself pinned to the CPU twin elsewhere), a seeded sample of members against the twin directly, the
decoder's output against the encoder's input and the oracle's inflate.  Bit-exact, no tolerances."""
import base64
import ctypes
import json
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import hdtest
import pipe_model as pm

pytestmark = pytest.mark.gpu

# (level, frame, block_bytes)
CONFIGS = [(1, "bgzf", 0xff00), (2, "bgzf", 0xff00), (3, "bgzf", 0xff00), (6, "migz", 65536), (1, "raw_flush", 4096),
           (0, "bgzf", 0xff00), (6, "gzip", 65536), (1, "zlib", 8192)]
DEPTHS = [2, 4]
P = 3                                           # blocks_per_batch of every pattern but "p1"
HEAD_TAIL = {"bgzf": (18, 8), "migz": (20, 8), "gzip": (10, 8), "zlib": (2, 4), "raw_flush": (0, 0)}
HD_INFLATE_MAX_IN = 1 << 28                     # include/hipdeflate_params.h
JOIN_S = 120


@pytest.fixture(scope="module")
def pkg():
    p = hdtest.pkg()
    assert os.path.exists(p.LIB_PATH), "libhipdeflate.so missing: run __graft_entry__.build()"
    assert p.available(), "no usable MI355X: the HIP path must be the one that runs"
    return p


def make_source():
    s = hdtest.synth()
    return bytes(s.fastq_like(3 << 20, seed=31)) + bytes(s.text_like(1 << 20, seed=32))


@pytest.fixture(scope="module")
def source():
    return make_source()


def frame_id(pkg, frame):
    return {"bgzf": pkg.FRAME_BGZF, "migz": pkg.FRAME_MIGZ, "gzip": pkg.FRAME_GZIP, "zlib": pkg.FRAME_ZLIB,
            "raw_flush": pkg.FRAME_RAW_FLUSH}[frame]


def slot_of(pkg, level, frame, B):
    """the slot the header states for a pipe: hipdeflate_bound, a BGZF member never above 65536"""
    slot = int(pkg.lib().hipdeflate_bound(B, level))
    return min(slot, 65536) if frame == "bgzf" else slot


def cut(source, sizes, start):
    """the batches' bytes: consecutive pieces of the source, wrapping round"""
    out, pos = [], start % len(source)
    for n in sizes:
        if pos + n > len(source):
            pos = 0
        out.append(source[pos:pos + n])
        pos += n
    return out


# ---- drivers: one call of the C ABI per method, the model beside it ---------------------------------------------------


class Enc:
    def __init__(self, pkg, level, frame, B, P, depth, on=None):
        self.L, self.cap = pkg.lib(), B * P
        if on is None:
            self.p = self.L.hipdeflate_pipe_open(level, frame_id(pkg, frame), B, P, depth)
        else:
            self.p = self.L.hipdeflate_pipe_open_on(on, level, frame_id(pkg, frame), B, P, depth)
        assert self.p, "hipdeflate_pipe_open failed"
        self.model = pm.Slots(depth)

    def input(self):
        cap = ctypes.c_size_t()
        buf = self.L.hipdeflate_pipe_input(self.p, ctypes.byref(cap))
        assert not buf or cap.value == self.cap
        return buf

    def feed(self, data):
        """input + submit from the one thread that also fetches: only where the slot rule allows it"""
        assert self.model.can_input(), "the test itself would block here"
        self.model.input()
        self.feed_unchecked(data)
        assert self.model.submit() == 0

    def feed_unchecked(self, data):
        buf = self.input()
        assert buf
        if data:
            ctypes.memmove(buf, data, len(data))
        assert self.L.hipdeflate_pipe_submit(self.p, len(data)) == 0

    def result_raw(self):
        d, n, nb = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32(0xdead)
        rc = self.L.hipdeflate_pipe_result(self.p, ctypes.byref(d), ctypes.byref(n), ctypes.byref(nb))
        return rc, d, n.value, nb.value

    def result(self):
        want = self.model.result()
        rc, d, n, nb = self.result_raw()
        if want == pm.E_ARG:
            return rc, None, None
        return rc, ctypes.string_at(d, n) if n else b"", nb

    def members(self, nb):
        """-> (rc, out_len, dst_off, crc32) as lists, or None each where the library answers NULL"""
        a, b, c = ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_void_p(1)
        rc = self.L.hipdeflate_pipe_members(self.p, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        if rc:
            return rc, None, None, None

        def arr(ptr, dtype, width):
            return None if not ptr.value else [int(x) for x in np.frombuffer(ctypes.string_at(ptr, width * nb), dtype=dtype)]
        return rc, arr(a, np.uint32, 4), arr(b, np.uint64, 8), arr(c, np.uint32, 4)

    def close(self):
        self.L.hipdeflate_pipe_close(self.p)
        self.p = None


class Dec:
    def __init__(self, pkg, max_members, in_cap, out_cap, depth, on=None):
        self.L, self.in_cap = pkg.lib(), in_cap
        if on is None:
            self.p = self.L.hipdeflate_unpipe_open(max_members, in_cap, out_cap, depth)
        else:
            self.p = self.L.hipdeflate_unpipe_open_on(on, max_members, in_cap, out_cap, depth)
        assert self.p, "hipdeflate_unpipe_open failed"
        self.model = pm.Slots(depth)

    def input(self, buf_bytes):
        assert self.model.can_input(), "the test itself would block here"
        self.model.input()
        cap = ctypes.c_size_t()
        buf = self.L.hipdeflate_unpipe_input(self.p, ctypes.byref(cap))
        assert buf and cap.value == self.in_cap and len(buf_bytes) <= self.in_cap
        if buf_bytes:
            ctypes.memmove(buf, buf_bytes, len(buf_bytes))

    def submit(self, ioff, ilen, osz):
        n = len(ioff)
        a, b, c = np.array(ioff, dtype=np.uint64), np.array(ilen, dtype=np.uint32), np.array(osz, dtype=np.uint32)
        rc = self.L.hipdeflate_unpipe_submit(self.p, a.ctypes.data if n else None, b.ctypes.data if n else None,
                                             c.ctypes.data if n else None, n)
        if rc == 0:
            assert self.model.submit() == 0
        return rc

    def feed(self, batch):
        self.input(batch.buf)
        assert self.submit(batch.ioff, batch.ilen, batch.osz) == 0

    def result(self):
        want = self.model.result()
        d, n = ctypes.c_void_p(), ctypes.c_size_t()
        rc = self.L.hipdeflate_unpipe_result(self.p, ctypes.byref(d), ctypes.byref(n))
        if want == pm.E_ARG:
            return rc, None
        return rc, ctypes.string_at(d, n.value) if n.value else b""

    def close(self):
        self.L.hipdeflate_unpipe_close(self.p)
        self.p = None


# ---- what a result must hold ------------------------------------------------------------------------------------------

_expect_cache = {}


def expect(pkg, level, frame, B, batches, key=None):
    """-> per batch (run, member sizes, offsets, crc32 of each block, the blocks, status of each block): the model's
    block table encoded by pkg.batch_deflate in one call, in the pipe's frame, level and slot"""
    if key is not None and key in _expect_cache:
        return _expect_cache[key]
    table = pm.block_table(B, [len(b) for b in batches])
    blob = b"".join(batches)
    offs, lens, base = [], [], 0
    for b, blocks in zip(batches, table):
        offs += [base + o for o, _ in blocks]
        lens += [ln for _, ln in blocks]
        base += len(b)
    members, crc, st = pkg.batch_deflate(blob, offs, lens, level, frame_id(pkg, frame), slot=slot_of(pkg, level, frame, B)) \
        if offs else ([], [], [])
    out, k = [], 0
    for b, blocks in zip(batches, table):
        ms = members[k:k + len(blocks)]
        run, sizes, doff = pm.expected_run(ms)
        out.append((run, sizes, doff, [zlib.crc32(b[o:o + ln]) for o, ln in blocks], [b[o:o + ln] for o, ln in blocks],
                    [int(x) for x in st[k:k + len(blocks)]]))
        k += len(blocks)
    if key is not None:
        _expect_cache[key] = out
    return out


def parse_sizes(pkg, frame, run, nmembers):
    """the member sizes as a reader finds them in the run itself, and what the members inflate to; None for the
    frame that carries no length (raw, flushed)"""
    if frame == "raw_flush":
        return None, None
    sizes, plain, pos = [], [], 0
    if frame == "bgzf":
        for o, ln, isz in pkg.bgzf_scan(run):                 # the BSIZE walk
            sizes.append(ln + 18)
            plain.append(zlib.decompress(run[o:o + ln - 8], -15))
            assert len(plain[-1]) == isz
        return sizes, plain
    wbits = 15 if frame == "zlib" else 31
    for _ in range(nmembers):
        d = zlib.decompressobj(wbits)
        plain.append(d.decompress(run[pos:]))
        assert d.eof
        sizes.append(len(run) - pos - len(d.unused_data))
        pos += sizes[-1]
    assert pos == len(run)
    return sizes, plain


def check_result(pkg, enc, frame, want, got, what, rng=None):
    """one fetched result and its member table against the expectation"""
    run, sizes, doff, crcs, blocks, _ = want
    rc, data, nb = got
    assert rc == 0, what
    assert nb == len(blocks), (what, "nblocks", nb, len(blocks))
    assert data == run, (what, "run of %d bytes, expected %d" % (len(data), len(run)))
    rc, olen, off, crc = enc.members(nb)
    assert rc == 0, what
    if nb == 0:
        assert olen is None and off is None and crc is None, (what, "an empty batch has no member table")
        return
    assert olen == sizes and off == doff and crc == crcs, what
    psizes, plain = parse_sizes(pkg, frame, data, nb)
    if psizes is not None:
        assert psizes == olen and plain == blocks, what
    if frame == "bgzf" and rng is not None:
        # BAM virtual offsets: (member offset << 16) | offset in the block names the byte that inflating from there yields
        for _ in range(4):
            i = int(rng.integers(0, nb))
            u = int(rng.integers(0, len(blocks[i])))
            v = (off[i] << 16) | (u & 0xffff)
            c, w = v >> 16, v & 0xffff
            bsize = int.from_bytes(data[c + 16:c + 18], "little") + 1
            assert zlib.decompress(data[c + 18:c + bsize - 8], -15)[w] == blocks[i][u], (what, i, u)


def check_twin_sample(pkg, level, frame, B, expected, rng, count=6):
    """a seeded sample of the expected members against the CPU twin directly"""
    flat = [(m_off, n, blk, run) for run, sizes, doff, _, blocks, _ in expected for m_off, n, blk in zip(doff, sizes, blocks)]
    h, t = HEAD_TAIL[frame]
    room = slot_of(pkg, level, frame, B) - h - t
    for k in rng.integers(0, len(flat), count):
        o, n, blk, run = flat[int(k)]
        m = run[o:o + n]
        r, twin = (hdtest.oracle_twin_flush if frame == "raw_flush" else hdtest.oracle_twin)(blk, level, cap=room)
        assert r == 0 and m[h:len(m) - t] == twin, (level, frame, len(blk))


def drive(pkg, enc, frame, batches, expected, ops, what, rng=None):
    sub = got = 0
    for op in ops:
        if op == "S":
            enc.feed(batches[sub])
            sub += 1
        else:
            check_result(pkg, enc, frame, expected[got], enc.result(), what + (got,), rng)
            got += 1
    assert sub == got == len(batches)


# ---- encoder pipe -----------------------------------------------------------------------------------------------------


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("level,frame,B", CONFIGS)
def test_pipe_submit_patterns(pkg, source, level, frame, B, depth):
    """every submit pattern of the model: result k is the concatenation of batch k's expected members, nblocks is
    the model's, a 0-byte batch gives 0 bytes and 0 blocks in its place, the member table is the run's"""
    rng = np.random.default_rng(level * 1000 + B + depth)
    stalls = pkg.lib().hipdeflate_stall_count()
    for k, (name, (p, sizes)) in enumerate(pm.patterns(B, P).items()):
        batches = cut(source, sizes, 77777 * k + 4099 * level)
        expected = expect(pkg, level, frame, B, batches, key=(level, frame, B, name))
        assert not any(any(e[5]) for e in expected)
        if depth == DEPTHS[0]:
            check_twin_sample(pkg, level, frame, B, expected, rng)
        enc = Enc(pkg, level, frame, B, p, depth)
        try:
            drive(pkg, enc, frame, batches, expected, pm.schedule("eager", len(batches), depth), (name, depth), rng)
        finally:
            enc.close()
    assert pkg.lib().hipdeflate_stall_count() == stalls


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("level,frame,B", CONFIGS)
def test_pipe_fetch_orders_do_not_change_the_bytes(pkg, source, level, frame, B, depth):
    """depth - 1 submits ahead, and all `depth` slots filled before the first fetch, drained, filled again: the
    same results in the same order as with one fetch per submit"""
    pats = pm.patterns(B, P)
    for k, name in enumerate(pats):
        p, sizes = pats[name]
        batches = cut(source, sizes, 77777 * k + 4099 * level)
        expected = expect(pkg, level, frame, B, batches, key=(level, frame, B, name))
        for order in ("lagged", "fill_drain"):
            ops = pm.schedule(order, len(batches), depth)
            assert order != "fill_drain" or ops.startswith("S" * depth + "R")
            enc = Enc(pkg, level, frame, B, p, depth)
            try:
                drive(pkg, enc, frame, batches, expected, ops, (name, order, depth))
            finally:
                enc.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", [2, 3])
def test_pipe_large_runs_are_whole_when_result_returns(pkg, source, depth):
    """runs of 16 MiB (256 stored members), read the moment result returns: the copy of the payload to the host is
    the last thing result waits for, and a slot's landing buffer still holds the run of `depth` batches ago"""
    level, frame, B, per = 0, "bgzf", 0xff00, 256
    sizes = [per * B, per * B - 1, per * B, per * B - B + 1, per * B, per * B]
    base = np.frombuffer((source * (per * B // len(source) + 1))[:per * B], dtype=np.uint8)
    batches = [(base[:n] ^ np.uint8(k + 1)).tobytes() for k, n in enumerate(sizes)]      # no two batches share a block
    expected = expect(pkg, level, frame, B, batches)
    for order in ("eager", "fill_drain"):
        enc = Enc(pkg, level, frame, B, per, depth)
        try:
            sub = got = 0
            for op in pm.schedule(order, len(batches), depth):
                if op == "S":
                    enc.feed(batches[sub])
                    sub += 1
                else:
                    rc, data, nb = enc.result()
                    assert rc == 0 and nb == len(expected[got][4]), (order, got)
                    assert data == expected[got][0], (order, got, "the run was not whole when result returned")
                    got += 1
        finally:
            enc.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", [2, 3])
def test_pipe_driven_from_two_threads(pkg, source, depth):
    """one thread does input / submit, one does result, as the header allows: input() waits here and the consumer
    frees it; the bytes are the serial bytes; a result's data stays unchanged until the next result call while the
    producer runs on"""
    level, frame, B = 2, "bgzf", 0xff00
    sizes = pm.pat_random(B, P, seed=depth, n=64)
    batches = cut(source, sizes, 123457)
    expected = expect(pkg, level, frame, B, batches)
    enc = Enc(pkg, level, frame, B, P, depth)
    ready, progressed, errors, results = threading.Semaphore(0), threading.Event(), [], []

    def producer():
        try:
            for b in batches:
                enc.feed_unchecked(b)            # (not the single-threaded rule: this input() may wait)
                ready.release()
                progressed.set()
        except BaseException as e:               # noqa: B036 -- reported by the test's thread
            errors.append(("producer", repr(e)))
            ready.release()

    def consumer():
        try:
            for k in range(len(batches)):
                if not ready.acquire(timeout=JOIN_S) or errors:
                    errors.append(("consumer", "no batch %d to fetch" % k))
                    return
                rc, d, n, nb = enc.result_raw()
                first = ctypes.string_at(d, n) if n else b""
                progressed.clear()
                progressed.wait(0.005)           # let the producer fill and submit the slots that are free
                again = ctypes.string_at(d, n) if n else b""
                results.append((rc, first, again, nb))
        except BaseException as e:               # noqa: B036
            errors.append(("consumer", repr(e)))

    threads = [threading.Thread(target=producer, daemon=True), threading.Thread(target=consumer, daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    alive = [t.is_alive() for t in threads]
    assert not any(alive), ("a thread is still waiting", alive, errors, len(results))
    enc.close()
    assert not errors, errors
    assert len(results) == len(batches)
    for k, (rc, first, again, nb) in enumerate(results):
        assert rc == 0 and nb == len(expected[k][4]), k
        assert first == expected[k][0], (k, "the serial bytes")
        assert again == first, (k, "a held result changed while the producer ran on")


@pytest.mark.timeout(300)
def test_pipe_misuse_is_answered_and_the_pipe_goes_on(pkg, source):
    level, frame, B, depth = 1, "bgzf", 0xff00, 2
    L = pkg.lib()
    enc = Enc(pkg, level, frame, B, 2, depth)
    batches = cut(source, [B + 5, 2 * B, 0, 17, 2 * B - 1, 1], 999)
    expected = expect(pkg, level, frame, B, batches)
    k = 0

    def good_batch():
        nonlocal k
        enc.feed(batches[k])
        check_result(pkg, enc, frame, expected[k], enc.result(), ("after a refusal", k))
        k += 1

    try:
        # nothing pending, nothing held, nothing being filled
        assert enc.result() == (pkg.HD_E_ARG, None, None)
        assert enc.members(0)[0] == pkg.HD_E_ARG
        assert L.hipdeflate_pipe_submit(enc.p, 16) == pkg.HD_E_ARG and enc.model.submit() == pm.E_ARG
        good_batch()
        # a result is held now: the table is there; a result call that finds nothing still gives the slot back
        assert enc.members(len(expected[0][4]))[0] == 0
        assert enc.result() == (pkg.HD_E_ARG, None, None)
        assert enc.members(0)[0] == pkg.HD_E_ARG
        good_batch()
        # input twice, then more bytes than the buffer holds; the batch being filled survives both
        assert enc.model.can_input()
        enc.model.input()
        buf = enc.input()
        assert buf and not enc.model.can_input()
        assert enc.input() is None
        assert L.hipdeflate_pipe_submit(enc.p, enc.cap + 1) == pkg.HD_E_ARG
        ctypes.memmove(buf, batches[k], len(batches[k]))
        assert L.hipdeflate_pipe_submit(enc.p, len(batches[k])) == 0 and enc.model.submit() == 0
        check_result(pkg, enc, frame, expected[k], enc.result(), ("after input twice", k))
        k += 1
        assert L.hipdeflate_pipe_submit(enc.p, 0) == pkg.HD_E_ARG
        while k < len(batches):
            good_batch()
        assert L.hipdeflate_pipe_result(None, None, None, None) == pkg.HD_E_ARG
        assert L.hipdeflate_pipe_members(None, None, None, None) == pkg.HD_E_ARG
    finally:
        enc.close()
    # open: block_bytes a multiple of 16, 2 <= depth <= 16
    fr = frame_id(pkg, frame)
    for bad in ((B + 8, 4, 3), (B - 1, 4, 3), (0, 4, 3), (B, 0, 3), (B, 4, 1), (B, 4, 0), (B, 4, -1), (B, 4, 17)):
        assert not L.hipdeflate_pipe_open(level, fr, bad[0], bad[1], bad[2]), bad
    assert not L.hipdeflate_pipe_open(level, 6, B, 4, 3) and not L.hipdeflate_pipe_open(level, -1, B, 4, 3)
    p16 = L.hipdeflate_pipe_open(level, fr, B, 4, 16)
    assert p16
    L.hipdeflate_pipe_close(p16)
    enc = Enc(pkg, level, frame, B, 2, depth)
    try:
        enc.feed(batches[0])
        check_result(pkg, enc, frame, expected[0], enc.result(), ("after refused opens",))
    finally:
        enc.close()


@pytest.mark.timeout(300)
def test_pipe_block_that_does_not_fit_its_slot(pkg, source):
    """HD_FRAME_BGZF with block_bytes = 65536: the slot is 65536 bytes, and an incompressible block of 65536 bytes
    has no member that small.  result answers 1; a refused block has out_len 0 and adds nothing to the run; the
    other members are where the table says and are batch_deflate's for the same slot; the next batch is clean"""
    level, frame, B, per = 1, "bgzf", 65536, 6
    rnd = np.random.default_rng(2718).integers(0, 256, 3 * B, dtype=np.uint8).tobytes()
    mixed = rnd[:B] + source[:B] + rnd[B:2 * B] + source[B:2 * B] + rnd[2 * B:3 * B] + rnd[:100]
    clean = source[5 * B: 5 * B + 2 * B + 300]
    batches = [clean, mixed, clean, mixed[:B], clean[:7]]
    expected = expect(pkg, level, frame, B, batches)
    assert expected[1][5] == [1, 0, 1, 0, 1, 0] and expected[3][5] == [1] and not any(expected[0][5] + expected[4][5])
    for e in expected:
        assert all((n == 0) == (s != 0) for n, s in zip(e[1], e[5])), "batch_deflate reports a refused block with out_len 0"
    for depth, order in ((2, "eager"), (3, "lagged"), (3, "fill_drain")):
        enc = Enc(pkg, level, frame, B, per, depth)
        try:
            sub = got = 0
            for op in pm.schedule(order, len(batches), depth):
                if op == "S":
                    enc.feed(batches[sub])
                    sub += 1
                    continue
                run, sizes, doff, crcs, blocks, st = expected[got]
                rc, data, nb = enc.result()
                assert rc == (1 if any(st) else 0), (depth, order, got)
                assert nb == len(blocks) and data == run, (depth, order, got, len(data), len(run))
                rc, olen, off, crc = enc.members(nb)
                assert rc == 0 and olen == sizes and off == doff and crc == crcs, (depth, order, got)
                fit = [b for b, s in zip(blocks, st) if not s]
                assert [zlib.decompress(data[o:o + ln - 8], -15) for o, ln, _ in pkg.bgzf_scan(data)] == fit
                got += 1
        finally:
            enc.close()


# ---- decoder pipe -----------------------------------------------------------------------------------------------------

EOF_STREAM = (b"\x03\x00", b"")                 # the payload of BGZF's EOF member: out_size 0


class Batch:
    """A member table laid over an input buffer: members in TABLE order, placed in the buffer in another order, at
    odd offsets, with bytes that belong to nobody between them; in_len of some members takes trailing bytes in"""

    def __init__(self, members, seed, osz=None, physical=None):
        rng = np.random.default_rng(seed)
        n = len(members)
        order = list(rng.permutation(n)) if physical is None else physical
        buf = bytearray(rng.integers(0, 256, 1, dtype=np.uint8).tobytes())      # member 0 of the buffer starts at 1
        self.ioff, self.ilen = [0] * n, [0] * n
        for i in order:
            z = members[i][0]
            if (len(buf) & 1) == 0:
                buf += b"\xee"
            self.ioff[i] = len(buf)
            trail = int(rng.integers(0, 9))
            junk = rng.integers(0, 256, trail + int(rng.integers(0, 5)), dtype=np.uint8).tobytes()
            buf += z + junk
            self.ilen[i] = len(z) + (trail if i % 2 else 0)
        self.end = max([o + ln for o, ln in zip(self.ioff, self.ilen)] + [0])
        self.buf = bytes(buf[:self.end])
        self.osz = [len(m[1]) for m in members] if osz is None else osz
        self.plain = b"".join(m[1] for m in members)
        self.members = members

    def verdict(self):
        """the status hipdeflate_unpipe_result states for this table: the first member's, in table order, that is
        not 0 -- the oracle's status, or 3 where the stream yields fewer bytes than out_size"""
        for o, ln, cap in zip(self.ioff, self.ilen, self.osz):
            r, out = hdtest.oracle_inflate(self.buf[o:o + ln], cap)
            if r:
                return r
            if len(out) != cap:
                return 3
        return 0


@pytest.fixture(scope="module")
def streams(pkg, source):
    """(raw DEFLATE stream, what it inflates to): our own members at levels 1 / 3 / 6 and the reference's encoders'
    full-size streams of tests/golden/ref_streams_full.json"""
    own = []
    sizes = [0xff00, 1, 777, 40000, 65536, 5000, 0xff00, 31, 12345, 0xff00, 2, 60000]
    for level in (1, 3, 6):
        offs, o = [], 1000 * level
        for n in sizes:
            offs.append(o)
            o += n
        members, _, st = pkg.batch_deflate(source, offs, sizes, level, pkg.FRAME_RAW)
        assert not any(st)
        own += [(m, source[a:a + n]) for m, a, n in zip(members, offs, sizes)]
    ref = []
    for s in json.load(open(os.path.join(hdtest.GOLDEN, "ref_streams_full.json"))):
        z = base64.b64decode(s["stream"])
        r, out = hdtest.oracle_inflate(z, s["out_len"])
        assert r == 0 and hdtest.sha(out) == s["out_sha256"]
        ref.append((z, out))
    return own, ref


def drive_dec(dec, batches, ops, what, statuses=None):
    sub = got = 0
    for op in ops:
        if op == "S":
            dec.feed(batches[sub])
            sub += 1
        else:
            rc, data = dec.result()
            want = statuses[got] if statuses else 0
            assert rc == want, (what, "batch", got, "status", rc, "expected", want)
            if want == 0:
                assert data == batches[got].plain, (what, "batch", got, len(data), len(batches[got].plain))
            got += 1
    assert sub == got == len(batches)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", [2, 3])
def test_unpipe_member_tables_the_loop_never_makes(pkg, streams, depth):
    """members at odd offsets with trailing bytes, in an order that is not their order in the buffer; members of
    out_size 0 at the start, the middle and the end; nmembers == max_members; sum(out_size) == out_cap; no members
    at all: the result is the concatenation in table order"""
    own, ref = streams
    max_members = 12
    batches = [
        Batch([], 1),
        Batch([EOF_STREAM] + own[0:4] + [EOF_STREAM] + own[4:7] + [EOF_STREAM], 2),
        Batch(own[12:24], 3),                                            # nmembers == max_members
        Batch(ref[-1:] + ref[0:8], 4),                                   # the 1 MiB member among full blocks
        Batch([EOF_STREAM] * 3, 5),                                      # members, and not a byte of output
        Batch(own[24:36], 6, physical=list(range(11, -1, -1))),          # the buffer holds them back to front
        Batch([], 7),
    ]
    batches += [Batch(ref[k:k + 12], 10 + k) for k in range(8, len(ref) - 1, 12)]
    batches += [Batch(own[7:12], 8), Batch([EOF_STREAM], 9)]
    assert any(len(b.ioff) == max_members for b in batches) and all(len(b.ioff) <= max_members for b in batches)
    assert all(any(o & 1 for o in b.ioff) for b in batches if b.ioff)
    assert any(b.ioff != sorted(b.ioff) for b in batches)
    in_cap, out_cap = max(b.end for b in batches), max(len(b.plain) for b in batches)    # both met exactly by a batch
    for order in pm.FETCH_ORDERS:
        dec = Dec(pkg, max_members, in_cap, out_cap, depth)
        try:
            drive_dec(dec, batches, pm.schedule(order, len(batches), depth), (order, depth))
        finally:
            dec.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("depth", [2, 3])
def test_unpipe_verdicts_are_the_oracles_on_the_batch_that_held_the_member(pkg, streams, depth):
    own, ref = streams
    good = own[0:6]

    def with_sizes(members, delta, seed):
        return Batch(members, seed, osz=[len(m[1]) + delta.get(i, 0) for i, m in enumerate(members)])

    cut_short = (ref[3][0][:len(ref[3][0]) // 2], ref[3][1])             # input runs out inside a block
    flipped = bytearray(own[3][0])
    flipped[0] |= 0x06                                                   # block type 3
    flipped = (bytes(flipped), own[3][1])
    batches = [
        Batch(good, 1),
        with_sizes(own[6:12], {2: +1, 4: -1}, 2),                        # fewer bytes than out_size, then more: 3
        Batch(ref[0:5], 3),
        Batch(own[12:14] + [cut_short] + own[14:16], 4),                 # damaged: 1
        Batch([flipped], 5),
        Batch(own[16:20], 6),
        with_sizes(own[20:24] + [cut_short], {1: -1}, 7),                # several bad members: the first one's, 3
        Batch([cut_short] + own[24:26], 8, osz=[len(cut_short[1]), len(own[24][1]) + 1, len(own[25][1])]),   # ... 1
        Batch(ref[5:9], 9),
    ]
    statuses = [b.verdict() for b in batches]
    assert statuses == [0, 3, 0, 1, 1, 0, 3, 1, 0], statuses
    in_cap, out_cap = max(b.end for b in batches), max(sum(b.osz) for b in batches)
    for order in pm.FETCH_ORDERS:
        dec = Dec(pkg, 8, in_cap, out_cap, depth)
        try:
            drive_dec(dec, batches, pm.schedule(order, len(batches), depth), (order, depth), statuses)
        finally:
            dec.close()


@pytest.mark.timeout(300)
def test_unpipe_refusals_leave_the_batch_to_be_submitted_again(pkg, streams):
    own, _ = streams
    members = own[0:4]
    b = Batch(members, 1)
    in_cap, out_cap = b.end + 10, len(b.plain) + 10
    L = pkg.lib()
    dec = Dec(pkg, 4, in_cap, out_cap, 2)
    try:
        assert dec.result() == (pkg.HD_E_ARG, None)
        assert dec.submit(b.ioff, b.ilen, b.osz) == pkg.HD_E_ARG          # submit without input
        refused = [
            ("nmembers > max_members", b.ioff + [b.ioff[0]], b.ilen + [b.ilen[0]], b.osz + [0]),
            ("sum(out_size) > out_cap", b.ioff, b.ilen, b.osz[:3] + [b.osz[3] + 11]),
            ("a member reaching past in_cap", b.ioff, b.ilen[:2] + [in_cap - b.ioff[2] + 1] + b.ilen[3:], b.osz),
            ("a member of HD_INFLATE_MAX_IN bytes", b.ioff, [HD_INFLATE_MAX_IN] + b.ilen[1:], b.osz),
            ("a member of more than HD_INFLATE_MAX_IN bytes", b.ioff, b.ilen[:3] + [0xffffffff], b.osz),
        ]
        for what, ioff, ilen, osz in refused:
            dec.input(b.buf)
            assert dec.submit(ioff, ilen, osz) == pkg.HD_E_ARG, what
            assert dec.submit(b.ioff, b.ilen, b.osz) == 0, what           # the same input buffer, a valid table
            assert dec.result() == (0, b.plain), what
        assert L.hipdeflate_unpipe_result(None, None, None) == pkg.HD_E_ARG
    finally:
        dec.close()
    for bad in ((0, 64, 64, 2), (4, 0, 64, 2), (4, 64, 0, 2), (4, 64, 64, 1), (4, 64, 64, 17)):
        assert not L.hipdeflate_unpipe_open(*bad), bad
    p16 = L.hipdeflate_unpipe_open(4, 64, 64, 16)
    assert p16
    L.hipdeflate_unpipe_close(p16)


# ---- one context, several users at once ---------------------------------------------------------------------------------


def shared_context_child():
    """Runs in a process of its own (the device list is fixed by the first use): a level-2 pipe, a level-6 pipe, an
    unpipe and a loop of pkg.batch_deflate at level 3, first one after the other, then at once from four threads --
    on one context, then with the pipes spread over the two contexts of the list 0,0."""
    pkg = hdtest.pkg()
    L = pkg.lib()
    assert L.hipdeflate_init_devices((ctypes.c_int * 2)(0, 0), 2) == 0 and L.hipdeflate_device_count() == 2
    source = make_source()
    B, per, depth, nbatch = 0xff00, 4, 3, 32

    def enc_job(level, on):
        def job():
            batches = cut(source, pm.pat_random(B, per, seed=level, n=nbatch), 1000 * level)
            enc, out, sub = Enc(pkg, level, "bgzf", B, per, depth, on), [], 0
            try:
                for op in pm.schedule("lagged", nbatch, depth):
                    if op == "S":
                        enc.feed(batches[sub])
                        sub += 1
                    else:
                        rc, data, nb = enc.result()
                        out.append((rc, data, nb, enc.members(nb)))
            finally:
                enc.close()
            assert pkg.bgzf_decompress_bytes(b"".join(o[1] for o in out) + pkg.BGZF_EOF) == b"".join(batches)
            return out
        return job

    offs = list(range(0, 48 * 40000, 40000))
    raw, _, st = pkg.batch_deflate(source, offs, [40000] * 48, 1, pkg.FRAME_RAW)
    assert not any(st)
    tables = [Batch([(raw[(k + j) % 48], source[offs[(k + j) % 48]:offs[(k + j) % 48] + 40000]) for j in range(6)], k)
              for k in range(nbatch)]

    def dec_job(on):
        def job():
            dec = Dec(pkg, 6, max(t.end for t in tables), 6 * 40000, depth, on)
            out, sub = [], 0
            try:
                for op in pm.schedule("lagged", nbatch, depth):
                    if op == "S":
                        dec.feed(tables[sub])
                        sub += 1
                    else:
                        out.append(dec.result())
            finally:
                dec.close()
            assert out == [(0, t.plain) for t in tables]
            return out
        return job

    boffs = list(range(0, 300 * 10000, 10000))

    def batch_job():
        out = []
        for _ in range(6):
            members, crc, st = pkg.batch_deflate(source, boffs, [10000] * 300, 3, pkg.FRAME_BGZF)
            out.append((members, list(crc), list(st)))
        return out

    for phase, (e2, e6, ed) in (("one context", (None, None, None)), ("the list 0,0", (0, 1, 1))):
        jobs = [enc_job(2, e2), enc_job(6, e6), dec_job(ed), batch_job]
        alone = [j() for j in jobs]
        stalls = L.hipdeflate_stall_count()
        together, errors = [None] * len(jobs), []

        def run(i):
            try:
                together[i] = jobs[i]()
            except BaseException as e:           # noqa: B036
                errors.append((i, repr(e)))
        threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(jobs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_S)
        assert not any(t.is_alive() for t in threads), (phase, "a user is still waiting")
        assert not errors, (phase, errors)
        for i in range(len(jobs)):
            assert together[i] == alone[i], (phase, "user %d: not what the same calls give alone" % i)
        assert L.hipdeflate_stall_count() == stalls, phase
    L.hipdeflate_shutdown()
    print("SHARED-CONTEXT-OK")


@pytest.mark.timeout(300)
def test_one_context_shared_by_two_pipes_an_unpipe_and_batch_calls(pkg):
    """the scan's tile buffer and the dynamic levels' token scratch are one per context: users on different streams
    take turns, and nobody's bytes change for it"""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_pipes as t; t.shared_context_child()" % (
        hdtest.ROOT, os.path.join(hdtest.ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if k != "HIPDEFLATE_DEVICES"}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode == 0 and "SHARED-CONTEXT-OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
