"""The files that tests/test_member_any_model.py pins on the model and tests/test_gpu_member_any.py runs on the device: each
builder returns a Case -- the blob, the arguments of the call, and what the contract says the walk answers.  Payloads are
text or bytes in 32..126, which hold no 1f 8b: a candidate is only where a case plants one, and every case states how
many it expects."""
import struct
import zlib

import numpy as np

import framed_model
import hdtest
import member_any_model as am
import member_index_model as mim

FHCRC, FEXTRA, FNAME, FCOMMENT = framed_model.FHCRC, framed_model.FEXTRA, framed_model.FNAME, framed_model.FCOMMENT


class Case:
    def __init__(self, blob, status=0, nmembers=None, ncandidates=None, nsized=None, end=None, first_offset=0, max_member_in=0,
                 nbytes=None):
        self.blob, self.first_offset, self.max_member_in = bytes(blob), first_offset, max_member_in
        self.nbytes = len(self.blob) if nbytes is None else nbytes
        self.want = {"status": status, "nmembers": nmembers, "ncandidates": ncandidates, "nsized": nsized, "end_offset": end}

    def model(self, cap=None):
        """-> (rows, summary) of the model on a table of cap entries (default: enough)"""
        cap = len(am.walk(self.blob, self.first_offset, self.max_member_in, self.nbytes)[0]) + 3 if cap is None else cap
        return am.summary(self.blob, cap, self.first_offset, self.max_member_in, self.nbytes)

    def check_model(self):
        """the model answers what the case states -> (rows, summary)"""
        rows, s = self.model()
        for k, v in self.want.items():
            assert v is None or s[k] == v, (k, s[k], v)
        return rows, s


_CORPUS = []


def text(n, seed=0):
    """n bytes of text from one corpus (made once: the generator costs a second a call), at a place the seed picks"""
    if not _CORPUS:
        _CORPUS.append(bytes(hdtest.synth().text_like(1 << 20, seed=9)))
    at = (seed * 7919) % ((1 << 20) - n + 1)
    return _CORPUS[0][at:at + n]


def printable(n, seed=0):
    return bytes(np.random.default_rng(seed).integers(32, 127, n, dtype=np.uint8))


def small(i, seed=0, **kw):
    """plain member number i of a file: 20..400 bytes of text"""
    n = 20 + (i * 37 + seed * 11) % 381
    return am.plain_member(text(n, seed=seed * 1000 + i), **kw)


def starts(parts):
    return [sum(len(p) for p in parts[:i]) for i in range(len(parts) + 1)]


def gunzip_all(blob):
    """the loop over zlib.decompressobj(31) and unused_data -> (contents, member boundaries)"""
    out, cuts, rest = [], [0], bytes(blob)
    while rest:
        z = zlib.decompressobj(31)
        out.append(z.decompress(rest))
        assert z.eof
        rest = z.unused_data
        cuts.append(len(blob) - len(rest))
    return b"".join(out), cuts


# ---- 1. member counts ----

COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 5000)


def counts(n):
    blob = b"".join(small(i, seed=n) for i in range(n))
    return Case(blob, 0, n, n, n, len(blob))


def empty_members(n=300):
    m = am.plain_member(b"")
    assert len(m) == 20
    return Case(m * n, 0, n, n, n, 20 * n)


# ---- 2. headers ----

HEADERS = {
    "fname_1": dict(flg=FNAME, fname=b"a"), "fname_63": dict(flg=FNAME, fname=b"n" * 63), "fname_64": dict(flg=FNAME, fname=b"n" * 64),
    "fname_65": dict(flg=FNAME, fname=b"n" * 65), "fname_5000": dict(flg=FNAME, fname=b"n" * 5000),
    "fcomment": dict(flg=FCOMMENT, fcomment=b"a comment of some length"), "fhcrc": dict(flg=FHCRC),
    "extra_0": dict(flg=FEXTRA, extra=b""), "extra_4": dict(flg=FEXTRA, extra=b"Ap\x00\x00"),
    "extra_6_not_bc": dict(flg=FEXTRA, extra=b"BD\x02\x00\x20\x00"), "extra_300": dict(flg=FEXTRA, extra=b"Zz\x28\x01" + b"x" * 296),
    "all_four": dict(flg=FEXTRA | FNAME | FCOMMENT | FHCRC, extra=b"Ap\x01\x00q", fname=b"file.txt", fcomment=b"made by a test"),
}


def header(name):
    parts = [small(0, seed=5), am.plain_member(text(300, seed=6), **HEADERS[name]), small(2, seed=5)]
    blob = b"".join(parts)
    return Case(blob, 0, 3, 3, 3, len(blob))


# ---- 3. ending bits ----

def ending_bits(kind):
    """members whose final block ends on each of the eight bit positions of a byte (a stored block ends on a byte)"""
    if kind == "stored":
        parts = [am.plain_member(printable(n, seed=n), level=0) for n in (1, 100, 70000)]
        return Case(b"".join(parts), 0, 3, 3, 3)
    strategy, btype = (zlib.Z_FIXED, 1) if kind == "static" else (zlib.Z_DEFAULT_STRATEGY, 2)
    found = {}
    for n in range(400, 700):
        m = am.plain_member(text(n, seed=n), strategy=strategy)
        stream = m[10:-8]
        if (stream[0] >> 1) & 3 != btype:
            continue
        r, _, bits = framed_model.oracle_inflate_bits(stream, n)
        assert r == 0 and (bits + 7) // 8 == len(stream)
        found.setdefault(bits % 8, m)
        if len(found) == 8:
            break
    assert sorted(found) == list(range(8)), sorted(found)
    parts = [found[k] for k in range(8)]
    return Case(b"".join(parts), 0, 8, 8, 8)


# ---- 4. alignment ----

def aligned_parts(n):
    """member k starts at offset k mod 16: the FNAME of the member in front of it is as long as that takes"""
    parts, o = [], 0
    for k in range(n):
        body = text(50 + 7 * k, seed=k)
        for ln in range(1, 17):
            m = am.plain_member(body, flg=FNAME, fname=b"n" * ln)
            if (o + len(m)) % 16 == (k + 1) % 16:
                break
        parts.append(m)
        o += len(m)
    assert all(s % 16 == k % 16 for k, s in enumerate(starts(parts)[:-1]))
    return parts


def every_alignment():
    return Case(b"".join(aligned_parts(33)), 0, 33, 33, 33)


def stored_of_length(total, seed):
    """a level-0 plain member of exactly `total` bytes"""
    n = total - 18 - 5
    for _ in range(8):
        m = am.plain_member(printable(n, seed=seed), level=0)
        if len(m) == total:
            return m
        n -= len(m) - total
    raise AssertionError(total)


BOUNDARIES = (1024, 65536, 262144, 524288)
STRADDLES = (0, 1, 2, 3, 4, 15, 16, 17)


def straddle(boundary, k):
    """the second member starts at boundary - k"""
    parts = [stored_of_length(boundary - k, seed=boundary + k), small(1, seed=k), small(2, seed=k)]
    return Case(b"".join(parts), 0, 3, 3, 3)


# ---- 5. decoys ----

def decoy(depth):
    """a whole valid file of three members inside the stored payload of a level-0 member, `depth` deep, between two members"""
    inner, n = b"".join(small(i, seed=50) for i in range(3)), 3
    for d in range(depth):
        inner = small(0, seed=51 + d) + am.plain_member(inner, level=0) + small(2, seed=51 + d)
        n += 3
    return Case(inner, 0, 3, n, n, len(inner))


def decoy_joins_chain():
    """a decoy D in the stored payload of R1 whose own stored block runs over the rest of R1 and over R2 up to R2's trailer, which
    serves as its own: D ends where R3 starts"""
    p2 = text(3000, seed=60)
    r2, r3 = am.plain_member(p2), small(3, seed=60)
    rest = len(p2) - len(r2)
    assert rest >= 0
    d = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3, 1]) + struct.pack("<HH", len(p2), len(p2) ^ 0xffff)
    r1 = am.plain_member(b"before the decoy " + d + printable(rest, seed=61), level=0)
    blob = r1 + r2 + r3
    at = blob.index(d)
    cls, hdr, total, size = am.member(blob, at, len(blob))
    assert (cls, hdr, at + total, size) == (am.OK, 10, len(r1) + len(r2), len(p2))
    return Case(blob, 0, 3, 4, 4, len(blob))


def decoy_magics(n=4096):
    parts = [small(0, seed=70), am.plain_member(b"\x1f\x8b\x08\x00" * n, level=0), small(2, seed=70)]
    return Case(b"".join(parts), 0, 3, n + 3, n + 3)


# ---- 6. mixed kinds ----

def coded(kind, chunk):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return mim.gz_member(kind, c.compress(chunk) + c.flush(), zlib.crc32(chunk), len(chunk))


def mixed(n=40):
    kinds = ["BC", None, "MZ", "MG", None, "IG1", "IG2", None]
    parts = []
    for i in range(n):
        k = kinds[i % len(kinds)]
        parts.append(small(i, seed=80) if k is None else coded(k, text(100 + 13 * i, seed=i)))
    plain = sum(1 for i in range(n) if kinds[i % len(kinds)] is None)
    return Case(b"".join(parts), 0, n, n, plain)


def pure_bgzf(n=2048):
    src = text(64, seed=81)
    blob = b"".join(coded("BC", src[i % 20:i % 20 + 1 + (i * 7) % 40]) for i in range(n - 1)) + hdtest.pkg().BGZF_EOF
    return Case(blob, 0, n, n, 0)


# ---- 7. cuts and corruption ----

def three(last=None):
    last = am.plain_member(text(2000, seed=90), flg=FNAME | FHCRC, fname=b"last") if last is None else last
    return [small(0, seed=91), small(1, seed=91), last]


def cuts():
    """every cut inside the last member's header and trailer, and 16 inside its stream: [(nbytes, Case)]"""
    parts = three()
    blob, at, n = b"".join(parts), len(parts[0]) + len(parts[1]), len(parts[2])
    hdr = 10 + 5 + 2
    inside = list(range(1, hdr + 1)) + [hdr + 1 + (n - 8 - hdr - 2) * k // 15 for k in range(16)] + list(range(n - 8, n))
    return [(at + c, Case(blob, 2, 2, end=at, nbytes=at + c)) for c in inside]


def corrupt(kind):
    parts = three()
    at = len(parts[0]) + len(parts[1])
    if kind == "isize":
        parts[1] = parts[1][:-4] + struct.pack("<I", struct.unpack("<I", parts[1][-4:])[0] ^ 1)
        return Case(b"".join(parts), 1, 1, end=len(parts[0]))
    if kind == "crc":
        parts[1] = parts[1][:-8] + struct.pack("<I", struct.unpack("<I", parts[1][-8:-4])[0] ^ 0x8000) + parts[1][-4:]
        return Case(b"".join(parts), 0, 3)
    if kind == "reserved_btype":
        parts[2] = parts[2][:17] + bytes([parts[2][17] | 7]) + parts[2][18:]
        return Case(b"".join(parts), 1, 2, end=at)
    if kind == "nlen_then_cut":
        data = printable(200000, seed=92)                              # four stored blocks of 65535 bytes at the most, by hand
        blocks = [data[o:o + 65535] for o in range(0, len(data), 65535)]
        stream = b"".join(bytes([i == len(blocks) - 1]) + struct.pack("<HH", len(b), len(b) ^ 0xffff) + b for i, b in enumerate(blocks))
        m = bytearray(am.plain_member(b"")[:10] + stream + struct.pack("<II", zlib.crc32(data), len(data)))
        assert gunzip_all(bytes(m))[0] == data
        second, third = 10 + 5 + 65535, 10 + 2 * (5 + 65535)
        m[second + 3] ^= 0x10
        parts[2] = bytes(m)
        return Case(b"".join(parts), 1, 2, end=at, nbytes=at + third + 5 + 1000)
    if kind == "garbage":
        return Case(b"".join(parts) + b"garbage!", 1, 3, end=sum(map(len, parts)))
    assert kind in (1, 2, 3)
    return Case(b"".join(parts) + b"\x1f\x8b\x08"[:kind], 2, 3, end=sum(map(len, parts)))


CORRUPT = ("isize", "crc", "reserved_btype", "nlen_then_cut", "garbage", 1, 2, 3)


# ---- 8. max_member_in ----

def bounded(kind):
    big = am.plain_member(text(20000, seed=100))
    t = len(big)
    assert t > 1000
    if kind == "exact":
        parts = [small(0, seed=101), big, small(2, seed=101)]
        return Case(b"".join(parts), 0, 3, max_member_in=t)
    if kind == "one_longer":
        parts = [small(0, seed=101), big, small(2, seed=101)]
        return Case(b"".join(parts), 4, 1, end=len(parts[0]), max_member_in=t - 1)
    if kind == "last_bound_past_end":
        parts = [small(0, seed=101), big]
        return Case(b"".join(parts), 0, 2, max_member_in=t + 100)
    if kind == "last_cut_by_end":                        # the window ends at nbytes, the bound lies behind it: CUT, not TOO LONG
        parts = [small(0, seed=101), big]
        return Case(b"".join(parts), 2, 1, end=len(parts[0]), max_member_in=t, nbytes=len(parts[0]) + t - 1)
    assert kind == "bgzf_longer"
    parts = [small(0, seed=101), coded("BC", text(20000, seed=102)), small(2, seed=101)]
    assert len(parts[1]) > 1000 and max(len(parts[0]), len(parts[2])) < 1000
    return Case(b"".join(parts), 0, 3, nsized=2, max_member_in=1000)


BOUNDED = ("exact", "one_longer", "last_bound_past_end", "last_cut_by_end", "bgzf_longer")


# ---- 9. first_offset ----

def resumes():
    """[(k, Case)]: the walk resumed behind member k - 1 of a file of 40, at aligned and unaligned starts; then the edges"""
    parts = aligned_parts(40)
    blob, at = b"".join(parts), starts(parts)
    ks = [16, 32, 1, 2, 7, 15, 17, 39]
    out = [(k, Case(blob, 0, 40 - k, 40 - k, 40 - k, len(blob), first_offset=at[k])) for k in ks]
    out.append(("end", Case(blob, 0, 0, 0, 0, len(blob), first_offset=len(blob))))
    out.append(("inside", Case(blob, 1, 0, end=at[3] + 1, first_offset=at[3] + 1)))
    return out
