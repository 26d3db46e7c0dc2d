"""Raw, zlib and gzip members at the edge offsets of a 6.06 GiB input and a 6.06 GiB output: the layout, the expected
answers and the checker of test_gpu_far_offsets.py's section D2 (hipdeflate_batch_inflate_size_dev and
hipdeflate_batch_inflate_framed_dev), kept apart from the GPU so that test_far_offsets.py can run the same layout
through a stand-in over far_offsets.Sparse and through its address mutants.  Nothing here calls a kernel.

The framed family has addresses the block families do not: the header at in + in_off, the payload table another kernel
made (p_off = in_off + header), the trailer at in + p_off + bytes consumed, read byte by byte, and in_used = (p_off -
in_off) + consumed + trailer.  So besides far_offsets' placement (one member at a boundary kind of the input whose output
lies at ANOTHER boundary kind of the output, high / low / end rows crossed the other way, shuffled tables, sentinels over
the aliases of the input and around and over the aliases of the output) the members are chosen for where their parts fall:
a name whose NUL lies behind 2^32, an extra field that puts header and payload 64 KiB apart, a gzip member of 104 bytes
from 2^32 - 100 (CRC-32 | ISIZE cut by 2^32) and a zlib member of 102 bytes (the Adler-32 cut 2 | 2)."""
import collections

import numpy as np

import far_offsets as fo
import framed_gen as fg
import framed_model as M
import hdtest

BIG = fo.P32 + (1 << 31) + (64 << 20)
FRAMES = (M.RAW, M.ZLIB, M.GZIP)
FRAME_NAMES = {M.RAW: "raw", M.ZLIB: "zlib", M.GZIP: "gzip"}
# a launch: slot 0 is the boundary member; slots 1.. take these kinds.  The high rows are neighbours in the buffer
# (2 * GUARD + 1 apart), the end rows too: a refused member sits in slot 2 or 6 of its plan, between / beside valid ones.
IN_KINDS = ("high", "high", "high", "low", "end", "end", "low")
OUT_KINDS = ("low", "high", "low", "high", "end", "high", "end")
TAIL = 24                                            # non-zero bytes behind every member, outside its in_len

Case = collections.namedtuple("Case", "name frame data plain room follow")
Placed = collections.namedtuple("Placed", "case a b b2")          # input Row, output Row, the follow-up's output Row


def wrap(frame, stream, plain, **kw):
    if frame == M.RAW:
        return bytes(stream)
    return fg.zlib_member(stream, plain) if frame == M.ZLIB else fg.gzip_member(stream, plain, **kw)


_cases = {}


def cases(frame):
    """name -> Case.  plain: the contents where the member is valid by construction, None where the model must say;
    room: the out_cap that fits exactly (a refused member: what its stream needs, so that the verdict is the header's or
    the trailer's and not "does not fit"); follow: (second member, its contents) where in_used must find one"""
    if frame in _cases:
        return _cases[frame]
    s = hdtest.synth()
    text, fastq = bytes(s.text_like(400000, seed=41)), bytes(s.fastq_like(400000, seed=42))
    noise = bytes(s.random_bytes(70000, seed=43))
    out = {}

    def add(name, data, plain, room=None, follow=None):
        out[name] = Case(name, frame, bytes(data), plain, len(plain) if room is None else room, follow)

    for name, d, level in (("text300k", text[:300000], 6), ("fastq70k", fastq[:70000], 1), ("noise", noise[:66000], 6),
                           ("five", text[5000:5005], 9)):
        add(name, wrap(frame, fg.raw_deflate(d, level), d), d)
    d = fastq[100:100 + 0xff00]
    r, twin = hdtest.oracle_twin(d, 1)
    assert r == 0
    add("twin1", wrap(frame, twin, d), d)
    d = text[7000:12000]
    z = fg.raw_deflate(d, 6)
    base = wrap(frame, z, d, flg=M.FNAME, name=5)
    add("garbage7", base + bytes((i * 37 + 7) & 0xff for i in range(7)), d)
    add("cut1", base[:-1], None, len(d) + 512)         # (the stream loses its last byte: zeros are read past the cut, give them room)
    (m1, d1), (m2, d2) = fg.pairs()[frame]
    add("pair", m1 + m2, d1, follow=(m2, d2))

    def flipped(at, bit):
        m = bytearray(base)
        m[len(m) + at] ^= 1 << bit
        return m
    if frame == M.GZIP:
        add("name300", fg.gzip_member(z, d, flg=M.FNAME, name=300), d)
        add("extra65535", fg.gzip_member(z, d, flg=M.FEXTRA, xlen=65535, k=3), d)
        add("all_fields", fg.gzip_member(z, d, flg=M.FHCRC | M.FCOMMENT | M.FNAME, name=65, comment=63, k=5), d)
        d40 = noise[300:340]
        add("g104", fg.gzip_member(fo.stored_payload(d40), d40, flg=M.FNAME, name=40), d40)
        assert len(out["g104"].data) == 104
        add("crc_flip", flipped(-7, 2), None, len(d))
        add("isize_flip", flipped(-3, 5), None, len(d))
        add("bad_id", fg.gzip_member(z, d, id1=0x1e), None, len(d))
        add("reserved", fg.gzip_member(z, d, flg=0x40), None, len(d))
        add("no_nul", fg.gzip_header(flg=M.FNAME, name=40, nul=False) + fg._text(9, 30), None, 512)
    elif frame == M.ZLIB:
        d91 = noise[500:591]
        add("z102", fg.zlib_member(fo.stored_payload(d91), d91), d91)
        assert len(out["z102"].data) == 102
        add("adler_flip", flipped(-2, 3), None, len(d))
        add("bad_fcheck", fg.zlib_member(z, d, fcheck_off=1), None, len(d))
    _cases[frame] = out
    return out


PLANS = {
    M.GZIP: [("ends_at", ["extra65535", "fastq70k", "crc_flip", "five", "text300k", "twin1", "isize_flip", "noise"]),
             ("straddle", ["name300", "noise", "bad_id", "twin1", "fastq70k", "garbage7", "reserved", "five"]),
             ("starts_at", ["all_fields", "five", "no_nul", "text300k", "twin1", "pair", "cut1", "fastq70k"]),
             ("plus1", ["fastq70k", "garbage7", "crc_flip", "noise", "five", "all_fields", "no_nul", "twin1"]),
             ("straddle", ["g104", "twin1", "five", "name300"])],          # the low-offset control launch of the trailer cut
    M.ZLIB: [("ends_at", ["fastq70k", "noise", "adler_flip", "five", "text300k", "twin1", "cut1", "garbage7"]),
             ("straddle", ["z102", "five", "bad_fcheck", "twin1", "fastq70k", "noise", "adler_flip", "text300k"]),
             ("starts_at", ["twin1", "fastq70k", "cut1", "five", "noise", "pair", "bad_fcheck", "garbage7"]),
             ("plus1", ["noise", "text300k", "adler_flip", "garbage7", "five", "fastq70k", "cut1", "twin1"])],
    M.RAW: [("ends_at", ["fastq70k", "noise", "cut1", "five", "text300k", "twin1", "garbage7", "pair"]),
            ("straddle", ["text300k", "five", "cut1", "twin1", "fastq70k", "noise", "garbage7", "pair"]),
            ("starts_at", ["twin1", "fastq70k", "cut1", "five", "noise", "pair", "garbage7", "text300k"]),
            ("plus1", ["noise", "text300k", "cut1", "garbage7", "five", "fastq70k", "pair", "twin1"])],
}
CONTROL_KINDS = ("low", "low", "low")                # the control launch: nothing far but the member that straddles


def launches(frame):
    """-> [[Placed]] in the order of the tables (shuffled, the same at every call)"""
    c = cases(frame)
    out = []
    for r, (kind, names) in enumerate(PLANS[frame]):
        control = len(names) < 8
        kin = [kind] + list(CONTROL_KINDS if control else IN_KINDS)[:len(names) - 1]
        kout = [fo.BOUNDARY[(fo.BOUNDARY.index(kind) + 1 + control) % 4]] + list(CONTROL_KINDS if control else OUT_KINDS)[:len(names) - 1]
        ms = [c[n] for n in names]
        follow = [m for m in ms if m.follow]
        rin = fo.place(BIG, [(k, len(m.data) + TAIL) for k, m in zip(kin, ms)])
        rout = fo.place(BIG, [(k, m.room) for k, m in zip(kout, ms)] + [("high", len(m.follow[1])) for m in follow])
        extra = dict(zip((m.name for m in follow), rout[len(ms):]))
        # (the boundary member itself ends at / straddles the limit: the tail is placed behind it, not counted in)
        a0 = fo.Row(0, fo.edge_offset(kind, len(ms[0].data), BIG), len(ms[0].data), kind)
        rows = [Placed(m, (a0 if i == 0 else a)._replace(length=len(m.data)), b, extra.get(m.name))
                for i, (m, a, b) in enumerate(zip(ms, rin, rout))]
        order = np.random.default_rng(100 * frame + r).permutation(len(rows))
        out.append([rows[i] for i in order])
    return out


def boundary_position(launch):
    return next(i for i, p in enumerate(launch) if p.a.kind in fo.BOUNDARY)


_memo = {}


def want_size(case):
    k = (case.name, case.frame)
    if k not in _memo:
        _memo[k] = M.size(case.data, case.frame)
    return _memo[k]


def want_framed(case, cap):
    k = (case.name, case.frame, cap)
    if k not in _memo:
        _memo[k] = M.framed(case.data, case.frame, cap)
        if _memo[k][0] == 0 and case.plain is not None:
            assert _memo[k][4] == case.plain, case.name
    return _memo[k]


def caps_of(launch, short=None):
    """the rooms; short: the position whose out_cap is one below what its member needs"""
    return [p.case.room - (1 if i == short else 0) for i, p in enumerate(launch)]


def input_regions(launch):
    """the aliases of the far members in the input: filled with the sentinel, so that a header or a trailer read through
    a narrowed address finds neither"""
    return fo.regions([p.a for p in launch], BIG, ends=False)


def output_regions(launch, caps):
    return fo.regions([(p.b.offset, cap) for p, cap in zip(launch, caps)] + [(p.b2.offset, p.b2.length) for p in launch if p.b2], BIG)


def lay_input(src, launch, write=None):
    """fill the alias regions, then the members and the non-zero bytes behind each -> the regions"""
    write = write or (lambda mem, at, data: mem.__setitem__(slice(at, at + len(data)), np.frombuffer(bytes(data), dtype=np.uint8)))
    regs = input_regions(launch)
    fo.fill(src, regs)
    rng = np.random.default_rng(len(launch))
    for p in launch:
        write(src, p.a.offset, p.case.data + rng.integers(1, 256, TAIL, dtype=np.uint8).tobytes())
    return regs


def lay_output(out, launch, caps):
    """sentinels around every far room and over its aliases, zeros in the rooms -> the regions"""
    regs = output_regions(launch, caps)
    fo.fill(out, regs)
    for p, cap in zip(launch, caps):                  # (no stale bytes of an earlier launch where this one must write)
        out[p.b.offset:p.b.offset + cap] = 0
        if p.b2:
            out[p.b2.offset:p.b2.offset + p.b2.length] = 0
    return regs


def size_problems(launch, got):
    """got[i] = (status, out_size, in_used) of the size pass -> [problem]"""
    return [("size", p.case.name, p.a.kind, tuple(g), want_size(p.case)) for p, g in zip(launch, got) if tuple(g) != want_size(p.case)]


def framed_problems(launch, caps, got, out, regs, src, in_regs):
    """got[i] = (status, out_len, in_used, check) of the framed call, in_used / check None where the call did not ask
    -> [problem]: the four numbers, the bytes of every decoded member, every guard and alias of the output, the aliases of
    the input"""
    bad, rows = [], []
    for p, cap, g in zip(launch, caps, got):
        w = want_framed(p.case, cap)
        if tuple(w[k] if g[k] is None else g[k] for k in range(4)) != w[:4]:
            bad.append(("framed", p.case.name, p.a.kind, p.b.kind, tuple(g), w[:4]))
        elif w[0] == 0:
            rows.append((p.b.offset, w[4]))
    bad += fo.check_rows(out, rows, regs)
    if not fo.intact(in_regs, src):
        bad.append(("input alias",))
    return bad


def honest(all_launches):
    """the conditions that keep the layout a far-offset test (asserted by both halves)"""
    ps = [p for launch in all_launches for p in launch]
    assert sum(p.a.offset >= fo.P32 for p in ps) >= 10 and sum(p.b.offset >= fo.P32 for p in ps) >= 10
    assert any(p.case.plain is not None and len(p.case.plain) > 65536 and p.b.offset >= fo.P32 for p in ps)
    assert {p.a.kind for p in ps} >= set(fo.EDGES) and {p.b.kind for p in ps} >= set(fo.EDGES)
    assert all(p.a.kind != p.b.kind for p in ps if p.a.kind in fo.BOUNDARY)
    return sum(1 for p in ps if p.a.offset >= fo.P32 and want_framed(p.case, p.case.room)[0] != 0)
