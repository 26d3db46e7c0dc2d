"""Hand-built raw-DEFLATE streams with a known answer, aimed at the structural edges of the two inflate
kernels (hd_inflate.hpp, hd_inflate_lat.hpp).  Plain Python and numpy; nothing here shares code with
oracle/hd_inflate.c or the kernels.

A stream is described as a list of blocks (`Block`): stored, static or dynamic (with explicit or derived code
lengths and a chosen run-length coding of them), each holding a token list -- a literal is an int 0..255, a
match is (length, distance) or (length, distance, litlen symbol, offset symbol) to force a symbol.  `encode()`
packs the blocks LSB-first; `expand()` computes the output from the token lists byte by byte; that output and
the verdict each family states are the expected answers.

`corpus()` returns the named families as `Case`s, seeded and deterministic (a few seconds of CPU).  Every case
says which verdict the plain and the flushed entry points must give, whether zlib can be asked about it (the
libdeflate-only forms: litlen 286/287, offset 30/31, HLIT > 286, HDIST > 30), and what edges it reaches
(`stats`, counted from the token lists and code lengths as they are written).

Two corpora, one per kernel geometry: `corpus()` aims at the throughput kernel's 2 KiB ring (k_inflate: RING,
PIECE, NEAR below), `lat_corpus()` at the latency kernel's 64 KiB ring and its record queues (k_inflate_lat:
LAT_RING, LAT_FQ, LAT_PQ below).
"""
import collections

import numpy as np

OK, BAD_DATA, INSUFFICIENT_SPACE = 0, 1, 3       # include/hipdeflate_params.h

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258, 258, 258]                  # symbols 257..287 (286, 287: libdeflate decodes them as 258)
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577, 24577, 24577]   # 30, 31: libdeflate decodes them as 24577 + 13 bits
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 13, 13]
PRECODE_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STATIC_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
STATIC_DIST = [5] * 32

# the kernels' geometry the families aim at (hd_inflate.hpp)
RING = 2048                 # INF_RING: the throughput kernel's LDS output ring
PIECE = 1024                # HD_PIECE: output leaves the ring in 1 KiB pieces
NEAR = RING - 258 - 64      # INF_NEAR = 1726: a source at most this far back is read from the ring

# the latency kernel's geometry (hd_inflate_lat.hpp), what lat_corpus() aims at
LAT_RING = 65536            # INF_RING_LAT: its LDS output ring, twice the DEFLATE window
LAT_FQ = LAT_PQ = 4         # INF_FQ, INF_PQ: records in flight front -> sort and sort -> back
LAT_WIN = 704               # WIN_OUT_BUDGET: output bytes of one window record at the most
LAT_MAX_OUT = 1 << 20       # the largest room a call may state and still be decoded by that kernel (hd_api.hip)


def len_sym(length):
    """canonical litlen symbol for a match length (258 -> 285)"""
    if length == 258:
        return 285
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s


def dist_sym(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """RFC 1951 3.2.2: codes from lengths (entries with length 0 get None)"""
    bl = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for b in range(1, 16):
        code = (code + bl.get(b - 1, 0)) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft_used(lens, maxlen=15):
    return sum(1 << (maxlen - l) for l in lens if l)


def fill_lengths(fixed, pool, nsyms, maxlen=15):
    """lengths for `nsyms` symbols: `fixed` {symbol: length} as given, every symbol of `pool` (in order) a length
    such that the code is complete.  The room left is cut into the codewords its binary digits make, the
    shortest of them split in two until there is one per pool symbol."""
    lens = [0] * nsyms
    for s, l in fixed.items():
        lens[s] = l
    room = (1 << maxlen) - kraft_used(lens, maxlen)
    assert room >= 0
    parts = sorted(maxlen - k for k in range(maxlen + 1) if room >> k & 1)
    pool = [s for s in pool if s not in fixed]
    assert len(parts) <= len(pool) or not parts, "not enough symbols to complete the code"
    while len(parts) < len(pool):
        i = min(range(len(parts)), key=lambda j: parts[j])
        assert parts[i] < maxlen, "too many symbols for the room"
        l = parts.pop(i)
        parts += [l + 1, l + 1]
        parts.sort()
    for s, l in zip(pool, parts):
        lens[s] = l
    return lens


def auto_lengths(freq, nsyms, maxlen=15):
    """a complete code over the symbols with freq > 0 (frequent ones shorter); one symbol: the allowed single
    length-1 codeword; none: the empty code"""
    used = sorted((s for s in range(nsyms) if freq.get(s)), key=lambda s: (-freq[s], s))
    lens = [0] * nsyms
    if len(used) == 1:
        lens[used[0]] = 1
    elif used:
        lens = fill_lengths({}, used, nsyms, maxlen)
    return lens


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, n):
        self.bits(rev(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.buf += b

    def pos(self):
        return 8 * len(self.buf) + self.n

    def value(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


class Block:
    """kind: 'stored' | 'static' | 'dynamic' | 'btype3'.  For dynamic blocks lit_lens / dist_lens (None: derived
    from the tokens), hlit / hdist (None: as few as the lengths need), rle 'zlib' (runs over the litlen and offset
    lengths as one sequence: a run may cross the boundary) | 'split' (no run crosses it) | 'plain' (no 16/17/18),
    hclen (None: as few as needed), items (the code-length items as given, for faults).  Stored blocks: data,
    and for faults nlen / length (what the header says)."""

    def __init__(self, kind, tokens=None, data=b"", final=False, **kw):
        self.kind, self.tokens, self.data, self.final = kind, list(tokens or []), bytes(data), final
        self.lit_lens = kw.pop("lit_lens", None)
        self.dist_lens = kw.pop("dist_lens", None)
        self.hlit = kw.pop("hlit", None)
        self.hdist = kw.pop("hdist", None)
        self.rle = kw.pop("rle", "zlib")
        self.hclen = kw.pop("hclen", None)
        self.items = kw.pop("items", None)
        self.pre_lens = kw.pop("pre_lens", None)
        self.nlen = kw.pop("nlen", None)
        self.length = kw.pop("length", None)
        assert not kw, kw


def tok_syms(t):
    """(litlen symbol, length, offset symbol, distance) of a match token"""
    if len(t) == 4:
        return t[2], t[0], t[3], t[1]
    return len_sym(t[0]), t[0], dist_sym(t[1]), t[1]


def _rle(seq, mode):
    """code-length items (symbol, extra bit count, extra value, run start, run length)"""
    items, i = [], 0
    while i < len(seq):
        v = seq[i]
        if mode == "plain":
            items.append((v, 0, 0, i, 1))
            i += 1
            continue
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                items.append((18, 7, k - 11, i, k))
                i, r = i + k, r - k
            while r >= 3:
                k = min(r, 10)
                items.append((17, 3, k - 3, i, k))
                i, r = i + k, r - k
        else:
            items.append((v, 0, 0, i, 1))
            i, r = i + 1, r - 1
            while r >= 3:
                k = min(r, 6)
                items.append((16, 2, k - 3, i, k))
                i, r = i + k, r - k
        for _ in range(r):
            items.append((v, 0, 0, i, 1))
            i += 1
    return items


def block_codes(b):
    """(litlen lengths, offset lengths) a Huffman block is written with"""
    if b.kind == "static":
        return STATIC_LIT, STATIC_DIST
    lit, dist = b.lit_lens, b.dist_lens
    if lit is None or dist is None:
        lf, df = collections.Counter({256: 1}), collections.Counter()
        for t in b.tokens:
            if isinstance(t, int):
                lf[t] += 1
            else:
                ls, _, ds, _ = tok_syms(t)
                lf[ls] += 1
                df[ds] += 1
        lit = auto_lengths(lf, 286) if lit is None else lit
        dist = auto_lengths(df, 30) if dist is None else dist
    return lit, dist


def encode(blocks, chunk=False, stats=None):
    """-> the stream.  chunk: every block non-final and the 00 00 ff ff marker behind them (the full-flush form
    of the 7dictzip / 7razf chunks).  stats (a Counter) gets what the stream reaches."""
    st = stats if stats is not None else collections.Counter()
    w = BitWriter()
    out = 0
    for bi, b in enumerate(blocks):
        final = b.final and not chunk
        w.bits(int(final), 1)
        if b.kind == "btype3":
            w.bits(3, 2)
            continue
        if b.kind == "stored":
            w.bits(0, 2)
            st["stored_align_%d" % ((w.pos() - 3) & 7)] += 1
            w.align()
            ln = len(b.data) if b.length is None else b.length
            nl = (~ln & 0xffff) if b.nlen is None else b.nlen
            w.raw(bytes([ln & 255, ln >> 8, nl & 255, nl >> 8]))
            w.raw(b.data)
            st["stored_empty" if not b.data else "stored_blocks"] += 1
            if len(b.data) == 65535:
                st["stored_65535"] += 1
            out += len(b.data)
            continue
        lit, dist = block_codes(b)
        if b.kind == "static":
            w.bits(1, 2)
        else:
            w.bits(2, 2)
            _write_dynamic_header(w, b, lit, dist, st)
        lc, dc = canonical(lit), canonical(dist)
        for t in b.tokens:
            if isinstance(t, int):
                assert lit[t], "literal %d has no codeword" % t
                w.huff(lc[t], lit[t])
                out += 1
                if lit[t] > 9:
                    st["lit_code_gt9"] += 1
                continue
            ls, length, ds, d = tok_syms(t)
            assert lit[ls] and (dist[ds] or kraft_used(dist) == 0), (ls, ds)
            w.huff(lc[ls], lit[ls])
            eb = LEN_EXTRA[ls - 257]
            w.bits(length - LEN_BASE[ls - 257], eb)
            if dist[ds]:
                w.huff(dc[ds], dist[ds])
            else:
                w.bits(0, 1)                      # the empty offset code: one bit, decoded as symbol 0
            w.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
            if lit[ls] > 9:
                st["lit_code_gt9"] += 1
            if dist[ds] > 8:
                st["dist_code_gt8"] += 1
            if ls >= 286:
                st["litlen_286_287"] += 1
            if ds >= 30:
                st["offset_30_31"] += 1
            if lit[ls] == 1 and ls == 285:
                st["amp_1bit_285"] += 1
            _match_stats(st, out, length, d)
            out += length
        assert lit[256] or b.kind == "dynamic", "EOB"
        if lit[256]:
            w.huff(lc[256], lit[256])
            if lit[256] == 15:
                st["eob_15bit"] += 1
        st["huff_blocks"] += 1
    if chunk:
        w.bits(0, 3)
        w.align()
        w.raw(b"\x00\x00\xff\xff")
        st["chunk_form"] += 1
    return w.value()


def _match_stats(st, out, length, d):
    st["matches"] += 1
    if d in (NEAR, NEAR + 1):
        st["dist_%d" % d] += 1
    src = out - d
    if d <= NEAR:
        st["near"] += 1
        if src % RING + length > RING:
            st["near_src_wraps_ring"] += 1
        if out % RING + length > RING:
            st["dst_wraps_ring"] += 1
        if d < length <= 16:
            st["overlap_le16"] += 1
    else:
        st["far"] += 1
        if src % PIECE + min(length, d) > PIECE:
            st["far_src_crosses_piece"] += 1
    if length <= 8:
        st["len_le8"] += 1
    elif length <= 16:
        st["len_9_16"] += 1
    if d == out:
        st["dist_eq_out"] += 1


def _write_dynamic_header(w, b, lit, dist, st):
    hlit = b.hlit or max(257, max((i + 1 for i, l in enumerate(lit) if l), default=0))
    hdist = b.hdist or max(1, max((i + 1 for i, l in enumerate(dist) if l), default=0))
    seq = list(lit[:hlit]) + [0] * (hlit - len(lit)) + list(dist[:hdist]) + [0] * (hdist - len(dist))
    if b.items is not None:
        items = b.items
    elif b.rle == "split":
        items = _rle(seq[:hlit], "zlib") + [(s, e, v, i + hlit, r) for s, e, v, i, r in _rle(seq[hlit:], "zlib")]
    else:
        items = _rle(seq, b.rle)
    for s, e, v, i, r in items:
        if r > 1 and i < hlit < i + r:
            st["repeat_crosses_boundary"] += 1
            st["repeat_crosses_boundary_%d" % s] += 1
    pf = collections.Counter(it[0] for it in items)
    if b.pre_lens is not None:
        pl = b.pre_lens
    else:
        if len(pf) == 1:                          # zlib wants a complete precode: a second, unused codeword
            pf[0 if 0 not in pf else 1] = 0.5
        pl = auto_lengths(pf, 19, 7)
    hclen = max(4, max(k + 1 for k in range(19) if pl[PRECODE_ORDER[k]]))
    if b.hclen:
        assert b.hclen >= hclen
        hclen = b.hclen
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(pl[PRECODE_ORDER[k]], 3)
    pc = canonical(pl)
    for s, e, v, i, r in items:
        w.huff(pc[s], pl[s])
        w.bits(v, e)
    st["hlit_%d" % hlit] += 1
    st["hdist_%d" % hdist] += 1
    st["hclen_%d" % hclen] += 1
    st["rle_" + (b.rle if b.items is None else "given")] += 1
    for l in lit:
        if l > 9:
            st["litlen_codeword_gt9_defined"] += 1
    if lit[256] == 15:
        st["eob_len15_defined"] += 1


def expand(blocks):
    """The high-precision reference: the output of the token lists, one byte at a time."""
    out = bytearray()
    put = out.append
    for b in blocks:
        if b.kind == "stored":
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                put(t)
                continue
            length, d = t[0], t[1]
            assert 1 <= d <= len(out), "distance %d past the %d bytes produced" % (d, len(out))
            for _ in range(length):
                put(out[-d])
    return bytes(out)


class Case:
    """one stream with its answer: `code` for hdo_inflate / the plain entry points, `code_flushed` for the
    flushed ones; `expected` the output when the code is 0; `zlib` False for the libdeflate-only forms"""
    __slots__ = ("name", "family", "stream", "cap", "code", "expected", "code_flushed", "chunk", "zlib", "stats",
                 "blocks")

    def __init__(self, name, family, stream, cap, code, expected, code_flushed=None, chunk=False, zlib_ok=True,
                 stats=None):
        self.name, self.family, self.stream, self.cap = name, family, stream, cap
        self.code, self.expected = code, expected
        self.code_flushed = code if code_flushed is None else code_flushed
        self.chunk, self.zlib, self.stats = chunk, zlib_ok, stats or collections.Counter()
        self.blocks = None

    def tuple(self):
        return self.name, self.stream, self.cap, self.code, self.expected


def valid(name, family, blocks, chunk=False, zlib_ok=True, cap=None):
    st = collections.Counter()
    s = encode(blocks, chunk=chunk, stats=st)
    exp = expand(blocks)
    if chunk:
        # the plain inflate reads on past the marker: a zero header (stored, non-final), then no LEN -> bad data
        c = Case(name, family, s, len(exp) if cap is None else cap, BAD_DATA, exp, OK, True, zlib_ok, st)
    else:
        c = Case(name, family, s, len(exp) if cap is None else cap, OK, exp, zlib_ok=zlib_ok, stats=st)
    c.blocks = blocks
    return c


def fault(name, family, stream, code, cap, code_flushed=None, stats=None):
    return Case(name, family, stream, cap, code, b"", code_flushed, stats=stats)


# ---- token helpers --------------------------------------------------------------------------------------------


def rand_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def lits(data):
    return list(bytes(data))


def sym_tokens(rng, syms, n, out0, dist_syms=()):
    """n tokens drawn from the litlen symbols `syms` (literals and length symbols; a length symbol only where an
    offset symbol of `dist_syms` reaches back no further than the output so far)"""
    toks, out = [], out0
    for _ in range(n):
        s = int(syms[int(rng.integers(0, len(syms)))])
        if s < 256:
            toks.append(s)
            out += 1
            continue
        ok = [d for d in dist_syms if DIST_BASE[d] <= out]
        if s == 256 or not ok:
            continue
        ds = int(ok[int(rng.integers(0, len(ok)))])
        hi = min(out, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1)
        d = int(rng.integers(DIST_BASE[ds], hi + 1))
        lb = LEN_BASE[s - 257]
        ln = lb + int(rng.integers(0, 1 << LEN_EXTRA[s - 257])) if s < 285 else 258
        if s == 284:
            ln = min(ln, 257)                    # 284 + 31 would also say 258: not a form encoders write
        toks.append((ln, d, s, ds))
        out += ln
    return toks


# ---- families ---------------------------------------------------------------------------------------------------

MATCH_LENGTHS = [3, 4, 8, 9, 15, 16, 17, 63, 64, 65, 66, 128, 257, 258]
MATCH_DISTS = list(range(1, 21)) + [64, 65, 255, 256, 257, 1023, 1024, 1025, 1725, 1726, 1727, 2047, 2048, 2049,
                                    4096, 8193, 16385, 24577, 32767, 32768]


def _phases(length, d):
    """output positions (mod RING) for a (length, distance) match: the destination at and across the ring's wrap
    and a piece edge, the source at and across them"""
    h = length // 2
    dst = {0, 1, RING - 1, PIECE - 1, (RING - h) % RING, (PIECE - h) % RING}
    src = {(s + d) % RING for s in (0, RING - 1, PIECE - 1, (RING - h) % RING, (PIECE - h) % RING)}
    return sorted(dst | src)


def fam_match_matrix(rng):
    """every (length, distance) at the output phases of _phases: stored filler of random bytes brings the output
    to the phase, a Huffman block (static or derived dynamic) holds 0 / 2 / 37 / 300 random literals, the match,
    a few literals"""
    cases = []
    for d in MATCH_DISTS:
        work = [(ln, ph) for ln in MATCH_LENGTHS for ph in _phases(ln, d)]
        k = 0
        while work:
            blocks = [Block("stored", data=rand_bytes(rng, d))]
            out = d
            while work and out < 48000:
                ln, ph = work.pop()
                nl = (0, 2, 37, 300)[k % 4]
                fill = (ph - nl - out) % RING
                blocks.append(Block("stored", data=rand_bytes(rng, fill)))
                out += fill
                pre = lits(rand_bytes(rng, nl))
                post = lits(rand_bytes(rng, 3))
                kind = ("static", "dynamic")[k % 2]
                blocks.append(Block(kind, tokens=pre + [(ln, d)] + post))
                out += nl + ln + 3
                k += 1
            blocks[-1].final = True
            cases.append(valid("match_d%d_%d" % (d, len(cases)), "match_matrix", blocks))
        # a distance of exactly the bytes produced, and one more (bad data); the match is the first token of a block
        # and, in a second stream, a token deep inside one
        for ln in (3, 258):
            pre = rand_bytes(rng, d)
            cases.append(valid("dist_eq_out_d%d_l%d" % (d, ln), "match_matrix",
                               [Block("stored", data=pre), Block("static", tokens=[(ln, d), 7], final=True)]))
        body = lits(rand_bytes(rng, min(d, 200)))
        toks = body + [(17, d), 1, 2] if d <= 200 else None
        if toks:
            cases.append(valid("dist_eq_out_inline_d%d" % d, "match_matrix", [Block("dynamic", tokens=toks, final=True)]))
        # (the stats would count this match as reaching back exactly to the start: it is one byte further)
        s = encode([Block("stored", data=rand_bytes(rng, d - 1)), Block("static", tokens=[(3, d), 7], final=True)])
        cases.append(fault("dist_past_out_d%d" % d, "faults", s, BAD_DATA, d + 1000))
    return cases


def fam_code_shapes(rng):
    cases = []
    pool_lits = list(rng.permutation(256)[:60])
    for L in range(10, 16):
        # litlen: EOB, 285 and a few literals at L bits, the rest completes the code
        fixed = {256: L, 285: L, int(pool_lits[0]): L, int(pool_lits[1]): L}
        syms = [int(s) for s in pool_lits[2:40]] + [257, 264, 265, 272, 280, 284]
        lit = fill_lengths(fixed, syms, 286)
        dist = auto_lengths({0: 3, 3: 2, 4: 1, 10: 1, 16: 1, 22: 1}, 30)
        long_syms = [s for s in fixed if s != 256]
        all_syms = [s for s in range(286) if lit[s] and s != 256]
        dsyms = [s for s in range(30) if dist[s]]
        prefix = Block("stored", data=rand_bytes(rng, 3000))
        for where in ("start", "middle", "end"):
            run = sym_tokens(rng, long_syms, 40, 3000, dsyms)
            other = sym_tokens(rng, all_syms, 300, 3000, dsyms)
            toks = run + other if where == "start" else other + run if where == "end" else other[:150] + run + other[150:]
            # the run was drawn at out=3000; redraw positions are all >= 3000 so every distance stays valid
            for rle in ("zlib", "plain"):
                cases.append(valid("litlen_%dbit_run_%s_%s" % (L, where, rle), "code_shapes",
                                   [prefix, Block("dynamic", tokens=toks, lit_lens=lit, dist_lens=dist, rle=rle,
                                                  final=True)]))
        # offset codes of L - 1 .. 15 bits
        dfixed = {29: 15, 28: 15, 20: L - 1, 5: L - 1}
        dist2 = fill_lengths(dfixed, [s for s in range(30) if s not in dfixed], 30)
        dsyms2 = [s for s in range(30) if dist2[s]]
        lit2 = auto_lengths(collections.Counter({s: 1 for s in list(range(65, 91)) + [256, 258, 266, 270, 285]}), 286)
        syms2 = [s for s in range(286) if lit2[s] and s != 256]
        pre2 = Block("stored", data=rand_bytes(rng, 32768))
        toks = sym_tokens(rng, syms2, 400, 32768, dsyms2)
        cases.append(valid("offset_%dbit" % (L - 1), "code_shapes",
                           [pre2, Block("dynamic", tokens=toks, lit_lens=lit2, dist_lens=dist2, final=True)]))
        longd = [(ln, d, s, ds) for t in toks if not isinstance(t, int) for (ln, d, s, ds) in [t] if dist2[ds] >= L - 1]
        if longd:
            cases.append(valid("offset_%dbit_run" % (L - 1), "code_shapes",
                               [pre2, Block("dynamic", tokens=[65, 66] + longd * 3 + [67], lit_lens=lit2, dist_lens=dist2,
                                            final=True)]))
    # HLIT 257 / 286 and HDIST 1 / 30 in the same block; the allowed incomplete offset codes
    lit_only = lits(rand_bytes(rng, 500))
    cases.append(valid("hlit257_empty_offset_code", "code_shapes",
                       [Block("dynamic", tokens=lit_only, final=True)]))
    cases.append(valid("hlit257_hdist30_empty_offset_code", "code_shapes",
                       [Block("dynamic", tokens=lit_only, dist_lens=[0] * 30, hdist=30, final=True)]))
    for ds in (0, 3, 17, 29):
        d0 = DIST_BASE[ds]
        dl = [0] * 30
        dl[ds] = 1
        pre = rand_bytes(rng, 32768)
        toks = [(int(rng.integers(3, 259)), d0 + int(rng.integers(0, 1 << DIST_EXTRA[ds]))) for _ in range(50)]
        cases.append(valid("single_offset_codeword_sym%d" % ds, "code_shapes",
                           [Block("stored", data=pre), Block("dynamic", tokens=toks, dist_lens=dl, hdist=30 if ds < 29 else None,
                                                             hlit=286, final=True)]))
    # a literal-only code: only EOB (single length-1 codeword) in a block of its own
    el = [0] * 286
    el[256] = 1
    cases.append(valid("litlen_only_eob", "code_shapes",
                       [Block("static", tokens=[5, 6]), Block("dynamic", tokens=[], lit_lens=el, final=True)]))
    # code-length runs across the litlen/offset boundary: zeros (17, 18) and a repeated length (16)
    for kind in ("zeros", "nonzero"):
        pre = rand_bytes(rng, 4000)
        if kind == "zeros":                                      # litlen 261..285 and offset 0..24 zero: one 18 run
            f = collections.Counter({s: 1 for s in range(0, 200)})
            f.update({256: 1, 260: 1, 285: 1})
            lit = auto_lengths(f, 286)
            lit[285] = 0
            lit[255] = lit[255] or max(lit)
            lit = fill_lengths({}, [s for s in range(286) if lit[s]], 286)
            dist = fill_lengths({}, [25, 26, 27, 28, 29], 30)
        else:                                                    # litlen 270..285 and offset 0..5 all 8 bits: 16s
            lit = fill_lengths({s: 8 for s in range(0, 100)} | {s: 8 for s in range(270, 286)} | {256: 8},
                               list(range(100, 160)), 286)
            dist = fill_lengths({s: 8 for s in range(0, 6)}, list(range(6, 30)), 30)
        for h, rle in ((None, "zlib"), (19, "zlib"), (None, "split")):
            lsyms = [s for s in range(286) if lit[s] and s != 256]
            dsyms = [s for s in range(30) if dist[s]]
            toks = sym_tokens(rng, lsyms, 600, 32768, dsyms)
            cases.append(valid("cross_boundary_%s_hclen%s_%s" % (kind, h or "min", rle), "code_shapes",
                               [Block("stored", data=pre + rand_bytes(rng, 32768 - len(pre))),
                                Block("dynamic", tokens=toks, lit_lens=lit, dist_lens=dist, hclen=h, rle=rle,
                                      final=True)]))
    # HLIT 288 / HDIST 32 (libdeflate reads them; zlib rejects "too many symbols")
    for hl, hd in ((288, 30), (286, 32), (288, 32)):
        toks = lits(rand_bytes(rng, 100)) + [(10, 3), (40, 90)]
        lit = auto_lengths(collections.Counter(toks[:100] + [256, len_sym(10), len_sym(40)]), 286) + [0, 0]
        dist = auto_lengths(collections.Counter({dist_sym(3): 1, dist_sym(90): 1}), 30) + [0, 0]
        cases.append(valid("hlit%d_hdist%d" % (hl, hd), "code_shapes",
                           [Block("dynamic", tokens=toks, lit_lens=lit, dist_lens=dist, hlit=hl, hdist=hd, final=True)],
                           zlib_ok=False))
    return cases


def fam_amplify(rng):
    cases = []
    for n in (1000, 4000):
        for d in (1, 2, 3, 4):
            lit = [0] * 286
            lit[285], lit[256], lit[65] = 1, 2, 3
            lit[66] = 3
            dl = [0] * 30
            dl[d - 1] = 1
            head = [65, 66, 65, 66][:d]
            cases.append(valid("amp_285_1bit_d%d_x%d" % (d, n), "amplify",
                               [Block("dynamic", tokens=head + [(258, d)] * n + [66], lit_lens=lit, dist_lens=dl,
                                      final=True)]))
    # Z_RLE-like: short runs at distance 1..4 of every length
    toks = [9, 8, 7, 6]
    for k in range(2000):
        toks.append((int(rng.integers(3, 259)), int(rng.integers(1, 5))))
        toks.append(int(rng.integers(0, 256)))
    cases.append(valid("rle_runs_d1_4", "amplify", [Block("dynamic", tokens=toks, final=True)]))
    # stored data re-copied at distance 32768, again and again
    lit = [0] * 286
    lit[285], lit[256] = 1, 1
    dl = [0] * 30
    dl[29] = 1
    cases.append(valid("stored_recopied_d32768", "amplify",
                       [Block("stored", data=rand_bytes(rng, 32768)),
                        Block("dynamic", tokens=[(258, 32768)] * 1000, lit_lens=lit, dist_lens=dl, final=True)]))
    return cases


def fam_blocks(rng):
    cases = []
    cases.append(valid("stored_empty_final", "blocks", [Block("stored", final=True)]))
    cases.append(valid("stored_empty_x5", "blocks", [Block("stored")] * 4 + [Block("static", tokens=[1, 2, 3]),
                                                                             Block("stored", final=True)]))
    for n in (1, 65535, "split"):
        for a in range(8):
            # a static block of 9-bit literals in front: 3 + 9a + 7 bits -> the stored header at every bit alignment
            lead = Block("static", tokens=[200 + i for i in range(a)])
            if n == "split":
                body = [Block("stored", data=rand_bytes(rng, 65535)), Block("stored", data=rand_bytes(rng, 1), final=True)]
            else:
                body = [Block("stored", data=rand_bytes(rng, n), final=True)]
            cases.append(valid("stored_%s_align%d" % (n, a), "blocks", [lead] + body))
    # hundreds of five-token blocks alternating stored / static / dynamic
    for seed_k in range(3):
        blocks = []
        for k in range(200):
            kind = ("stored", "static", "dynamic")[(k + seed_k) % 3]
            if kind == "stored":
                blocks.append(Block("stored", data=rand_bytes(rng, 5)))
            else:
                toks = lits(rand_bytes(rng, 3)) + [(int(rng.integers(3, 20)), int(rng.integers(1, 4))), 9]
                blocks.append(Block(kind, tokens=toks))
        blocks[-1].final = True
        cases.append(valid("tiny_blocks_200_%d" % seed_k, "blocks", blocks))
    # a dynamic block header right after a 258-byte match
    for kind in ("static", "dynamic"):
        pre = lits(rand_bytes(rng, 300))
        cases.append(valid("header_after_258_%s" % kind, "blocks",
                           [Block(kind, tokens=pre + [(258, 300)]), Block("dynamic", tokens=[(258, 1), 4, (100, 600)]),
                            Block("static", tokens=[(258, 258), 5], final=True)]))
    # static litlen 286/287 (length 258) and offset 30/31 (24577 + 13 bits): libdeflate decodes them, zlib rejects
    pre = rand_bytes(rng, 32768)
    for ls, ds in ((286, 0), (287, 5), (285, 30), (257, 31), (286, 31)):
        d = DIST_BASE[ds] + (int(rng.integers(0, 1 << DIST_EXTRA[ds])) if ds < 30 else int(rng.integers(0, 8192)))
        ln = 258 if ls >= 285 else 3
        cases.append(valid("static_lit%d_off%d" % (ls, ds), "libdeflate_only",
                           [Block("stored", data=pre), Block("static", tokens=[1, (ln, d, ls, ds), 2, (ln, d, ls, ds)],
                                                              final=True)], zlib_ok=False))
    return cases


def fam_faults(rng):
    cases = []
    big = 1 << 17
    good = [Block("static", tokens=lits(b"fault base ") + [(5, 3)])]
    s = encode(good + [Block("btype3")]) + b"\0\0"
    cases.append(fault("btype3", "faults", s, BAD_DATA, big))
    cases.append(fault("btype3_first", "faults", encode([Block("btype3")]) + b"\0\0", BAD_DATA, big))
    cases.append(fault("stored_nlen", "faults", encode([Block("stored", data=b"abcdef", nlen=0xfff8, final=True)]),
                       BAD_DATA, big))
    cases.append(fault("stored_nlen_first_byte", "faults",
                       encode(good + [Block("stored", data=b"abcdef", nlen=0xfff9 ^ 0x100, final=True)]), BAD_DATA, big))
    for have in (0, 50, 99):
        cases.append(fault("stored_len_past_input_%d" % have, "faults",
                           encode(good + [Block("stored", data=rand_bytes(rng, have), length=100, final=True)]),
                           BAD_DATA, big))
    cases.append(fault("stored_header_cut", "faults", encode(good) + b"\x00\x05\x00", BAD_DATA, big))
    # code-length items: a 16 first; repeats past HLIT + HDIST (by 16, 17, 18)
    lit = auto_lengths(collections.Counter({65: 1, 66: 1, 256: 1}), 286)
    seq_items = _rle(lit[:257] + [1], "zlib")
    cases.append(fault("rep16_first", "faults",
                       encode([Block("dynamic", tokens=[65], lit_lens=lit, dist_lens=[1] + [0] * 29,
                                     items=[(16, 2, 0, 0, 3)] + seq_items, final=True)]), BAD_DATA, big))
    for sym, e, r in ((18, 7, 11), (17, 3, 3), (16, 2, 3)):
        # the one offset length (HLIT + HDIST = 258) given as a run of r: past the end
        items = _rle(lit[:257], "zlib") + [(sym, e, 0, 257, r)]
        cases.append(fault("repeat_overrun_%d" % sym, "faults",
                           encode([Block("dynamic", tokens=[65], lit_lens=lit, dist_lens=[1] + [0] * 29, items=items,
                                         final=True)]), BAD_DATA, big))
    # over-subscribed and incomplete codes (litlen, offset, precode)
    base_lit = auto_lengths(collections.Counter({s: 1 for s in range(60, 80)} | {256: 1, 260: 1}), 286)
    over = list(base_lit)
    over[100] = min(l for l in base_lit if l)
    inc = list(base_lit)
    inc[max((s for s in range(286) if inc[s] and s not in (60, 61, 256, 260)), key=lambda s: (inc[s], s))] = 0
    toks = [60, 61, (6, 1)]
    dl = auto_lengths({0: 1, 1: 1}, 30)
    cases.append(fault("litlen_oversubscribed", "faults",
                       encode([Block("dynamic", tokens=toks, lit_lens=over, dist_lens=dl, final=True)]), BAD_DATA, big))
    cases.append(fault("litlen_incomplete", "faults",
                       encode([Block("dynamic", tokens=toks, lit_lens=inc, dist_lens=dl, final=True)]), BAD_DATA, big))
    one2 = [0] * 286
    one2[256] = 2
    cases.append(fault("litlen_single_2bit", "faults",
                       encode([Block("dynamic", tokens=[], lit_lens=one2, final=True)]), BAD_DATA, big))
    for nm, d in (("offset_oversubscribed", [1, 1, 1] + [0] * 27), ("offset_incomplete_1_2", [1, 2] + [0] * 28),
                  ("offset_single_2bit", [2] + [0] * 29), ("offset_incomplete_two_2bit", [2, 2] + [0] * 28)):
        cases.append(fault(nm, "faults", encode([Block("dynamic", tokens=toks[:2] + [(4, 1)], dist_lens=d, final=True)]),
                           BAD_DATA, big))
    # (written by hand: four 1-bit precode lengths for 16, 17, 18, 0; HCLEN 4)
    w = BitWriter()
    for v, n in ((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (1, 3), (1, 3), (1, 3)):
        w.bits(v, n)
    cases.append(fault("precode_oversubscribed", "faults", w.value() + bytes(8), BAD_DATA, big))
    # EOB with no codeword: the block never ends -- the decoder reads on past the input
    noeob = fill_lengths({}, list(range(97, 123)), 286)
    cases.append(fault("eob_len0", "faults",
                       encode([Block("dynamic", tokens=lits(b"hello"), lit_lens=noeob, final=True)]), BAD_DATA, big))
    cases.append(fault("empty_input", "faults", b"", BAD_DATA, big))
    # input cut inside a block (stored, static, dynamic)
    for kind in ("stored", "static", "dynamic"):
        if kind == "stored":
            bl = [Block("static", tokens=[1, 2]), Block("stored", data=rand_bytes(rng, 300), final=True)]
        else:
            bl = [Block(kind, tokens=lits(rand_bytes(rng, 200)) + [(50, 100)] + lits(rand_bytes(rng, 100)), final=True)]
        s = encode(bl)
        n = len(expand(bl))
        for cut in (len(s) // 2, len(s) - 20):
            cases.append(fault("cut_in_%s_%d" % (kind, cut), "faults", s[:cut], BAD_DATA, n + 20000))
    # one byte over the cap on a literal, on a match, on a stored block
    for nm, bl in (("literal", [Block("static", tokens=lits(b"abcdefg"), final=True)]),
                   ("match", [Block("static", tokens=lits(b"abcdefg") + [(30, 7)], final=True)]),
                   ("stored", [Block("static", tokens=lits(b"abc")), Block("stored", data=b"defghij", final=True)])):
        n = len(expand(bl))
        cases.append(fault("cap_over_on_%s" % nm, "faults", encode(bl), INSUFFICIENT_SPACE, n - 1))
    return cases


def corpus(seed=2026):
    """every case of every family (a few thousand streams), cap = exact for the valid ones; plus cap = exact - 1
    (INSUFFICIENT_SPACE) for every valid stream with output"""
    rng = np.random.default_rng(seed)
    fams = [fam_match_matrix(rng), fam_code_shapes(rng), fam_amplify(rng), fam_blocks(rng)]
    cases = [c for f in fams for c in f]
    # the chunk form of every fifth valid stream of each family
    cases += [valid("chunk_" + c.name, "chunk_" + c.family, c.blocks, chunk=True, zlib_ok=c.zlib)
              for f in fams for c in f[::5] if c.blocks]
    cases += fam_faults(rng)
    cases += chunk_cases(rng)
    tight = []
    for c in cases:
        if c.code == OK and c.expected:
            tight.append(Case(c.name + "_cap_minus1", "cap_minus1", c.stream, len(c.expected) - 1, INSUFFICIENT_SPACE, b"",
                              zlib_ok=c.zlib))
        if c.chunk and c.expected:
            tight.append(Case(c.name + "_cap_minus1", "cap_minus1", c.stream, len(c.expected) - 1, INSUFFICIENT_SPACE,
                              b"", chunk=True, zlib_ok=c.zlib))
    return cases + tight


def chunk_cases(rng):
    """the chunk form (every block non-final, the sync marker behind them) of stream shapes from every family"""
    out = []
    r2 = np.random.default_rng(int(rng.integers(0, 1 << 31)))
    for name, blocks in _chunk_shapes(r2):
        out.append(valid("chunk_" + name, "chunk", blocks, chunk=True))
    return out


def _chunk_shapes(rng):
    pre = rand_bytes(rng, 2500)
    yield "near_far", [Block("stored", data=pre),
                       Block("static", tokens=[(ln, d) for ln in (3, 9, 16, 17, 258) for d in (1, 8, 1726, 1727, 2049)])]
    yield "long_codes", [Block("stored", data=pre),
                         Block("dynamic", tokens=sym_tokens(rng, [65, 66, 285, 270], 300, 2500, [0, 21]),
                               lit_lens=fill_lengths({256: 15, 285: 15, 65: 14}, [270] + list(range(66, 90)), 286),
                               dist_lens=fill_lengths({21: 9}, list(range(21)), 30))]
    yield "amplify", [Block("static", tokens=[1] + [(258, 1)] * 500)]
    yield "stored_65535", [Block("static", tokens=[200, 201]), Block("stored", data=rand_bytes(rng, 65535))]
    yield "stored_empty", [Block("stored")]
    yield "tiny_blocks", [Block(("stored", "static", "dynamic")[k % 3], data=rand_bytes(rng, 5) if k % 3 == 0 else b"",
                                tokens=[] if k % 3 == 0 else [4, 5, (6, 2)]) for k in range(120)]
    yield "cross_boundary", [Block("stored", data=pre),
                             Block("dynamic", tokens=lits(rand_bytes(rng, 400)) + [(20, 2000)],
                                   rle="zlib", hclen=19)]
    yield "header_after_258", [Block("static", tokens=lits(pre[:300]) + [(258, 300)]), Block("dynamic", tokens=[(258, 1)])]
    yield "ends_on_match", [Block("static", tokens=[7, (258, 1), (258, 1)])]
    yield "ends_on_literal", [Block("dynamic", tokens=lits(b"xyz" * 40))]


_cached = None


def cached_corpus():
    """corpus() once per process"""
    global _cached
    if _cached is None:
        _cached = corpus()
    return _cached


# ---- the second corpus: the latency kernel's geometry (k_inflate_lat, hd_inflate_lat.hpp) -------------------------
#
# That kernel keeps the last 64 KiB of output in LDS and deals a stream to four wavefronts: the front parses and
# hands records on (a window of <= LAT_WIN output bytes, one literal, one match, one stored block of any length,
# the end), the sort stores a window's literals into the ring and passes every record on, the back executes the
# records in order.  LAT_FQ records wait between front and sort, LAT_PQ between sort and back.  Three things can
# go wrong there that corpus() never reaches: an index across the 64 KiB wrap, an output larger than the ring
# (every stream of corpus() stops before 48,000 bytes or is one stored block), and the sort's literal stores
# running more than the ring's spare half ahead of the back when the records in between are large stored blocks.

LAT_WRAP_DISTS = [1, 2, 7, 8, 9, 16, 17, 64, 65, 258, 1024, 32767, 32768]
LAT_LEAD_LITS = 6000        # more than LAT_FQ + LAT_PQ windows of LAT_WIN bytes
LAT_LEAD_MATCHES = [(258, 32768), (9, 32768), (64, 30000), (17, 16400)]
LAT_SIZES = [65535, 65536, 65537, 131071, 131072, 131073, 1048575, 1048576, 1048577]


def match_fill(rng, out, target):
    """blocks that bring the output from `out` to `target` cheaply: a stored seed of 300 random bytes if there is
    no history yet, then one static block of (258, 300) matches and fewer than 258 random literals"""
    blocks, gap = [], target - out
    assert gap >= 0
    if out < 300 and gap:
        n = min(gap, 300)
        blocks.append(Block("stored", data=rand_bytes(rng, n)))
        gap -= n
    if gap:
        blocks.append(Block("static", tokens=[(258, 300)] * (gap // 258) + lits(rand_bytes(rng, gap % 258))))
    return blocks


def lat_stats(blocks):
    """what a block list reaches of the latency kernel's geometry, counted from the lists"""
    st = collections.Counter()
    out, run = 0, []                                 # run: the stored blocks directly in front of the next block
    for b in blocks:
        if b.kind == "stored":
            if b.data and out % LAT_RING + len(b.data) > LAT_RING:
                st["lat_stored_wraps_ring"] += 1
            if b.data:
                run.append(len(b.data))
            out += len(b.data)
            continue
        nlit = sum(1 for t in b.tokens if isinstance(t, int))
        if nlit and run:
            # what can lie between the back and the sort's stores: the stored records still queued, and the
            # windows queued with them (counted as LAT_LEAD_LITS bytes whatever the block holds)
            lead = sum(run[-(LAT_FQ + LAT_PQ + 1):]) + LAT_LEAD_LITS
            if lead >= LAT_RING:
                st["lat_inflight_ge_64k"] += 1
            elif lead >= LAT_RING // 2:
                st["lat_inflight_32k_64k"] += 1
        run = []
        for t in b.tokens:
            if isinstance(t, int):
                out += 1
                continue
            ln, d = t[0], t[1]
            if out % LAT_RING + ln > LAT_RING:
                st["lat_dst_wraps_ring"] += 1
            if (out - d) % LAT_RING + min(ln, d) > LAT_RING:
                st["lat_src_wraps_ring"] += 1
            out += ln
    if out > LAT_RING:
        st["lat_out_gt_64k"] += 1
    if abs(out - LAT_MAX_OUT) <= 1:
        st["lat_out_1mib"] += 1
    return st


def stored_lead(stream):
    """the output bytes of the stored blocks a raw DEFLATE stream starts with (0: it starts with a Huffman block),
    read from the headers: what tells whether an encoder's stream puts large stored records in flight"""
    pos, total = 0, 0                                # pos: a bit position
    while 8 * len(stream) - pos >= 3:
        nxt = stream[(pos >> 3) + 1] if (pos >> 3) + 1 < len(stream) else 0
        hdr = (stream[pos >> 3] | nxt << 8) >> (pos & 7)
        if (hdr >> 1) & 3:
            break
        p = (pos + 3 + 7) >> 3
        ln, nl = int.from_bytes(stream[p:p + 2], "little"), int.from_bytes(stream[p + 2:p + 4], "little")
        assert len(stream) >= p + 4 and ln == nl ^ 0xffff
        total += ln
        pos = 8 * (p + 4 + ln)
        if hdr & 1:
            break
    return total


def lat_valid(name, family, blocks, chunk=False, extra=None):
    blocks[-1].final = True
    c = valid(name, family, blocks, chunk=chunk)
    c.stats.update(lat_stats(blocks))
    if extra:
        c.stats.update(extra)
    return c


def _lat_wrap_items():
    """(near, far): the matches of lat_wrap as (length, distance, kind, offset of the destination from the wrap).
    kind d<phase>: the destination starts at wrap + phase; s<phase>: the source does.  phase A = -length // 2,
    B = -1, 0, 1.  `far` holds the source kinds of the distances whose destination lies clear of the wrap, three
    queues that share a visit of a wrap with one `near` item.  The full matrix (14 lengths x 13 distances x 8
    kinds x 3 wraps) does not fit the corpus's budget of output bytes: every (length, distance) is there with its
    destination across the wrap at both phases that span it, the other kinds are a stride through the matrix."""
    def phases(ln):
        return (("A", -(ln // 2)), ("B", -1), ("0", 0), ("1", 1))
    span = [(ln, d, "d" + p, o) for p in "AB" for d in LAT_WRAP_DISTS for ln in MATCH_LENGTHS
            for q, o in phases(ln) if q == p]
    other = [(ln, d, "d" + p, o) for p in "01" for d in LAT_WRAP_DISTS for ln in MATCH_LENGTHS
             for q, o in phases(ln) if q == p]
    other += [(ln, d, "s" + p, o + d) for p in "AB01" for d in LAT_WRAP_DISTS if d < 258 for ln in MATCH_LENGTHS
              for q, o in phases(ln) if q == p]
    other = [other[(i * 13) % len(other)] for i in range(136)]
    near = []
    while span or other:                             # about three spanning ones to one of the others
        near += span[:3] + other[:1]
        span, other = span[3:], other[1:]
    far = []
    for ds in ((258,), (1024,), (32767, 32768)):
        q = [(ln, d, "s" + p, o + d) for ln in MATCH_LENGTHS for d in ds for p, o in phases(ln)]
        far.append([q[(i * 5) % len(q)] for i in range(len(q))])       # (5 is coprime to 56 and 112)
    return near, far


def fam_lat_wrap(rng):
    """matches whose destination or source lies at and across a multiple of 64 KiB (65536 m, m = 1, 2 in the short
    streams, m = 1..15 in the long ones), reached with match filler only: no large record is ever in flight, a
    failure here is a failure of the wrap.  0 / 2 / 37 / 300 literals in front of the match in its own block,
    static and derived dynamic blocks"""
    near, far = _lat_wrap_items()
    cases, k, s = [], 0, 0
    while near or any(far):
        long_one = (s % 17) in (0, 2, 5, 7, 10, 12, 15)
        blocks, out, extra = [], 0, collections.Counter()
        for m in (range(1, 16) if long_one else (1, 2)):
            wrap = m * LAT_RING
            for q in [near] + far:
                if not q:
                    continue
                ln, d, kind, o = q[0]
                nl = (0, 2, 37, 300)[k % 4]
                if wrap + o - nl < out:              # the visit's earlier matches are in the way: at a later wrap
                    continue
                q.pop(0)
                blocks += match_fill(rng, out, wrap + o - nl)
                blocks.append(Block(("static", "dynamic")[(k + k // 4) % 2],
                                    tokens=lits(rand_bytes(rng, nl)) + [(ln, d)] + lits(rand_bytes(rng, 3))))
                out = wrap + o + ln + 3
                extra["lat_wrap_" + kind] += 1
                extra["lat_wrap_pair_%d_%d" % (ln, d)] += 1
                extra["lat_wrap_m%d" % m] += 1
                k += 1
        cases.append(lat_valid("lat_wrap_%d" % s, "lat_wrap", blocks, extra=extra))
        s += 1
        assert s < 120
    # a stored block of 5,000 bytes across the wrap
    blocks, out = [], 0
    for m, back in ((1, 2500), (2, 1), (15, 4999)):
        blocks += match_fill(rng, out, m * LAT_RING - back) + [Block("stored", data=rand_bytes(rng, 5000))]
        out = m * LAT_RING - back + 5000
    blocks.append(Block("static", tokens=[(258, 5000), 1, 2, 3]))
    cases.append(lat_valid("lat_wrap_stored_5000", "lat_wrap", blocks))
    # a run of 13..15-bit codewords across it: the scalar path's records, one literal or one match each
    pool = [int(x) for x in rng.permutation(256)[:40]]
    for L, m in ((13, 1), (14, 1), (15, 1), (15, 2)):
        fixed = {256: L, 285: L, pool[0]: L, pool[1]: L}
        lit = fill_lengths(fixed, pool[2:] + [257, 264, 265, 272, 280, 284], 286)
        dist = auto_lengths({0: 3, 3: 2, 4: 1, 10: 1, 16: 1, 22: 1}, 30)
        dsyms = [x for x in range(30) if dist[x]]
        start = m * LAT_RING - 30
        run = sym_tokens(rng, [285, pool[0], pool[1]], 60, start, dsyms)
        other = sym_tokens(rng, [x for x in range(286) if lit[x] and x != 256], 100, start, dsyms)
        assert sum(1 if isinstance(t, int) else t[0] for t in run) > 30
        cases.append(lat_valid("lat_wrap_%dbit_run_m%d" % (L, m), "lat_wrap", match_fill(rng, 0, start) +
                               [Block("dynamic", tokens=run + other, lit_lens=lit, dist_lens=dist)]))
    # 200 KiB of (258, 1) at one bit per token: the ring wrapped three times by the windows' budget cuts
    lit = [0] * 286
    lit[285], lit[256], lit[65], lit[66] = 1, 2, 3, 3
    n = -(-200 * 1024 // 258)
    cases.append(lat_valid("lat_wrap_amp_285_1bit_200k", "lat_wrap",
                           [Block("dynamic", tokens=[65] + [(258, 1)] * n + [66], lit_lens=lit,
                                  dist_lens=[1] + [0] * 29)]))
    return cases


def _lead_block(rng, kind, match_first=False):
    body = lits(rand_bytes(rng, LAT_LEAD_LITS))
    post = lits(rand_bytes(rng, 100))
    return Block(kind, tokens=LAT_LEAD_MATCHES + body + post if match_first else body + LAT_LEAD_MATCHES + post)


def fam_lat_lead(rng):
    """large stored records in flight, then a Huffman block of 6,000 literals -- more than eight windows: the sort
    stores them while the back still copies the stored blocks -- then matches that read back into the stored
    bytes and 100 literals.  Each shape with a static block (no table build: the front is at its fastest) and
    with a dynamic one"""
    cases = []
    for kind in ("static", "dynamic"):
        for L in (32768, 57344, 61440, 65535):
            for b in (0, 1000, 40000, LAT_RING + 77):
                cases.append(lat_valid("lat_lead_one_%d_at_%d_%s" % (L, b, kind), "lat_lead", match_fill(rng, 0, b) +
                                       [Block("stored", data=rand_bytes(rng, L)), _lead_block(rng, kind)]))
        for L, ks in ((16383, (4, 5, 9, 12)), (65535, (2, 3, 15))):
            for n in ks:
                cases.append(lat_valid("lat_lead_%dx%d_%s" % (n, L, kind), "lat_lead",
                                       [Block("stored", data=rand_bytes(rng, L)) for _ in range(n)] +
                                       [_lead_block(rng, kind)]))
        blocks = []
        for _ in range(6):
            blocks += [Block("stored", data=rand_bytes(rng, 65535)), _lead_block(rng, kind)]
        cases.append(lat_valid("lat_lead_alternating_x6_%s" % kind, "lat_lead", blocks))
        cases.append(lat_valid("lat_lead_match_first_%s" % kind, "lat_lead",
                               [Block("stored", data=rand_bytes(rng, 65535)), _lead_block(rng, kind, True)]))
    return cases


_WORDS = [b"the", b"ring", b"holds", b"every", b"source", b"a", b"window", b"of", b"literals", b"goes", b"ahead",
          b"stored", b"block", b"behind", b"it", b"and", b"back", b"wavefront", b"copies", b"in", b"order"]


def _text_tokens(rng, n):
    """n output bytes that look like text to an encoder: words as literals, earlier phrases as matches"""
    toks, out = [], 0
    while out < n:
        if out > 100 and n - out >= 3 and int(rng.integers(0, 2)):
            ln = min(int(rng.integers(3, 40)), n - out)
            toks.append((ln, int(rng.integers(1, out + 1))))
            out += ln
        else:
            w = (_WORDS[int(rng.integers(0, len(_WORDS)))] + b" ")[:n - out]
            toks += lits(w)
            out += len(w)
    return toks


def fam_lat_sizes(rng):
    """outputs at and around the ring's size, twice it, and the largest room the latency kernel takes (one byte
    more goes to the lone launch of the batch kernel): of match filler, and of stored blocks with a text-like
    dynamic block behind them"""
    cases = []
    for n in LAT_SIZES:
        cases.append(lat_valid("lat_size_%d_fill" % n, "lat_sizes", match_fill(rng, 0, n)))
        tail = 3000 + n % 7
        piece = 65535 if n > 200000 else 16383
        blocks, left = [], n - tail
        while left:
            blocks.append(Block("stored", data=rand_bytes(rng, min(left, piece))))
            left -= len(blocks[-1].data)
        cases.append(lat_valid("lat_size_%d_stored_text" % n, "lat_sizes",
                               blocks + [Block("dynamic", tokens=_text_tokens(rng, tail))]))
    return cases


def lat_corpus(seed=2027):
    """the families aimed at the latency kernel; cap = exact, plus cap = exact - 1 (INSUFFICIENT_SPACE) for every
    valid case with output, plus the chunk form of one shape per family"""
    rng = np.random.default_rng(seed)
    fams = [fam_lat_wrap(rng), fam_lat_lead(rng), fam_lat_sizes(rng)]
    cases = [c for f in fams for c in f]
    for f, pick in zip(fams, ("lat_wrap_1", "lat_lead_one_65535_at_1000_static", "lat_size_131073_stored_text")):
        c = next(c for c in f if c.name == pick)
        cases.append(valid("chunk_" + c.name, "chunk_" + c.family, c.blocks, chunk=True))
        cases[-1].stats.update(lat_stats(c.blocks))
    tight = [Case(c.name + "_cap_minus1", "cap_minus1", c.stream, len(c.expected) - 1, INSUFFICIENT_SPACE, b"",
                  chunk=c.chunk) for c in cases if c.expected]
    return cases + tight


_cached_lat = None


def cached_lat_corpus():
    """lat_corpus() once per process"""
    global _cached_lat
    if _cached_lat is None:
        _cached_lat = lat_corpus()
    return _cached_lat
