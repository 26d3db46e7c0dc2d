"""A plain raw-DEFLATE token reader, written from RFC 1951 (plain Python; the slot tables are deflate_gen's).

`read(stream)` decodes a stream into its blocks and records, for every block, what an encoder put there:
the type, BFINAL, the first and the end bit, the code lengths (dynamic blocks), and the tokens with the output
position of each.  Stored blocks keep their length; an empty stored block that is not final is a SYNC FLUSH
point (the 00 00 ff ff marker of a full or sync flush), and `Stream.flushes` lists them.

It shares nothing with the oracle (oracle/hd_inflate.c), the CPU twin or the kernels: it is the second reader the
encode contracts (encode_contracts.py) stand on.  Which codes it takes is restated from the oracle's build_code() (`_table`);
the forms only libdeflate decodes -- its symbols, its one-symbol codes read from either bit -- are read with `wide=True` alone.  tests/test_index_models_vs_oracle.py holds the index
models built on `_table` and `_dynamic_header` to the oracle's verdicts.
"""
from deflate_gen import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, PRECODE_ORDER, STATIC_DIST, STATIC_LIT, rev


class DeflateError(ValueError):
    pass


class Block:
    """kind 'stored' | 'static' | 'dynamic'.  Tokens are three parallel lists: pos (output position of the token's
    first byte), length (0 = a literal), value (the literal byte, or the match distance).  Dynamic blocks also keep
    hlit / hdist / hclen and the litlen, offset and precode lengths as sent."""
    __slots__ = ("kind", "final", "start_bit", "end_bit", "out_start", "out_end", "pos", "length", "value",
                 "lit_lens", "dist_lens", "pre_lens", "hlit", "hdist", "hclen", "stored_len")

    def __init__(self, kind, final, start_bit, out_start):
        self.kind, self.final, self.start_bit, self.out_start = kind, final, start_bit, out_start
        self.end_bit = self.out_end = None
        self.pos, self.length, self.value = [], [], []
        self.lit_lens = self.dist_lens = self.pre_lens = None
        self.hlit = self.hdist = self.hclen = None
        self.stored_len = None

    @property
    def sync_flush(self):
        """an empty, non-final stored block: the marker a sync / full flush leaves"""
        return self.kind == "stored" and not self.final and self.stored_len == 0

    def tokens(self):
        """(pos, length, value) triples"""
        return list(zip(self.pos, self.length, self.value))

    def matches(self):
        """(pos, length, distance) of the matches"""
        return [(p, ln, d) for p, ln, d in zip(self.pos, self.length, self.value) if ln]


class Stream:
    __slots__ = ("blocks", "end_bit", "out", "nbytes")

    @property
    def flushes(self):
        """(block index, output position) of every sync-flush marker"""
        return [(i, b.out_start) for i, b in enumerate(self.blocks) if b.sync_flush]

    def all_matches(self):
        return [m for b in self.blocks for m in b.matches()]


def _table(lens, either_bit=False):
    """decode table of a code: index = the next `maxl` stream bits (LSB first) -> (symbol << 4) | length; -1 where no
    codeword is assigned.  An over-subscribed code is refused; so is an incomplete one, but for the empty code and the code
    of a single 1-bit codeword.  either_bit: those two as oracle/hd_inflate.c build_code() has them -- one symbol (0 for the
    empty code) from either value of one bit; without it the unused value has no codeword, as RFC 1951 and zlib have it."""
    maxl = max(lens) if any(lens) else 0
    if maxl == 0:
        return ([(0 << 4) | 1] * 2 if either_bit else [-1, -1]), 1
    t = [-1] * (1 << maxl)
    nxt, code, cnt = {}, 0, [0] * 16
    for l in lens:
        if l:
            cnt[l] += 1
    used = sum(c << (15 - l) for l, c in enumerate(cnt) if l)
    if used > 1 << 15:
        raise DeflateError("over-subscribed code")
    if used < 1 << 15:
        if used != 1 << 14 or cnt[1] != 1:
            raise DeflateError("incomplete code")
        e = (list(lens).index(1) << 4) | 1
        return [e, e if either_bit else -1], 1
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    for s, l in enumerate(lens):
        if l:
            r = rev(nxt[l], l)
            nxt[l] += 1
            t[r::1 << l] = [(s << 4) | l] * (1 << (maxl - l))
    return t, maxl


_STATIC = None


def _static_tables():
    global _STATIC
    if _STATIC is None:
        _STATIC = (_table(STATIC_LIT), _table(STATIC_DIST))
    return _STATIC


class _Bits:
    """LSB-first reader; reading past the end raises"""

    def __init__(self, data):
        self.data, self.pos, self.nbits = bytes(data), 0, 8 * len(data)

    def get(self, n):
        if n == 0:
            return 0
        p = self.pos
        if p + n > self.nbits:
            raise DeflateError("stream ends inside a block (bit %d)" % p)
        v = int.from_bytes(self.data[p >> 3:(p + n + 7 >> 3) + 1], "little") >> (p & 7)
        self.pos = p + n
        return v & ((1 << n) - 1)

    def sym(self, table, maxl):
        p = self.pos
        v = int.from_bytes(self.data[p >> 3:(p + maxl + 7 >> 3) + 1], "little") >> (p & 7)
        e = table[v & ((1 << maxl) - 1)]
        if e < 0:
            raise DeflateError("bits %d: no codeword" % p)
        self.pos = p + (e & 15)
        if self.pos > self.nbits:
            raise DeflateError("stream ends inside a codeword")
        return e >> 4


def _dynamic_header(bits, blk, oracle=False):
    """oracle: the oracle's rules alone -- none for a litlen code without an end-of-block codeword (such a block never ends:
    its reader runs out of input), an empty precode is a code like the others, and the one-symbol codes decode from either bit"""
    hlit = bits.get(5) + 257
    hdist = bits.get(5) + 1
    hclen = bits.get(4) + 4
    pre = [0] * 19
    for k in range(hclen):
        pre[PRECODE_ORDER[k]] = bits.get(3)
    if not oracle and not any(pre):
        raise DeflateError("empty precode")
    pt, pm = _table(pre, oracle)
    seq = []
    while len(seq) < hlit + hdist:
        s = bits.sym(pt, pm)
        if s < 16:
            seq.append(s)
        elif s == 16:
            if not seq:
                raise DeflateError("repeat with no previous length")
            seq += [seq[-1]] * (3 + bits.get(2))
        elif s == 17:
            seq += [0] * (3 + bits.get(3))
        else:
            seq += [0] * (11 + bits.get(7))
    if len(seq) != hlit + hdist:
        raise DeflateError("code-length repeat runs past HLIT + HDIST")
    blk.hlit, blk.hdist, blk.hclen = hlit, hdist, hclen
    blk.pre_lens, blk.lit_lens, blk.dist_lens = pre, seq[:hlit], seq[hlit:]
    if not oracle and blk.lit_lens[256] == 0:
        raise DeflateError("no end-of-block code")
    off = _table(blk.dist_lens, oracle)                # the offset code first, as the oracle builds them
    return _table(blk.lit_lens, oracle), off


def read(stream, expand=True, stop_at_final=True, wide=False):
    """-> Stream.  Decodes until a final block, or (stop_at_final False, or no final block) until the bytes run
    out on a block end.  expand: also rebuild the output (Stream.out), byte by byte for overlapping copies.
    wide: also the forms only libdeflate (and so the oracle) decodes -- litlen symbols 286 / 287 as length 258, offset
    symbols 30 / 31 as 24577 + 13 bits, a match through the empty offset code as offset symbol 0, the unused bit value of
    a one-codeword code, a litlen code without end-of-block; without it they are refused, as RFC 1951 has them and as no
    encoder may write them."""
    bits = _Bits(stream)
    out = bytearray()
    nout = 0
    blocks = []
    while True:
        if bits.pos + 3 > bits.nbits or (blocks and blocks[-1].final and stop_at_final):
            break
        if blocks and not blocks[-1].final and bits.nbits - bits.pos < 8 and \
                (bits.pos & 7) == 0:
            break                                      # byte-aligned end after a non-final block (flush forms)
        start = bits.pos
        final = bits.get(1)
        btype = bits.get(2)
        if btype == 3:
            raise DeflateError("block type 3 at bit %d" % start)
        blk = Block(("stored", "static", "dynamic")[btype], bool(final), start, nout)
        blocks.append(blk)
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            ln, nl = bits.get(16), bits.get(16)
            if ln != (~nl & 0xffff):
                raise DeflateError("stored LEN / NLEN mismatch at bit %d" % start)
            b0 = bits.pos >> 3
            if b0 + ln > len(bits.data):
                raise DeflateError("stored block runs past the stream")
            if expand:
                out += bits.data[b0:b0 + ln]
            bits.pos += 8 * ln
            nout += ln
            blk.stored_len = ln
        else:
            if btype == 1:
                (lt, lm), (dt, dm) = _static_tables()
            else:
                (lt, lm), (dt, dm) = _dynamic_header(bits, blk, oracle=wide)
            P, L, V = blk.pos, blk.length, blk.value
            sym = bits.sym
            while True:
                s = sym(lt, lm)
                if s < 256:
                    P.append(nout)
                    L.append(0)
                    V.append(s)
                    if expand:
                        out.append(s)
                    nout += 1
                    continue
                if s == 256:
                    break
                if s > (287 if wide else 285):
                    raise DeflateError("litlen symbol %d" % s)
                k = s - 257
                length = LEN_BASE[k] + bits.get(LEN_EXTRA[k])
                if not wide and blk.dist_lens is not None and not any(blk.dist_lens):
                    raise DeflateError("match in a block with no offset code")
                ds = sym(dt, dm)
                if ds > (31 if wide else 29):
                    raise DeflateError("offset symbol %d" % ds)
                d = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                if d > nout:
                    raise DeflateError("distance %d past the %d bytes produced" % (d, nout))
                P.append(nout)
                L.append(length)
                V.append(d)
                if expand:
                    if d >= length:
                        out += out[nout - d:nout - d + length]
                    else:
                        for _ in range(length):
                            out.append(out[-d])
                nout += length
        blk.end_bit = bits.pos
        blk.out_end = nout
    st = Stream()
    st.blocks, st.end_bit, st.nbytes = blocks, bits.pos, len(bits.data)
    st.out = bytes(out) if expand else None
    return st
