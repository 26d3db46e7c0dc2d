"""The encoder's promises, one function each, checked on the tokens of a stream (deflate_tokens.py).

`check(stream, data, level, form, room)` returns the list of `Violation`s of an encoded member: a rule name, an
output position and what was seen.  Every rule names the line of include/hipdeflate_params.h it restates (the
`HDR` citations below are looked up in the header when this module loads, so a moved line moves with it), and
where the header's words leave a bound open, the comment says which kernel line fixes it.

forms: 'plain' (hdo_deflate_twin, HD_FRAME_RAW), 'flush' (HD_FRAME_RAW_FLUSH), 'lat' and 'lat_flush' (the same with
HD_FRAME_LATENCY: hip_deflate, the hook, the lat contexts).  `room` is the destination size the encoder was given:
the latency form is taken only when it covers that form's worst case, the ordinary form otherwise
(oracle/hd_deflate_twin.c twin(), hd_segment.hpp).

Nothing here calls the oracle, the twin or a kernel.
"""
import collections
import os
import re

import deflate_tokens

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hipdeflate_params.h")


def _header():
    """{name: (value or None, line)} of every #define, and {marker text: line} for the prose rules"""
    defs = {}
    lines = open(HEADER).read().split("\n")
    for i, ln in enumerate(lines, 1):
        m = re.match(r"#define\s+(\w+)(\([^)]*\))?\s+(.*?)\s*(/\*.*)?$", ln)
        if not m or m.group(1) in defs:
            continue
        val = None
        if not m.group(2):
            try:
                val = int(eval(re.sub(r"(?<=[0-9a-fA-F])u\b", "", m.group(3)), {}))
            except Exception:
                pass
        defs[m.group(1)] = (val, i)
    return defs, lines


_DEFS, _LINES = _header()


def V(name):
    return _DEFS[name][0]


def HDR(name):
    """'hipdeflate_params.h:<line>' of a #define, or of the first line holding a phrase"""
    if name in _DEFS:
        return "hipdeflate_params.h:%d" % _DEFS[name][1]
    for i, ln in enumerate(_LINES, 1):
        if name in ln:
            return "hipdeflate_params.h:%d" % i
    raise KeyError(name)


WAVE, MIN_MATCH, MAX_MATCH, PIECE, LOOKAHEAD = V("HD_WAVE"), V("HD_MIN_MATCH"), V("HD_MAX_MATCH"), V("HD_PIECE"), V("HD_LOOKAHEAD")
L1_WIN, L2_WIN, L2_MIN_LEN = 1 << V("HD_L1_WIN_BITS"), 1 << V("HD_L2_WIN_BITS"), V("HD_L2_MIN_LEN")
WG_LEVEL, WG_WINDOW, WG_MIN_LEN, WG_CUT = V("HD_WG_LEVEL"), V("HD_WG_WINDOW"), V("HD_WG_MIN_LEN"), V("HD_WG_CUT")
WG_SPLIT_MIN, WG_SPLIT_OBS = V("HD_WG_SPLIT_MIN"), V("HD_WG_SPLIT_OBS")
BLOCK_TOKENS = V("HD_DYN_BLOCK_TOKENS")
SEG_BYTES, SEG_LIMIT = V("HD_SEG_BYTES"), V("HD_SEG_LIMIT")
PART_BYTES, PRIME_BYTES = V("HD_LAT_PART_BYTES"), V("HD_LAT_PRIME_BYTES")
SEG_PRIME = V("HD_LAT_SEG_PRIME")
LITLEN_MAXBITS, OFFSET_MAXBITS, PRECODE_MAXBITS = V("HD_LITLEN_MAXBITS"), V("HD_OFFSET_MAXBITS"), V("HD_PRECODE_MAXBITS")
_lat_seg = re.search(r"<= 1 \? (\d+)u : (\d+)u", _LINES[_DEFS["HD_LAT_SEG_BYTES"][1] - 1])
LAT_SEG = {1: int(_lat_seg.group(1)), 2: int(_lat_seg.group(2))}
_prime_min = re.search(r"\(n\) >= (\d+)u", _LINES[_DEFS["HD_LAT_PRIME"][1] - 1])
PRIME_MIN_N = int(_prime_min.group(1))            # 64: parts / segments shorter than this are not primed

FORMS = ("plain", "flush", "lat", "lat_flush")

Violation = collections.namedtuple("Violation", "rule pos what source")


def lat_prime(o, n):
    """HD_LAT_PRIME(o, n)"""
    return PRIME_BYTES if o >= PRIME_BYTES and n >= PRIME_MIN_N else 0


def stored_size(n):
    """HD_STORED_SIZE(n)"""
    return n + 5 * (1 if n == 0 else (n + 65534) // 65535)


def seg_worst(n, seg, flush):
    """HD_SEGN_WORST(n, seg, flush)"""
    return (n // seg) * (stored_size(seg) + 5) + (stored_size(n % seg) + 5 if n % seg else 0) + (0 if flush else 2)


# ---- the layout a member must have ------------------------------------------------------------------------------

Unit = collections.namedtuple("Unit", "start end prime seg")     # one parse: [start, end), primed with `prime` bytes


def layout(n, level, form, room=None):
    """-> (segments, units): the segments [start, end) the member is cut into (one segment = not segmented) and the
    parse units inside them (levels 1..2).  The choices restate twin() / twin_segmented() from their header lines:
      * levels >= HD_WG_LEVEL: one stream in every form ("long blocks ... no segments", "ONE codec per level");
      * levels 1..2 in a latency form, n > HD_LAT_SEG_BYTES(level) and room >= HD_SEGN_WORST: segments of
        HD_LAT_SEG_BYTES(level), a segment behind the first primed with HD_LAT_PRIME(HD_LAT_PRIME_BYTES, its length);
        at level 2 every segment parsed in HD_LAT_PART_BYTES parts (HD_LAT_PARTS), each primed with HD_LAT_PRIME(
        bytes ahead of it in the segment, its length) -- the first one with the segment's own priming;
      * else levels 1..2, n > HD_SEG_LIMIT: HD_SEG_BYTES segments, not primed."""
    flush = form.endswith("flush")
    lat = form.startswith("lat")
    seg = None
    if 1 <= level < WG_LEVEL:
        if lat and n > LAT_SEG[level] and (room is None or room >= seg_worst(n, LAT_SEG[level], flush)):
            seg = LAT_SEG[level]
        elif n > SEG_LIMIT:
            seg = SEG_BYTES
    if seg is None:
        return [(0, n)], [Unit(0, n, 0, 0)]
    segs, units = [], []
    for s in range(0, n, seg):
        e = min(n, s + seg)
        segs.append((s, e))
        sp = lat_prime(PRIME_BYTES, e - s) if (SEG_PRIME and s and seg != SEG_BYTES) else 0
        if level == 2 and seg == LAT_SEG[2]:
            for ps in range(s, e, PART_BYTES):
                pe = min(e, ps + PART_BYTES)
                units.append(Unit(ps, pe, lat_prime(ps - s, pe - ps) if ps > s else lat_prime(sp, pe - ps), len(segs) - 1))
        else:
            units.append(Unit(s, e, sp, len(segs) - 1))
    return segs, units


def ring_lo(q, pn, win):
    """Levels 1..2: the oldest byte a candidate may name, in parse coordinates (0 = where the parse starts, priming
    included).  The header says "4 KiB window" (HD_L1_WIN_BITS, HD_L2_WIN_BITS); the exact bound is the ring's:
    the step at S refills the ring a HD_PIECE at a time until it holds HD_LOOKAHEAD bytes past S or the whole parse
    (hd_deflate_static.hpp:595, hd_deflate_dynamic.hpp:1166), and a candidate must lie at or after
    filled - 2^WIN_BITS (hd_deflate_static.hpp:597 + the okm test, hd_deflate_dynamic.hpp:1168).  So the farthest
    reach is 4096 - HD_LOOKAHEAD + 63 = 3775 inside a block and 4096 - HD_MIN_MATCH = 4092 at its end: a distance
    of 4096 is never written."""
    S = q - q % WAVE
    want = min(pn, S + LOOKAHEAD)
    filled = -(-want // PIECE) * PIECE
    return filled - win


# ---- the checks ---------------------------------------------------------------------------------------------------


def _v(out, rule, pos, what, src):
    out.append(Violation(rule, pos, what, src))


def check_end(st, form, out):
    """Flush forms end in a sync flush -- an empty stored block, BFINAL = 0, the stream's last bytes 00 00 ff ff
    (DESIGN.md:214, HD_FRAME_RAW_FLUSH) -- and no block is final.  Ordinary members: the last block and no other has
    BFINAL = 1, and the stream ends in that block's last byte."""
    blocks = st.blocks
    if not blocks:
        _v(out, "end", 0, "no block", "DESIGN.md:214")
        return
    finals = [i for i, b in enumerate(blocks) if b.final]
    if form.endswith("flush"):
        if finals:
            _v(out, "end.flush_no_final", blocks[finals[0]].out_start, "a final block in a flush form", "DESIGN.md:214")
        if not blocks[-1].sync_flush or st.end_bit != 8 * st.nbytes:
            _v(out, "end.flush_sync", blocks[-1].out_start, "does not end in 00 00 ff ff", "DESIGN.md:214")
    else:
        if finals != [len(blocks) - 1]:
            _v(out, "end.final", blocks[-1].out_start, "final blocks at %s of %d" % (finals[:4], len(blocks)), "RFC 1951 3.2.3")
        if (st.end_bit + 7) // 8 != st.nbytes:
            _v(out, "end.trailing", blocks[-1].out_end, "%d bytes behind the final block" % (st.nbytes - (st.end_bit + 7) // 8),
               "RFC 1951 3.2.3")


def _complete(lens, maxbits):
    return sum(1 << (maxbits - l) for l in lens if l) == 1 << maxbits


def check_header(blk, out):
    """Every dynamic header: litlen and offset lengths <= 15 (HD_LITLEN_MAXBITS, HD_OFFSET_MAXBITS), precode lengths <= 7
    (HD_PRECODE_MAXBITS), HLIT <= 286 and HDIST <= 30 (RFC 1951 3.2.7), and every code complete -- or, for the offset
    code, one of the incomplete shapes RFC 1951 3.2.7 allows: one codeword of one bit, or none at all."""
    src = HDR("HD_LITLEN_MAXBITS")
    if max(blk.lit_lens) > LITLEN_MAXBITS or max(blk.dist_lens) > OFFSET_MAXBITS:
        _v(out, "header.maxbits", blk.out_start, "code length > 15", src)
    if max(blk.pre_lens) > PRECODE_MAXBITS:
        _v(out, "header.precode_maxbits", blk.out_start, "precode length > 7", HDR("HD_PRECODE_MAXBITS"))
    if blk.hlit > 286 or blk.hdist > 30:
        _v(out, "header.hlit_hdist", blk.out_start, "HLIT %d HDIST %d" % (blk.hlit, blk.hdist), "RFC 1951 3.2.7")
    if not _complete(blk.pre_lens, 7):
        _v(out, "header.precode_complete", blk.out_start, "incomplete precode", "RFC 1951 3.2.7")
    if not _complete(blk.lit_lens, 15):
        _v(out, "header.litlen_complete", blk.out_start, "incomplete litlen code", "RFC 1951 3.2.7")
    used = [l for l in blk.dist_lens if l]
    if not (_complete(blk.dist_lens, 15) or used == [1] or not used):
        _v(out, "header.offset_complete", blk.out_start, "offset code neither complete nor one 1-bit codeword", "RFC 1951 3.2.7")


def check_level0(st, out):
    """Level 0: stored blocks only (hipdeflate_params.h level map)."""
    for b in st.blocks:
        if b.kind != "stored":
            _v(out, "l0.stored_only", b.out_start, b.kind + " block", HDR("0      stored blocks only"))


def check_segments(st, segs, form, out):
    """Segmented members (levels 1..2): every segment is a run of blocks of its own that ends in a full flush exactly at
    the segment's end (HD_SEG_BYTES: "each ending in a full flush"; HD_LAT_SEG_BYTES: "coded, flushed and stitched
    exactly as the long blocks"), and an ordinary member has the empty final block 03 00 behind the last one.  Not
    segmented: no flush marker but a flush form's last one."""
    src = HDR("HD_SEG_BYTES") if segs[0][1] - segs[0][0] == SEG_BYTES else HDR("HD_LAT_SEG_BYTES")
    flushes = [(i, pos) for i, pos in st.flushes]
    want = [e for _, e in segs] if len(segs) > 1 else ([segs[0][1]] if form.endswith("flush") else [])
    got = [pos for _, pos in flushes]
    if len(segs) == 1 and not form.endswith("flush"):
        want = []
    if got != want:
        _v(out, "seg.flush_points", got[0] if got else 0, "flushes at %s, segment ends %s" % (got[:6], want[:6]), src)
    if len(segs) > 1 and not form.endswith("flush"):
        last = st.blocks[-1]
        if not (last.final and last.kind == "static" and not last.pos and last.start_bit == 8 * (st.nbytes - 2)
                and st.nbytes >= 2 and st.blocks[-2].sync_flush):
            _v(out, "seg.final_03_00", segs[-1][1], "no empty final block 03 00 behind the last segment", HDR("an empty final block (03 00)"))


def _segment_blocks(st, segs):
    """{segment index: [blocks holding data of it]} (marker and final empty blocks left out)"""
    ends = [e for _, e in segs]
    res = collections.defaultdict(list)
    k = 0
    for b in st.blocks:
        if b.sync_flush or (b.final and b.kind != "stored" and not b.pos and b.out_start == b.out_end):
            continue
        while k + 1 < len(segs) and b.out_start >= ends[k]:
            k += 1
        res[k].append(b)
    return res


def check_small_levels(st, data, level, form, segs, units, out):
    """Levels 1..2, per parse unit: matches of at least HD_MIN_MATCH / HD_L2_MIN_LEN bytes, inside the ring window
    (ring_lo), none running past the unit's end, none reaching back across the unit's start by more than its
    priming (HD_LAT_PRIME: 512, or 0 for the first segment, for HD_SEG_BYTES segments and for a part or segment of
    fewer than 64 bytes).  Level 1 writes static or stored blocks only; a segment is either all Huffman or all stored;
    level 2 closes a block of a whole-segment parse at the first step boundary where it holds HD_DYN_BLOCK_TOKENS
    tokens (and not behind the last step), and writes ONE block per latency segment (parts: "ONE wavefront builds
    one code over the tokens of all parts and emits them as one DEFLATE block")."""
    win = L1_WIN if level == 1 else L2_WIN
    min_len = MIN_MATCH if level == 1 else L2_MIN_LEN
    src_win = HDR("HD_L1_WIN_BITS") if level == 1 else HDR("HD_L2_WIN_BITS")
    src_min = HDR("HD_MIN_MATCH") if level == 1 else HDR("HD_L2_MIN_LEN")
    by_seg = _segment_blocks(st, segs)
    lat_parts = level == 2 and len(segs) > 1 and segs[0][1] == LAT_SEG[2]
    for k, (s, e) in enumerate(segs):
        blks = by_seg.get(k, [])
        kinds = {b.kind for b in blks}
        if "stored" in kinds and kinds - {"stored"}:
            _v(out, "seg.stored_all_or_none", s, "stored and Huffman blocks in one segment", HDR("HD_STORED_SIZE(n)"))
        for b in blks:
            if b.out_start < s or b.out_end > e:
                _v(out, "seg.block_in_segment", b.out_start, "block [%d, %d) crosses segment [%d, %d)" % (b.out_start, b.out_end, s, e),
                   HDR("HD_SEG_BYTES"))
            if level == 1 and b.kind == "dynamic":
                _v(out, "l1.static_or_stored", b.out_start, "dynamic block at level 1", HDR("1      greedy parse, static Huffman"))
        huff = [b for b in blks if b.kind != "stored"]
        if lat_parts and len(huff) > 1:
            _v(out, "l2.lat_one_block", s, "%d blocks in one latency segment" % len(huff), HDR("emits them as one DEFLATE block"))
        if level == 2 and not lat_parts:
            _check_l2_blocks(huff, s, e, out)
    ui = 0
    units_sorted = sorted(units)
    for b in st.blocks:
        for p, ln, d in zip(b.pos, b.length, b.value):
            if not ln:
                continue
            while ui + 1 < len(units_sorted) and p >= units_sorted[ui].end:
                ui += 1
            u = units_sorted[ui]
            if ln < min_len:
                _v(out, "l12.min_len", p, "length %d" % ln, src_min)
            if p + ln > u.end:
                _v(out, "l12.unit_end", p, "match [%d, %d) past the parse's end %d" % (p, p + ln, u.end),
                   HDR("HD_LAT_PART_BYTES") if lat_parts else HDR("HD_SEG_BYTES"))
            if p - d < u.start - u.prime:
                _v(out, "l12.prime_reach", p, "reaches %d back across %d (primed %d)" % (u.start - (p - d), u.start, u.prime),
                   HDR("HD_LAT_PRIME") if u.prime or u.start else HDR("HD_SEG_BYTES"))
            org = u.start - u.prime
            if p - d - org < ring_lo(p - org, u.end - org, win):
                _v(out, "l12.window", p, "distance %d outside the ring (oldest %d)" % (d, org + ring_lo(p - org, u.end - org, win)),
                   src_win)


def _check_l2_blocks(huff, s, e, out):
    """the token limit of a whole-segment level-2 parse (HD_DYN_BLOCK_TOKENS: "closed at the first step boundary at
    which it holds at least this many tokens"; steps stand on 64-byte strides from the segment's start)"""
    src = HDR("HD_DYN_BLOCK_TOKENS")
    last_step = s + (e - 1 - s) // WAVE * WAVE if e > s else s
    for i, b in enumerate(huff):
        nt = len(b.pos)
        if not nt:
            continue
        end_step = s + (b.pos[-1] - s) // WAVE * WAVE
        before = sum(1 for p in b.pos if p < end_step)
        if i + 1 < len(huff):
            if nt < BLOCK_TOKENS or before >= BLOCK_TOKENS:
                _v(out, "l2.block_tokens", b.out_end, "block of %d tokens (%d before its last step)" % (nt, before), src)
        else:
            if sum(1 for p in b.pos if p < last_step) >= BLOCK_TOKENS:
                _v(out, "l2.block_tokens", b.out_end, "last block runs past %d tokens" % BLOCK_TOKENS, src)


def check_wg(st, data, level, out):
    """Levels 3..9 (the workgroup parse): no match crosses a multiple of HD_WG_CUT; length >= HD_WG_MIN_LEN; distance
    <= HD_WG_WINDOW; one stream (no flush marker inside, whatever the length: "long blocks ... no segments"); a block
    ends only at a multiple of HD_WG_CUT, at the first one where it holds HD_DYN_BLOCK_TOKENS tokens, or by the split
    test -- then it is at least HD_WG_SPLIT_MIN bytes long, HD_WG_SPLIT_MIN bytes are left behind it, and it holds at
    least HD_WG_SPLIT_OBS tokens (the test runs only then; hd_deflate_twin.c deflate_wg, k_emit_wg's cut scan).  A
    member that falls back to stored is stored throughout."""
    n = len(data)
    kinds = {b.kind for b in st.blocks if not b.sync_flush}
    if "stored" in kinds and kinds - {"stored"}:
        _v(out, "wg.stored_all_or_none", 0, "stored and Huffman blocks in one member", HDR("HD_STORED_SIZE(n)"))
    huff = [b for b in st.blocks if b.kind != "stored"]
    for b in huff:
        for p, ln, d in zip(b.pos, b.length, b.value):
            if not ln:
                continue
            if p // WG_CUT != (p + ln - 1) // WG_CUT:
                _v(out, "wg.cut", p, "match [%d, %d) crosses %d" % (p, p + ln, (p // WG_CUT + 1) * WG_CUT), HDR("NO MATCH CROSSES"))
            if ln < WG_MIN_LEN:
                _v(out, "wg.min_len", p, "length %d" % ln, HDR("HD_WG_MIN_LEN"))
            if d > WG_WINDOW:
                _v(out, "wg.window", p, "distance %d" % d, HDR("HD_WG_WINDOW"))
    for i, b in enumerate(huff):
        last = i + 1 == len(huff)
        ntok = len(b.pos)
        # tokens before every interior cut of the block (no match crosses one, so the count is exact)
        cnt, j, first_full = 0, 0, None
        for c in range((b.out_start // WG_CUT + 1) * WG_CUT, min(b.out_end, n - 1) + 1, WG_CUT):
            if c >= n or (not last and c >= b.out_end):
                break
            while j < ntok and b.pos[j] < c:
                j += 1
            if j >= BLOCK_TOKENS:
                first_full = c
                break
        if first_full is not None:
            _v(out, "wg.block_tokens", first_full, "block goes on past %d tokens at the cut %d" % (BLOCK_TOKENS, first_full),
               HDR("blocks   a DEFLATE"))
        if last:
            continue
        here = b.out_end
        if here % WG_CUT:
            _v(out, "wg.block_end_at_cut", here, "block ends off a cut", HDR("blocks   a DEFLATE"))
        if ntok < BLOCK_TOKENS:                        # ended by the split test
            if here - b.out_start < WG_SPLIT_MIN or n - here < WG_SPLIT_MIN or ntok < WG_SPLIT_OBS:
                _v(out, "wg.split_min", here, "split block [%d, %d) of %d tokens, %d bytes behind" % (b.out_start, here, ntok, n - here),
                   HDR("HD_WG_SPLIT_MIN"))


def check(stream, data, level, form="plain", room=None, st=None):
    """-> list of Violations of one member (the raw DEFLATE payload) encoded from `data`"""
    out = []
    if st is None:
        try:
            st = deflate_tokens.read(stream, stop_at_final=True)
        except deflate_tokens.DeflateError as e:
            return [Violation("decode", 0, str(e), "RFC 1951")]
    if st.out != bytes(data):
        i = next((k for k in range(min(len(st.out), len(data))) if st.out[k] != data[k]), min(len(st.out), len(data)))
        _v(out, "roundtrip", i, "output differs from the input", "RFC 1951")
        return out
    check_end(st, form, out)
    for b in st.blocks:
        if b.kind == "dynamic":
            check_header(b, out)
    n = len(data)
    if level <= 0:
        check_level0(st, out)
        return out
    segs, units = layout(n, level, form, room)
    check_segments(st, segs, form, out)
    if level >= WG_LEVEL:
        check_wg(st, data, level, out)
    else:
        check_small_levels(st, data, level, form, segs, units, out)
    return out


# ---- what a member reaches (the coverage counts of test_encode_contracts.py) -------------------------------------

def edges(st, data, level, form, room=None):
    """Counter of the edges one member reaches"""
    c = collections.Counter()
    n = len(data)
    segs, units = layout(n, level, form, room)
    huff = [b for b in st.blocks if b.kind != "stored"]
    for b in huff:
        for p, ln, d in zip(b.pos, b.length, b.value):
            if not ln:
                continue
            c["matches"] += 1
            if d == 4096:
                c["dist_4096"] += 1
            if d == 32768:
                c["dist_32768"] += 1
            if level >= WG_LEVEL and (p + ln) % WG_CUT == 0:
                c["match_ends_at_cut"] += 1
            if ln == 258:
                c["len_258"] += 1
    if 1 <= level < WG_LEVEL:
        us = sorted(units)
        win = L1_WIN if level == 1 else L2_WIN
        ui = 0
        for b in huff:
            for p, ln, d in zip(b.pos, b.length, b.value):
                if not ln:
                    continue
                while ui + 1 < len(us) and p >= us[ui].end:
                    ui += 1
                u = us[ui]
                if u.prime and u.start - (p - d) == u.prime:
                    c["reach_%d_across_lat_border" % u.prime] += 1
                org = u.start - u.prime
                if p - d - org == ring_lo(p - org, u.end - org, win):
                    c["at_ring_edge"] += 1
        if len(segs) > 1:
            c["segmented_%d" % (segs[0][1] - segs[0][0])] += 1
    if level >= WG_LEVEL:
        for b in huff[:-1]:
            c["wg_block_end_tokens" if len(b.pos) >= BLOCK_TOKENS else "wg_block_end_split"] += 1
    elif level == 2:
        for b in huff[:-1]:
            if len(b.pos) >= BLOCK_TOKENS:
                c["l2_block_end_tokens"] += 1
    if any(b.kind == "stored" and b.stored_len for b in st.blocks) and level >= 1:
        c["stored_fallback"] += 1
    return c


# ---- many members at once -----------------------------------------------------------------------------------------

def _check_job(item):
    name, stream, data, level, form, room = item
    try:
        st = deflate_tokens.read(stream)
    except deflate_tokens.DeflateError as e:
        return name, [tuple(Violation("decode", 0, str(e), "RFC 1951"))], collections.Counter()
    return name, [tuple(v) for v in check(stream, data, level, form, room, st=st)], edges(st, data, level, form, room)


def check_many(items, nproc=None):
    """items: (name, stream, data, level, form, room).  -> ([(name, violation tuple)], Counter of edges), checked on a
    pool of fresh interpreters (spawned, not forked: a forked worker would inherit a parent's open GPU); a (stream,
    level class, form, layout) met twice is checked once"""
    import multiprocessing
    seen, jobs = set(), []
    for it in items:
        name, stream, data, level, form, room = it
        key = (hash(bytes(stream)), len(stream), min(level, WG_LEVEL), form.endswith("flush"),
               len(layout(len(data), level, form, room)[0]))
        if key not in seen:
            seen.add(key)
            jobs.append(it)
    jobs.sort(key=lambda j: -len(j[2]))
    nproc = nproc or max(1, min(8, os.cpu_count() or 1))
    with multiprocessing.get_context("spawn").Pool(nproc) as pool:
        res = pool.map(_check_job, jobs, chunksize=4)
    bad = [(name, v) for name, vs, _ in res for v in vs]
    total = collections.Counter()
    for _, _, e in res:
        total.update(e)
    total["members"] = len(jobs)
    return bad, total
