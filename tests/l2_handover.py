"""Level 2's hand-over between its two codecs, restated from the sources, and the inputs that sit on it (plain Python and
numpy; nothing here calls a kernel, the twin is called through `tokens()` and encode_room.Block only).

hd_deflate_dynamic.hpp launch_level2: a block of n bytes in a launch whose room is split_max = min(out_stride, out_cap)
is coded by
  * the SPLIT path -- k_deflate_static<TOK> parses into a record in HBM, k_deflate_dynamic<EMIT = 1> writes the member
    from it -- when n <= split_max and its tokens fit the record's cap_tok = split_max / 4 * 3 + 128 (split_layout);
  * the FUSED kernel -- k_deflate_dynamic<EMIT = 0>, a persistent grid of at most 2560 wavefronts -- when n > split_max,
    when a pass of the parse finds `tokens stored + tokens of the pass > cap_tok` (emit_tokens), and for every block of
    the launch when split_max > (256 << 10) + 65536 (split_sub_batch gives 0 blocks per launch pair).
The parse hands its tokens over in PASSES: a step (64 input positions) queues its tokens, 64 leave whenever 64 or more
wait, what waits leaves at a DEFLATE block close (the first step boundary with >= HD_DYN_BLOCK_TOKENS tokens in the
open block, never behind the last step) and at the block's end.  `passes()` replays that on the token positions of the
twin's own member, and `closes` must then be the twin's DEFLATE blocks -- test_l2_handover.py holds it to that.

The constants are read from the sources by regular expression: a change of geometry fails test_l2_handover.py instead
of moving the GPU cases of test_gpu_l2_handover.py off their edges without a word.

A case is (blocks, stride, cap): stride a multiple of 16, cap with the byte granularity (cap_tok moves by 3 per 4 bytes
of cap, so it only takes values = 2 mod 3).
"""
import collections
import os
import re

import numpy as np

import deflate_tokens
import encode_contracts as ec
import encode_gen
import encode_room as er
import hdtest

LEVEL = 2
_CSRC = os.path.join(hdtest.ROOT, "7bgzf_amd", "csrc")


def _src(name):
    return open(os.path.join(_CSRC, name)).read()


def _read_constants():
    """{name: value} -- every one from the line of the sources that sets it; a line that no longer reads so is an error"""
    st, dy = _src("hd_deflate_static.hpp"), _src("hd_deflate_dynamic.hpp")

    def one(pattern, text, what):
        m = re.search(pattern, text)
        assert m, "the sources no longer hold %s: restate tests/l2_handover.py" % what
        return [int(g, 0) for g in m.groups()]

    c = {}
    c["tok_div"], c["tok_mul"], c["tok_add"] = one(r"l\.cap_tok = full \?[^:]*: max_block / (\d+) \* (\d+) \+ (\d+);", st,
                                                   "split_layout's cap_tok")
    c["db_extra"], = one(r"l\.max_db = l\.cap_tok / HD_DYN_BLOCK_TOKENS \+ (\d+);", st, "split_layout's max_db")
    c["sub_max"], = one(r"constexpr uint32_t SPLIT_SUB_BATCH_MAX = (\d+);", dy, "SPLIT_SUB_BATCH_MAX")
    c["budget_mib"], c["budget_shift"] = one(r"constexpr uint64_t SPLIT_SCRATCH_BUDGET = \(uint64_t\)(\d+) << (\d+);", dy,
                                             "SPLIT_SCRATCH_BUDGET")
    a, b = one(r"inline uint32_t parse_slots\(\)\s*\{\s*return (\d+)u \* (\d+)u;", dy, "parse_slots()")
    c["parse_slots"] = a * b
    a, b = one(r"inline uint32_t dynamic_grid\(uint32_t nblocks\)\s*\{\s*const uint32_t slots = (\d+)u \* (\d+)u;", dy,
               "dynamic_grid()")
    c["fused_slots"] = a * b
    a, sh, add = one(r"if \(split_max > \((\d+)u << (\d+)\) \+ (\d+)u\)\s*return 0;", dy, "split_sub_batch's largest room")
    c["split_room_max"] = (a << sh) + add
    return c


def overflow_check_in_source():
    """emit_tokens hands a block over when `tokens stored + tokens of the pass > cap_tok`, as overflow_pass() restates it"""
    return re.search(r"if \(ntok_slab \+ count > lay\.cap_tok\)\s*return use_static = false;", _src("hd_deflate_static.hpp")) is not None


C = _read_constants()
FUSED_SLOTS = C["fused_slots"]
SPLIT_ROOM_MAX = C["split_room_max"]
BLOCK_TOKENS = ec.BLOCK_TOKENS
STEP = ec.WAVE


def cap_tok(split_max):
    """split_layout(split_max).cap_tok: the tokens a record holds"""
    return split_max // C["tok_div"] * C["tok_mul"] + C["tok_add"]


def record_bytes(split_max):
    """split_layout(split_max).bytes"""
    ct = cap_tok(split_max)
    max_db = ct // BLOCK_TOKENS + C["db_extra"]
    off_hist = (ct * 4 + 16 + max_db * 4 + 15) & ~15
    return off_hist + max_db * 320 * 4


def sub_batch(nblocks, split_max):
    """split_sub_batch: the blocks of one parse + emit launch pair; 0 = the fused kernel takes the whole launch"""
    sub = min((C["budget_mib"] << C["budget_shift"]) // record_bytes(split_max), C["sub_max"])
    if split_max > SPLIT_ROOM_MAX:
        return 0
    if sub >= nblocks:
        return nblocks
    slots = C["parse_slots"]
    if sub >= slots:
        sub -= sub % slots
    elif sub < slots // 2:
        sub = 0
    return sub


def fused_grid(nblocks):
    """dynamic_grid: the fused kernel's persistent wavefronts; wavefront j takes blocks j, j + grid, ..."""
    return min(nblocks, FUSED_SLOTS)


def route(n, tokens_per_pass, split_max):
    """'split' | 'fused' for a block of n bytes whose parse hands over `tokens_per_pass`, in a launch that has a split path"""
    if n > split_max or split_max > SPLIT_ROOM_MAX:
        return "fused"
    return "fused" if overflow_pass(tokens_per_pass, cap_tok(split_max)) is not None else "split"


def overflow_pass(tokens_per_pass, ct):
    """index of the pass whose tokens no longer fit a record of ct tokens, or None"""
    have = 0
    for k, c in enumerate(tokens_per_pass):
        if have + c > ct:
            return k
        have += c
    return None


Passes = collections.namedtuple("Passes", "counts kinds closes total")
# counts[k]: tokens of pass k; kinds[k]: 'full' (64, inside a step), 'close' (step_boundary, in front of a close),
# 'end' (behind the last step); closes: the DEFLATE blocks' token counts; total: all tokens


def passes(n, positions):
    """the parse's passes for a block of n bytes whose tokens start at `positions` (ascending)"""
    per_step = np.bincount(np.asarray(positions, dtype=np.int64) // STEP, minlength=(n + STEP - 1) // STEP) if n else []
    counts, kinds, closes = [], [], []
    queued = in_block = 0                       # tokens waiting; tokens of the open DEFLATE block, waiting ones included
    for s, c in enumerate(per_step):
        queued += int(c)
        in_block += int(c)
        if queued >= 64:
            counts.append(64)
            kinds.append("full")
            queued -= 64
        if in_block >= BLOCK_TOKENS and (s + 1) * STEP < n:
            if queued:
                counts.append(queued)
                kinds.append("close")
                queued = 0
            closes.append(in_block)
            in_block = 0
    if queued:
        counts.append(queued)
        kinds.append("end")
    if n:
        closes.append(in_block)
    return Passes(counts, kinds, closes, sum(counts))


_TOKENS = {}


def tokens(data):
    """(token start positions, the DEFLATE blocks' token counts) of the twin's level-2 member of `data`; cached"""
    k = hdtest.sha(data)
    if k not in _TOKENS:
        r, m = hdtest.oracle_twin(data, LEVEL, cap=2 * len(data) + 66560)
        assert r == 0
        st = deflate_tokens.read(m, expand=False)
        assert all(b.kind != "stored" for b in st.blocks) or len(data) == 0, "a stored member says nothing about the parse"
        _TOKENS[k] = ([p for b in st.blocks for p in b.pos], [len(b.pos) for b in st.blocks] if len(data) else [])
    return _TOKENS[k]


def block_passes(data):
    return passes(len(data), tokens(data)[0])


_MODELS = {}


def model(data, flush):
    """encode_room.Block of a block at level 2 (one twin call per form); cached by the bytes"""
    k = (hdtest.sha(data), flush)
    if k not in _MODELS:
        _MODELS[k] = er.Block(data, LEVEL, flush)
    return _MODELS[k]


def up16(v):
    return (v + 15) & ~15


def cap_for(ct, k=0):
    """a cap whose record holds exactly ct tokens (ct = 2 mod 3), + k of the 4 bytes that do not move it"""
    assert (ct - C["tok_add"]) % C["tok_mul"] == 0 and 0 <= k < C["tok_div"], (ct, k)
    return (ct - C["tok_add"]) // C["tok_mul"] * C["tok_div"] + k


# ---- inputs ---------------------------------------------------------------------------------------------------------

def filler(n, seed):
    """n bytes in which no 4-gram occurs twice: n literal tokens"""
    return encode_gen.Builder(n, np.random.default_rng(seed)).bytes() if n else b""


def planted(n, seed, plants=(), runs=()):
    """filler with repeats (dst, length, dist) and runs (at, length) planted"""
    b = encode_gen.Builder(n, np.random.default_rng(seed))
    for dst, length, dist in plants:
        b.far_plant(dst, length, dist)          # (the filler between source and copy keeps off the source's table slot)
    for at, length in runs:
        b.run(at, length)
    return b.bytes()


Case = collections.namedtuple("Case", "name blocks stride cap want")     # want: the route of each block


# ---- test A: the capacity line in one record ------------------------------------------------------------------------

A_CAP, A_STRIDE = 1164, 1168
A_FILLER = (1001, 1002, 1003, 1064, 1065, 1066)
# what the issue expects of each filler block at cap_tok 1001: the route, and the kind and size of the pass that overflows
# (a block of 1024 bytes and more has a 16th full pass, 960 + 64 > 1001: only 1002 .. 1023 bytes overflow on the short last pass)
A_EXPECT = {1001: ("split", None, None), 1002: ("fused", "end", 42), 1003: ("fused", "end", 43), 1064: ("fused", "full", 64),
            1065: ("fused", "full", 64), 1066: ("fused", "full", 64)}


def case_a():
    blocks = collections.OrderedDict()
    for i, n in enumerate(A_FILLER):
        blocks["filler_%d" % n] = filler(n, 100 + i)
    blocks["empty"] = b""
    blocks["filler_63"] = filler(63, 110)
    # repeats of 4, 16 and 258 take 3 + 15 + 257 = 275 tokens off.  No block of the room's 1164 bytes holds all three and
    # still has more than 1001 tokens, so the overflowing one is there twice: with the repeats of 4 and 16 alone (1160
    # bytes, 1142 tokens), and with all three in 1290 bytes (1015 tokens) -- longer than the room, the fused kernel's by
    # the n > split_max rule before any token is counted, and its member (about 800 bytes) fits
    pl = ((200, 4, 100), (400, 16, 150), (700, 258, 300))
    blocks["planted_fits"] = planted(1160, 111, pl)
    blocks["planted_overflows"] = planted(1160, 112, pl[:2])
    blocks["planted_long"] = planted(1290, 113, pl)
    want = {"empty": "split", "filler_63": "split", "planted_fits": "split", "planted_overflows": "fused", "planted_long": "fused"}
    want.update({"filler_%d" % n: A_EXPECT[n][0] for n in A_FILLER})
    return Case("A", blocks, A_STRIDE, A_CAP, want)


# ---- test B: overflow around a DEFLATE block close ------------------------------------------------------------------

B_FILLER = (32768, 32769, 32832, 32833, 33000, 65536, 65537, 65601)
B_PLANTED = (("planted4", 32968, 4), ("planted5", 32968, 5))     # one repeat of 4 / 5 bytes at 5000, 300 back


_B_INPUT = {}


def b_input(name, extra=0):
    """the input `name` of test B, `extra` bytes longer"""
    if (name, extra) not in _B_INPUT:
        if name.startswith("filler_"):
            d = filler(int(name[7:]) + extra, 200 + int(name[7:]) % 97)
        else:
            n, L = {k: (n, L) for k, n, L in B_PLANTED}[name]
            d = planted(n + extra, 300 + L, ((5000, L, 300),))
        _B_INPUT[(name, extra)] = d
    return _B_INPUT[(name, extra)]


B_INPUTS = tuple("filler_%d" % n for n in B_FILLER) + tuple(k for k, _, _ in B_PLANTED)

BCase = collections.namedtuple("BCase", "name input extra data cap_tok stride cap want target exact")


_B = None


def _close_count(p, n):
    """tokens stored when the close that matters is done: the first one -- or, in a block of 64 KiB and more, all that
    close in front of the tail (a record of the first DEFLATE block's 32768 tokens belongs to a room of 43520 bytes,
    less than the block: the n > split_max rule would decide, and the member would not fit); None: no such close"""
    cl = p.closes[:-1]
    if n >= 65536:
        cl = [sum(cl)] if len(cl) > 1 else []
    return cl[0] if cl else None


def _exact(p, n, target):
    if target.startswith("whole"):
        e = p.total
    else:
        e = _close_count(p, n)
    return None if e is None else e - (1 if target.endswith("-1") else 0)


def cases_b():
    """(input x {close, close-1, whole, whole-1}): rooms whose cap_tok is the tokens stored at the close / of the whole
    member, or one less; and every input once in a room of 0.76 n < n.  cap_tok is always 2 mod 3.  Another residue is
    reached with the input one or two bytes longer ('+1', '+2' in the name) where that moves the count, else by the
    nearest cap_tok ('~' in the name, at most two tokens off) at which the same pass of the same parse overflows as at
    the exact count -- test_l2_handover.py checks that it is the same pass.  Cases that come out as the same
    (input, length, cap_tok) are planned once; filler of exactly 65536 bytes has no close in front of its tail."""
    global _B
    if _B is not None:
        return _B
    out, seen = [], set()
    k = 0
    for name in B_INPUTS:
        for target in ("close", "close-1", "whole", "whole-1"):
            found = None
            for off in (0, 1, -1, 2, -2):                          # exact first, then the nearest
                for extra in (0, 1, 2):
                    data = b_input(name, extra)
                    p = block_passes(data)
                    e = _exact(p, len(data), target)
                    if e is None or (e + off) % 3 != 2:
                        continue
                    if overflow_pass(p.counts, e + off) == overflow_pass(p.counts, e):
                        found = (extra, data, p, e + off, e)
                        break
                if found:
                    break
            if not found:
                continue
            extra, data, p, ct, e = found
            if (name, extra, ct) in seen:
                continue
            seen.add((name, extra, ct))
            cap = cap_for(ct, k % 4)
            k += 1
            out.append(BCase("%s%s/%s%s=%d" % (name, "+%d" % extra if extra else "", "~" if ct != e else "", target, ct), name, extra,
                             data, ct, up16(cap) + 16 * (k % 3), cap, route(len(data), p.counts, cap), target, e))
    for name in B_INPUTS:
        data = b_input(name)
        cap = len(data) * 76 // 100
        out.append(BCase("%s/room<n" % name, name, 0, data, cap_tok(cap), up16(cap), cap, "fused", "size", None))
    _B = out
    return out


# ---- test C: the planted-edge corpus through both codecs ------------------------------------------------------------

C_SPLIT_ROOM = ec.SEG_LIMIT                       # the largest split_max of the split path
C_FUSED_ROOM = ec.SEG_LIMIT + 16                  # one stride step on: split_sub_batch returns 0
C_LAUNCH = 64


def blocks_c():
    blocks = collections.OrderedDict((c.name, c.data) for c in encode_gen.cached_corpus() if c.family != "seg")
    s = hdtest.synth()
    blocks["text_%d" % ec.SEG_LIMIT] = bytes(s.text_like(ec.SEG_LIMIT, seed=41))
    blocks["fastq_%d" % ec.SEG_LIMIT] = bytes(s.fastq_like(ec.SEG_LIMIT, seed=42))
    return blocks


# ---- test D: the fused kernel's grid stride -------------------------------------------------------------------------

D_CAP = 1008
D_BLOCKS = 2 * 2560 + 40
D_POOL_OVER, D_POOL_FIT = 331, 167               # primes: 2560 is a multiple of neither, so b, b + 2560, b + 5120 differ


D_TINY = (3, 2560 + 17, 5120 + 29)               # with their wavefronts' other two blocks: all three kinds in every order


def kind_d(i):
    """'over' | 'fit' | 'tiny': the kind moves by one along a wavefront's blocks i, i + 2560, i + 5120"""
    if i in D_TINY or i % 211 == 100:
        return "tiny"
    return ("over", "over", "fit")[(i + i // FUSED_SLOTS) % 3]


_D = None


def blocks_d():
    """-> (data of each block, kind of each block)"""
    global _D
    if _D is None:
        s = hdtest.synth()
        fq = bytes(s.fastq_like(D_POOL_FIT * 1000, seed=51))
        ph = hdtest.corpus_phrases(52, 24)
        over, fit = [], []
        for j in range(D_POOL_OVER):
            n = 990 + j % 17                                       # 990 .. 1006 bytes
            pl = ((300 + j % 40, 4 + j % 9, 50 + j % 200),) if j % 2 else ()
            runs = ((600 + j % 50, 3 + j % 30),) if j % 3 == 0 else ()
            over.append(planted(n, 1000 + j, pl, runs))
        for j in range(D_POOL_FIT):
            if j % 4 == 3:
                fit.append(ph[j % len(ph)][(j * 37) % 100:][:900 + j % 100])
            else:
                fit.append(fq[j * 1000 + j % 13:(j + 1) * 1000])
        data, kinds = [], []
        for i in range(D_BLOCKS):
            k = kind_d(i)
            kinds.append(k)
            data.append(over[i % D_POOL_OVER] if k == "over" else fit[i % D_POOL_FIT] if k == "fit" else
                        (b"", b"Q", b"z")[(i // 211) % 3])
        _D = (data, kinds)
    return _D


# ---- test E: hand-over across launch pairs --------------------------------------------------------------------------

E_BLOCKS, E_BYTES, E_ROOM = 66000, 1000, 1024
E_OVER = (0, 2559, 2560, 64511, 64512, 64513, 65535, 65536, 65999)


def e_filler(i):
    return filler(E_BYTES, 7000 + i)


_E = None


def data_e():
    """the launch's input, E_BLOCKS x E_BYTES back to back: FASTQ-like, filler at E_OVER"""
    global _E
    if _E is None:
        a = np.array(hdtest.synth().fastq_like(E_BLOCKS * E_BYTES, seed=61)[:E_BLOCKS * E_BYTES], dtype=np.uint8)
        for i in E_OVER:
            a[i * E_BYTES:(i + 1) * E_BYTES] = np.frombuffer(e_filler(i), dtype=np.uint8)
        _E = a.tobytes()
    return _E


def block_e(i):
    return data_e()[i * E_BYTES:(i + 1) * E_BYTES]


def e_checked():
    """the blocks compared with the twin: the overflowing ones, their neighbours, every 173rd"""
    s = set(range(0, E_BLOCKS, 173))
    for i in E_OVER:
        s |= {j for j in (i - 1, i, i + 1) if 0 <= j < E_BLOCKS}
    return sorted(s)
