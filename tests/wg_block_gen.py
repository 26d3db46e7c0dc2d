"""Seeded blocks of at most 64 KiB for the PER-BLOCK schedule of levels 3..9 (plain Python and numpy).

The per-block schedule (HD_FRAME_LATENCY, no block longer than 64 KiB: hd_deflate_wg.hpp k_stage_in, k_parse_wg shared by
4 or 2 workgroups, hd_emit_wg.hpp k_emit_wg) writes the throughput form's bytes.  What can go wrong in it depends on a
block's PIECES (1 KiB, HD_WG_CUT), on where its matches have their sources, and on how many DEFLATE blocks its member has.
`corpus()` returns `Input`s -- name, family, data -- in these families:

  sizes      text-like blocks of SIZES bytes: 0, 1, 2, ... 9, 15, 16, 17, 32, 33, 63 and 64 pieces (PIECE_COUNTS), so that
             the shares of SP = 2 and SP = 4 workgroups, [npieces * q / SP, npieces * (q + 1) / SP), take every rounding,
             sharers without a piece included, and the last positions of a block against HD_LAZY_KEY_BYTES = 6;
  borders    blocks of 64, 33, 17 and 9 pieces made of a stretch of text-like bytes repeated with sparse mutations:
             matches at distances around 4096, 16384, 32767 and 32768 that start in one share and have their source in
             an earlier one, which the sharer only REPLAYED; `far_32769`, whose only copy lies 32769 bytes back (no match
             at all: its filler has no 4-gram twice); two FASTQ-like blocks;
  cuts       members of 4 .. 10 DEFLATE blocks: independent random bytes of two (or four) kinds in turn, stretches of
             1024 .. 7168 bytes, 65536 bytes in all.  k_emit_wg builds the codes of EW_SLOTS = 4 DEFLATE blocks side by
             side and takes another path from the fifth on, and once more from the ninth;
  fallbacks  noise (stored by verdict), a many-block input with a noise tail, zeros, Fibonacci literal frequencies.

What the twin makes of them -- the DEFLATE block counts of `cuts`, the matches across share borders of `borders` -- is
pinned by tests/test_wg_block_gen.py.

Members of NINE or more DEFLATE blocks (a third round of k_emit_wg): the split rule (hd_emit_wg.hpp, the twin's
wg_split_check) looks at a block at a piece boundary once it is HD_WG_SPLIT_MIN = 5000 bytes long and has
HD_WG_SPLIT_OBS = 512 new tokens, and the first look only takes note.  The shortest block is therefore five pieces of one
kind and a sixth whose tokens -- 512 of them at least -- are of another: `cut10`, 5120 bytes of 00 / ff (matches) and
1024 random digits (literals) in turn, gives ten blocks at levels 3..6.  Even schedules of two to four kinds every
2048 .. 7168 bytes (about 290 were measured with the twin) stop at 8: the piece behind a change of kind goes to the
block in front, and the next block then needs two looks.
"""
import collections

import numpy as np

import encode_gen
import hdtest

MAX_BLOCK = 65536
PIECE = 1024                                          # HD_WG_CUT (include/hipdeflate_params.h)
SIZES = [0, 1, 5, 6, 7, 1023, 1024, 1025, 1029, 1030, 2047, 2048, 2049, 3072, 4096, 4097, 5119, 5120, 5121, 6144, 7168, 8192, 9216,
         15360, 16384, 17408, 32767, 32768, 32769, 64511, 64512, 64513, 65279, 65280, 65530, 65531, 65535, 65536]
# (5121 and 6144 are there for the six pieces that the lengths around them leave out)
PIECE_COUNTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64]

Input = collections.namedtuple("Input", "name family data")


def npieces(n):
    return (n + PIECE - 1) // PIECE


def share_borders(n, sp):
    """first bytes of the shares of workgroups 1 .. sp - 1 (hd_deflate_wg.hpp pfirst), those at byte 0 left out"""
    return [b for b in (PIECE * (npieces(n) * q // sp) for q in range(1, sp)) if b]


# ---- the kinds of bytes ----------------------------------------------------------------------------------------------

def _pick(rng, alphabet, n):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)]


def _kind(rng, kind, n, text):
    if kind == "digits":
        return _pick(rng, b"0123456789", n)
    if kind == "acgt":
        return _pick(rng, b"ACGT", n)
    if kind == "00ff":
        return _pick(rng, b"\x00\xff", n)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    assert kind == "text"
    o = int(rng.integers(0, len(text) - n))
    return text[o:o + n]


def _text(rng, n=200000):
    return np.asarray(hdtest.synth().text_like(n, seed=int(rng.integers(1, 1 << 30))), dtype=np.uint8)


# ---- families --------------------------------------------------------------------------------------------------------

def fam_sizes(rng):
    text = _text(rng)
    out = []
    for k, n in enumerate(SIZES):
        o = (k * 4999) % (len(text) - MAX_BLOCK)          # (no two blocks the same bytes)
        out.append(Input("size_%d" % n, "sizes", text[o:o + n].tobytes()))
    return out


def _repeated(rng, text, n, period, every):
    """n bytes: a stretch of `period` text-like bytes, then copies of it, each copy the one before with a byte changed
    every ~`every` bytes -- matches at distance `period`, cut short at the mutations"""
    o = int(rng.integers(0, len(text) - period))
    cur = text[o:o + period].copy()
    parts, have = [], 0
    while have < n:
        parts.append(cur)
        have += period
        cur = cur.copy()
        p = int(rng.integers(every // 2, every))
        while p < period:
            cur[p] = (int(cur[p]) + 1 + int(rng.integers(0, 255))) & 0xff
            p += int(rng.integers(every // 2, every + every // 2))
    return np.concatenate(parts)[:n].tobytes()


# (name, bytes, period, a mutation every ~this many bytes)
BORDER_BLOCKS = [
    ("b64_d4096", 65536, 4096, 90), ("b64_d16384", 65536, 16384, 90), ("b64_d32767", 65536, 32767, 90),
    ("b64_d32768", 65536, 32768, 90), ("b64_d32768_ragged", 65536 - 321, 32768, 120),
    ("b33_d4096", 33 * 1024 - 77, 4096, 90), ("b33_d16384", 33 * 1024, 16384, 60),
    ("b17_d4096", 17 * 1024, 4096, 60), ("b17_d16384", 17 * 1024, 16384, 40),
    ("b9_d4096", 9 * 1024, 4096, 60), ("b9_d4096_ragged", 9 * 1024 - 3, 4096, 40),
]


def fam_borders(rng):
    text = _text(rng)
    out = [Input(name, "borders", _repeated(rng, text, n, period, every)) for name, n, period, every in BORDER_BLOCKS]
    # the only copy of anything lies 32769 bytes back: one byte beyond the window
    a = encode_gen.Builder(32769, rng).bytes()
    out.append(Input("far_32769", "borders", a + a[:MAX_BLOCK - 32769]))
    fq = hdtest.synth().fastq_like(MAX_BLOCK, seed=int(rng.integers(1, 1 << 30)))
    out.append(Input("fastq_65280", "borders", bytes(fq[:65280])))
    out.append(Input("fastq_65536", "borders", bytes(fq[:65536])))
    return out


# (name, the kinds in turn, the lengths of the stretches in turn, the length of the first stretch if it differs)
CUT_SCHEDULES = [
    ("cut7", ("digits", "00ff"), (5120,), None),
    ("cut6", ("acgt", "digits"), (5120,), None),
    ("cut5", ("acgt", "digits"), (6144,), None),
    ("cut4", ("text", "digits", "acgt", "noise"), (5120,), None),
    ("cut8", ("digits", "acgt"), (4096,), None),
    ("cut8_l3", ("digits", "acgt"), (7168,), 5120),
    ("cut10", ("00ff", "digits"), (5120, 1024), None),
]


def _alternating(rng, text, kinds, lens, first=None, n=MAX_BLOCK):
    parts, have, k = [], 0, 0
    while have < n:
        m = min(first if first and not parts else lens[k % len(lens)], n - have)
        parts.append(_kind(rng, kinds[k % len(kinds)], m, text))
        have += m
        k += 1
    return np.concatenate(parts)


def fam_cuts(rng):
    text = _text(rng)
    return [Input(name, "cuts", _alternating(rng, text, kinds, lens, first).tobytes())
            for name, kinds, lens, first in CUT_SCHEDULES]


def fam_fallbacks(rng):
    text = _text(rng)
    out = [Input("noise_%d" % n, "fallbacks", rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in (65536, 65535, 1024)]
    a = _alternating(rng, text, ("digits", "00ff"), (5120,)).copy()
    a[40960:] = rng.integers(0, 256, MAX_BLOCK - 40960, dtype=np.uint8)
    out.append(Input("cut7_noise_tail", "fallbacks", a.tobytes()))
    out.append(Input("zeros_65536", "fallbacks", bytes(MAX_BLOCK)))
    out.append(Input("fib_lits", "fallbacks", hdtest.corpus_small()["fib_lits"]))
    return out


def corpus(seed=2031):
    rng = np.random.default_rng(seed)
    out = []
    for fam in (fam_sizes, fam_borders, fam_cuts, fam_fallbacks):
        out += fam(np.random.default_rng(int(rng.integers(0, 1 << 31))))
    assert all(len(c.data) <= MAX_BLOCK for c in out) and len({c.name for c in out}) == len(out)
    return out


_cached = None


def cached_corpus():
    global _cached
    if _cached is None:
        _cached = corpus()
    return _cached
