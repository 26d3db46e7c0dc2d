"""Seeded encoder inputs with repeats planted at the encoder's edges (plain Python and numpy).

All filler is drawn from 64 byte values below 144 (8-bit static codes, so level 1 stays Huffman-coded) and then
REPAIRED until no 4-gram occurs twice within 64 KiB: the only matches an encoder can find are the planted ones, and
the right parse near them is known.  A planted repeat copies `length` bytes from `dist` back, and the bytes on both
sides of it are made to differ from the source's neighbours, so the repeat is exactly as long as planted.  For
far repeats the filler between source and copy is also repaired so that no position shares the source's hash
table slot (HD_HASH_SLOT at levels 1..2, HD_HASH_SLOT6 at each workgroup bucket count): the table still names the
source when the copy is parsed, so a window edge is really reached.

`corpus()` returns `Input`s -- name, family, data -- in these families:
  cut     repeats of length {3 .. 520} starting or ending at -2..+2 around 64-byte steps, HD_WG_CUT multiples,
          HD_LAT_PART_BYTES multiples, HD_LAT_SEG_BYTES(1|2) multiples (and HD_SEG_BYTES multiples in `seg`);
  window  distances 1 .. 32769 inside a block and across a latency segment / part border, and the level-1/2 ring
          edge (encode_contracts.ring_lo) and one byte beyond it;
  runs    runs of one byte, 3..1100 long, straddling cuts and borders;
  split   data whose kind flips at chosen offsets, blocks past HD_DYN_BLOCK_TOKENS tokens, incompressible blocks;
  sizes   0..8 bytes and each of 63, 64, 1024, 2048, 4080, 8160, 0xff00, 0x10000 +-1;
  seg     HD_SEG_LIMIT +-1 and one 1 MiB MiGz block, repeats around their HD_SEG_BYTES borders.
"""
import collections

import numpy as np

import encode_contracts as ec

ALPHA_LO, ALPHA_N = 0x30, 64
WINDOW_UNIQUE = 1 << 16
K1, K2, K3 = 0x9E3779, 0xC2B2AE, 0x85EBCA            # HD_HASH_K1..K3 (include/hipdeflate_params.h)
L12_ENTRIES = 1536                                    # HD_TABLE_ENTRIES(12, 11)
WG_BUCKETS = (32768, 16384, 8192)                     # HD_WG_BUCKETS(3 | 5 | 6)

LENS = [3, 4, 5, 6, 8, 15, 16, 17, 63, 64, 65, 257, 258, 259, 520]
DISTS = [1, 2, 3, 4, 8, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 32767, 32768, 32769]
RUNS = [3, 4, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, 257, 258, 259, 300, 520, 1100]

Input = collections.namedtuple("Input", "name family data")


def _grams(a):
    a = a.astype(np.uint32)
    return a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)


def _slot4(v, entries):
    v = v.astype(np.uint64)
    t = ((v & 0xffffff) * K1 + (v >> 16) * K2) & 0xffffffff
    return ((t >> 16) * entries) >> 16


def _slot6(a, entries):
    v = _grams(a)[:-2].astype(np.uint64)
    vh = (a[4:-1].astype(np.uint64) | (a[5:].astype(np.uint64) << 8))
    t = ((v & 0xffffff) * K1 + (v >> 16) * K2 + (vh & 0xffff) * K3) & 0xffffffff
    return ((t >> 16) * entries) >> 16


class Builder:
    """filler + planted repeats; `protect` marks the bytes repairs must not touch"""

    def __init__(self, n, rng):
        self.rng = rng
        self.a = (rng.integers(0, ALPHA_N, n) + ALPHA_LO).astype(np.uint8)
        self.protect = np.zeros(n, dtype=bool)
        self.far = []                                 # (src, dst) of repeats whose table slot must survive
        self._unique()

    def _fresh(self, i, avoid=()):
        while True:
            v = int(self.rng.integers(0, ALPHA_N)) + ALPHA_LO
            if v not in avoid:
                self.a[i] = v
                return

    def _touch(self, j, span):
        """change one unprotected byte of [j, j + span); False if all are protected"""
        for k in range(j, min(j + span, len(self.a))):
            if not self.protect[k]:
                self._fresh(k, (self.a[k],))
                return True
        return False

    def _unique(self):
        """no 4-gram twice within WINDOW_UNIQUE, except where both copies are protected (planted)"""
        for _ in range(50):
            if len(self.a) < 5:
                return
            g = _grams(self.a)
            order = np.argsort(g, kind="stable")
            gs = g[order]
            same = (gs[1:] == gs[:-1]) & (order[1:] - order[:-1] < WINDOW_UNIQUE)
            bad = order[1:][same]
            fixed = 0
            for j in bad:
                if self.protect[j:j + 4].all():
                    continue
                fixed += self._touch(int(j), 4)
            if not fixed:
                return

    def plant(self, dst, length, dist):
        """a repeat of exactly `length` bytes at dst copied from dst - dist (overlapping: a run of period dist)"""
        a = self.a
        src = dst - dist
        assert src >= 0 and dst + length <= len(a), (dst, length, dist)
        for k in range(length):
            a[dst + k] = a[src + k]
        self.protect[max(src, 0):src + min(length, dist)] = True
        self.protect[dst:dst + length] = True
        # the repeat is exactly as long as planted: its neighbours differ from the source's
        if dst + length < len(a) and not self.protect[dst + length]:
            self._fresh(dst + length, (a[dst + length - dist],))
            self.protect[dst + length] = True
        if src > 0 and not self.protect[dst - 1]:
            self._fresh(dst - 1, (a[src - 1],))
            self.protect[dst - 1] = True

    def run(self, at, length):
        v = int(self.rng.integers(0, ALPHA_N)) + ALPHA_LO
        self.a[at:at + length] = v
        self.protect[at:at + length] = True
        for k in (at - 1, at + length):
            if 0 <= k < len(self.a) and not self.protect[k]:
                self._fresh(k, (v,))

    def far_plant(self, dst, length, dist):
        self.plant(dst, length, dist)
        self.far.append((dst - dist, dst))

    def _clear_slots(self):
        """no position strictly between a far source and its copy shares the source's slot in any table"""
        a = self.a
        for _ in range(8):
            changed = 0
            for src, dst in self.far:
                if dst - src < 8 or src + 6 > len(a):
                    continue
                lo, hi = src + 1, dst
                g4 = _grams(a[lo:hi + 3]) if hi + 3 <= len(a) else None
                if g4 is None or not len(g4):
                    continue
                key4 = _grams(a[src:src + 4])[0]
                hit = _slot4(g4, L12_ENTRIES) == _slot4(np.array([key4]), L12_ENTRIES)[0]
                if hi + 5 <= len(a):
                    s6 = a[lo:hi + 5]
                    for b in WG_BUCKETS:
                        hit[:len(s6) - 5] |= _slot6(s6, b) == _slot6(a[src:src + 6], b)[0]
                for j in np.nonzero(hit)[0]:
                    changed += self._touch(lo + int(j), 4)
            if not changed:
                return
            self._unique()

    def bytes(self):
        self._unique()
        self._clear_slots()
        return self.a.tobytes()


def _place(b, cursor, boundary, off, anchor, length, dist, far=False):
    """plant a repeat whose start (anchor 's') or end ('e') is at boundary + off; -> the new cursor, or None"""
    dst = boundary + off if anchor == "s" else boundary + off - length
    if dst - dist < cursor or dst + length + 2 > len(b.a):
        return None
    (b.far_plant if far else b.plant)(dst, length, dist)
    return dst + length + 2


def _matrix(rng, name, period, lens, offs, n_hint, mod=None, dist_of=lambda L: None):
    """one input: a repeat of every length x offset x anchor near successive multiples of `period` (those with
    (k * period) % mod[0] == mod[1] when mod is given)"""
    jobs = [(L, o, an) for L in lens for o in offs for an in "se"]
    b = Builder(n_hint, rng)
    cursor, k = 64, 1
    done = 0
    for L, o, an in jobs:
        while True:
            bd = k * period
            k += 1
            if bd + 600 > n_hint:
                break
            if mod and (bd % mod[0]) != mod[1]:
                continue
            d = dist_of(L) or int(rng.integers(min(L, 400) + 16, 496))
            c = _place(b, cursor, bd, o, an, L, d)
            if c is not None:
                cursor = c
                done += 1
                break
    b.a, b.protect = b.a[:cursor + 64], b.protect[:cursor + 64]
    return Input(name, "cut", b.bytes()), done, len(jobs)


def fam_cut(rng):
    out = []
    offs = [-2, -1, 0, 1, 2]
    # 64-byte steps mid-piece (multiples of 64 that are not cuts), every length
    for part in range(3):
        ls = LENS[part::3]
        out.append(_matrix(rng, "step64_%d" % part, 64, ls, offs, 130 * 1024, mod=(1024, 512))[0])
    # HD_WG_CUT multiples (the even ones are HD_LAT_PART_BYTES multiples too)
    for part in range(3):
        ls = LENS[part::3]
        out.append(_matrix(rng, "cut1024_%d" % part, ec.WG_CUT, ls, offs, 52 * 1024)[0])
    # HD_LAT_PART_BYTES multiples that are not segment starts (2048, 4096, 6144 inside an 8160 segment)
    out.append(_matrix(rng, "part2048", 2048, [4, 5, 17, 258], offs, 90 * 1024)[0])
    # HD_LAT_SEG_BYTES(1) and (2) multiples; sources inside the 512-byte priming reach
    out.append(_matrix(rng, "lat4080", ec.LAT_SEG[1], [4, 5, 16, 258], [-1, 0, 1], 110 * 1024)[0])
    out.append(_matrix(rng, "lat8160", ec.LAT_SEG[2], [4, 17, 259], [-1, 0, 1], 160 * 1024)[0])
    return out


def fam_window(rng):
    out = []
    # inside a block: distances at every window edge, copies 16 bytes long
    n = 34000 + len(DISTS) * 700
    b = Builder(n, rng)
    dst = 33500
    for d in DISTS:
        b.far_plant(dst, 16, d)
        dst += 700
    out.append(Input("window_in", "window", b.bytes()))
    # across a latency border: the copy starts 0 / 5 / 40 bytes behind a multiple of 4080 or 8160 or 2048
    n = 8160 * 12
    b = Builder(n, rng)
    borders = [k * 4080 for k in range(9, 24)] + [k * 8160 + 2048 * j for k in range(5, 11) for j in (1, 2, 3)]
    borders = sorted(set(borders))
    ds = [1, 2, 4, 8, 63, 64, 65, 300, 505, 506, 507, 508, 511, 512, 513, 514, 600, 4095, 4096, 4097, 8191, 32768]
    for i, bd in enumerate(borders):
        for j, delta in enumerate((0, 5, 40)):
            d = ds[(3 * i + j) % len(ds)]
            if bd + delta - d < 64 or bd + delta + 40 > n:
                continue
            if any(abs((bd + delta) - x) < 60 for _, x in b.far):
                continue
            b.far_plant(bd + delta, 12, d)
    out.append(Input("window_border", "window", b.bytes()))
    # the level-1/2 ring edge: at each phase p of a step, distance = the farthest the ring allows, and one more
    n = 40000
    b = Builder(n, rng)
    dst = 5000
    k = 0
    while dst + 40 < n - 600:
        q = dst
        lo = ec.ring_lo(q, n, ec.L1_WIN)
        d = q - lo + (k & 1)
        b.far_plant(dst, 10, d)
        k += 1
        dst += 509 + (k * 7) % 64
    # the end of the block: the lookahead reaches past it, the ring holds everything from filled - 4096
    q = n - 24
    b.far_plant(q, 12, q - ec.ring_lo(q, n, ec.L1_WIN))
    out.append(Input("window_ring_edge", "window", b.bytes()))
    return out


def fam_runs(rng):
    out = []
    for name, period, runs, phases in (("runs_cut", ec.WG_CUT, RUNS, 3), ("runs_lat", ec.LAT_SEG[1], RUNS[1::2], 2)):
        n = 8 * 1024 + len(runs) * phases * period
        b = Builder(n, rng)
        k = 2
        for R in runs:
            for phase in (-R // 2, -1, 1 - R)[:phases]:
                at = k * period + phase
                k += 2 if R > period // 2 else 1
                if at > 0 and at + R + 2 < n:
                    b.run(at, R)
        out.append(Input(name, "runs", b.bytes()))
    return out


def _phrases(rng, n, words=40, wlen=(6, 24)):
    """compressible bytes: phrases of a small dictionary back to back"""
    dic = [(rng.integers(0, ALPHA_N, int(rng.integers(*wlen))) + ALPHA_LO).astype(np.uint8) for _ in range(words)]
    parts, have = [], 0
    while have < n:
        w = dic[int(rng.integers(0, words))]
        parts.append(w)
        have += len(w)
    return np.concatenate(parts)[:n]


def fam_split(rng):
    out = []
    # the kind flips (phrases <-> filler) at offsets around HD_WG_SPLIT_MIN and around cuts
    for flips in ([5000, 10000, 15000, 20000], [4990, 9999, 15100, 30000], [5120, 10240, 16384, 22528],
                  [3000, 6000, 12000, 18000, 25000]):
        n = flips[-1] + 8000
        b = Builder(n, rng)
        edges = [0] + flips + [n]
        for i in range(0, len(edges) - 1, 2):
            lo, hi = edges[i], edges[i + 1]
            b.a[lo:hi] = _phrases(rng, hi - lo)
            b.protect[lo:hi] = True
        out.append(Input("flip_%d" % flips[0], "split", b.bytes()))
    # past HD_DYN_BLOCK_TOKENS tokens: all literals, and all short matches
    out.append(Input("all_literals_70000", "split", Builder(70000, rng).bytes()))
    out.append(Input("short_matches", "split", _phrases(rng, 170000, words=3000, wlen=(5, 6)).tobytes()))
    out.append(Input("short_matches_4", "split", _phrases(rng, 135000, words=3000, wlen=(4, 5)).tobytes()))
    # incompressible: the stored fallback
    out.append(Input("random_20000", "split", rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()))
    out.append(Input("random_ff00", "split", rng.integers(0, 256, 0xff00, dtype=np.uint8).tobytes()))
    return out


def _sized(rng, n):
    """n bytes of filler with a repeat every ~300 bytes"""
    b = Builder(n, rng)
    p = 64
    while p + 40 < n:
        d = int(rng.integers(20, min(p, 2000) + 1))
        L = int(rng.integers(5, 30))
        if p + L + 2 < n and p - d >= 0:
            b.plant(p, L, d)
        p += int(rng.integers(150, 450))
    return b.bytes()


SIZES = [63, 64, 1024, 2048, 4080, 8160, 0xff00, 0x10000]


def fam_sizes(rng):
    ns = sorted(set(range(0, 9)) | {s + k for s in SIZES for k in (-1, 0, 1)})
    return [Input("size_%d" % n, "sizes", _sized(rng, n)) for n in ns]


def fam_seg(rng):
    """blocks past HD_SEG_LIMIT (levels 1..2 cut them into HD_SEG_BYTES segments): repeats at the segment borders"""
    out = []
    for n in (ec.SEG_LIMIT - 1, ec.SEG_LIMIT, ec.SEG_LIMIT + 1, 1 << 20):
        b = Builder(n, rng)
        p = 64
        while p + 600 < n:                                    # background repeats, so the blocks stay Huffman
            b.plant(p, 24, int(rng.integers(30, min(p, 3000) + 1)))
            p += 280
        for k in range(1, n // ec.SEG_BYTES + 1):
            bd = k * ec.SEG_BYTES
            for j, (o, an, L, d) in enumerate(((0, "s", 16, 100), (-1, "e", 258, 300), (2, "s", 5, 20))):
                dst = bd + o if an == "s" else bd + o - L
                if dst - d > 0 and dst + L + 2 < n:
                    b.protect[dst - 3:dst + L + 3] = False
                    b.plant(dst, L, d)
        out.append(Input("seg_%d" % n, "seg", b.bytes()))
    return out


def corpus(seed=2027):
    rng = np.random.default_rng(seed)
    out = []
    for fam in (fam_cut, fam_window, fam_runs, fam_split, fam_sizes, fam_seg):
        out += fam(np.random.default_rng(int(rng.integers(0, 1 << 31))))
    return out


_cached = None


def cached_corpus():
    global _cached
    if _cached is None:
        _cached = corpus()
    return _cached
