"""The inputs the preset-dictionary tests share (test_dict_model.py on the CPU, test_gpu_dict_deflate.py and
test_gpu_dict_inflate.py on the device): one master buffer per kind from 7bgzf_amd.synth, never modified.  The dictionary is
the stretch that ends at byte AT, the blocks lie behind it -- history and data of one source, as a caller's would be."""
import hdtest

AT = 64 << 10                     # where the dictionary ends and the blocks begin
MASTER = 1400 << 10
KINDS = ("text", "fastq")
ENC_LEVELS = (3, 4, 5, 6)
# dict_len: used 1024, 1024 (one byte unused), 4096 (904 unused), the whole window, the window's last 32 KiB
DICT_LENS = (1024, 1025, 5000, 32768, 40000)
# block lengths: one byte; a maximal match; one piece; a CISO sector; an odd size over four pieces; with 32 KiB of history
# the last size that fits the parse's ring whole (the table snapshot), the first that does not (replay), and the filler path
BLOCK_LENS = (1, 258, 1024, 2048, 4101, 32 << 10, 33 << 10, 64 << 10)

_data = {}


def master(kind):
    if kind not in _data:
        s = hdtest.synth()
        if kind == "text":
            _data[kind] = bytes(s.text_like(MASTER, seed=41))
        elif kind == "fastq":
            _data[kind] = bytes(s.fastq_like(MASTER, seed=42))
        else:
            _data[kind] = bytes(s.random_bytes(64 << 10, seed=43))
    return _data[kind]


def dictionary(kind, dict_len):
    assert dict_len <= AT
    return master(kind)[AT - dict_len:AT]


def blocks(kind, lens=BLOCK_LENS, gap=0):
    """-> (offsets into master(kind), lengths): the blocks one behind the other from AT, `gap` bytes between them"""
    offs, o = [], AT
    for n in lens:
        offs.append(o)
        o += n + gap
    assert o <= len(master(kind))
    return offs, list(lens)


# ---- decode: streams zlib wrote, and hand-built streams at each edge of the source logic --------------------------------------

DEC_DICT_LENS = (1, 100, 1024, 32767, 32768, 40000)
DEC_BLOCK_LENS = (10, 3000, 64 << 10)       # the scalar loop only; windows and far sources; windows across many pieces
DEC_LEVELS = (0, 1, 6, 9)


def zlib_member(data, d, level, wbits, strategy=0):
    import zlib
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy, zdict=bytes(d)) if len(d) else \
        zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(bytes(data)) + c.flush()


def replay(window, blocks):
    """the bytes deflate_gen blocks make behind `window` (the dictionary's last 32 KiB), or None where a distance reaches in
    front of it"""
    out = bytearray(window)
    for b in blocks:
        if b.kind == "stored":
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                out.append(t)
                continue
            length, dist = t[0], t[1]
            if dist > len(out):
                return None
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(window):])


def hand_cases(kind, dict_len):
    """-> [(name, raw stream, expected output or None = status 1)]: one match at each edge, as a stream's last token (the
    scalar loop) and with 300 literals behind it (the window decode)"""
    import deflate_gen as dg
    d = dictionary(kind, dict_len)
    D = min(32768, dict_len)
    text = master(kind)
    lits = lambda n, at: list(text[AT + at:AT + at + n])
    shapes = [("first_at_D", [], (258, D)), ("first_past_D", [], (258, D + 1)), ("overlap_seam", [], (258, 1)),
              ("short_at_D", [], (3, D)),
              ("far_first_byte", lits(3000, 0), (258, 3000 + D)), ("far_past", lits(3000, 0), (258, 3001 + D)),
              ("far_straddle", lits(3000, 0), (100, 3010)),
              # ... through the lane groups' pass (at most 16 bytes) and through the open far loads (17 .. 64 bytes)
              ("far_group_straddle", lits(3000, 0), (12, 3005)), ("far_group8_straddle", lits(3000, 0), (7, 3003)),
              ("far_load_straddle", lits(3000, 0), (40, 3010)),
              ("near_first_byte", lits(300, 5000), (258, 300 + D)), ("near_straddle", lits(300, 5000), (100, 310)),
              ("near_short_straddle", lits(300, 5000), (12, 305))]
    cases = []
    for name, head, match in shapes:
        # (a distance is at most 32768: behind output a large dictionary's first byte is out of reach, its furthest byte is named)
        if match[1] > 32768:
            if "past" in name:
                continue
            match = (match[0], 32768)
        for tail in (0, 300):
            blocks = [dg.Block("dynamic", tokens=head + [match] + lits(tail, 9000), final=True)]
            cases.append(("%s_tail%d" % (name, tail), dg.encode(blocks), replay(d[-D:], blocks)))
    # stored and static blocks in front of and around matches into the dictionary
    blocks = [dg.Block("stored", data=bytes(lits(700, 100))), dg.Block("static", tokens=[(20, min(700 + D, 32768)), (5, 701)] + lits(40, 300)),
              dg.Block("stored", data=b""), dg.Block("static", tokens=[(258, 760 + 25 + min(D, 7))], final=True)]
    cases.append(("stored_static", dg.encode(blocks), replay(d[-D:], blocks)))
    return cases
