"""What keeps test_gpu_l2_handover.py honest (CPU): the arithmetic of l2_handover.py is the sources', its replay of the
parse's passes gives the twin's own DEFLATE blocks, and every planned case sits on the side of level 2's hand-over it was
planned for, in a room that holds the twin's member.  The numbers of cases are pinned: none is skipped or filtered."""
import collections

import encode_contracts as ec
import encode_room as er
import l2_handover as h


def _fits(data, frame, stride, cap):
    """the twin's member of the block in that frame fits the launch's room"""
    return h.model(data, frame == er.RAW_FLUSH).choose(er.payload_room(frame, stride, cap)).fits


def test_constants_read_from_the_sources():
    assert h.C["tok_div"] == 4 and h.C["tok_mul"] == 3 and h.C["tok_add"] == 128
    assert h.cap_tok(1164) == 1001 and h.cap_tok(43520) == 32768
    assert h.cap_tok(1167) == 1001 and h.cap_tok(1168) == 1004                  # 3 tokens per 4 bytes of room
    assert {h.cap_tok(c) % 3 for c in range(1000, 1100)} == {2}
    assert all(h.cap_tok(h.cap_for(ct, k)) == ct for ct in (1001, 32768, 65537) for k in range(4))
    assert h.FUSED_SLOTS == 2560 and h.fused_grid(5160) == 2560 and h.fused_grid(7) == 7
    assert h.C["parse_slots"] == 4608 and h.C["sub_max"] == 65536
    assert h.SPLIT_ROOM_MAX == 327680 == ec.SEG_LIMIT
    # a launch pair: whole rounds of the resident parse wavefronts below the 65536-block cap
    assert h.sub_batch(66000, 1024) == 64512 == 14 * 4608
    assert h.sub_batch(70000, 2048) == 64512                                    # (test_encode_many_small_blocks_across_sub_batches)
    assert h.sub_batch(64, 327680) == 64 and h.sub_batch(64, 327696) == 0
    assert h.sub_batch(5160, 1008) == 5160
    assert h.BLOCK_TOKENS == 32768 and h.STEP == 64
    assert h.overflow_check_in_source(), "emit_tokens' overflow check no longer reads `ntok_slab + count > lay.cap_tok`"


def test_route():
    assert h.route(1000, [64] * 15 + [41], 1164) == "split"                     # 1001 tokens: the last slab entry
    assert h.route(1000, [64] * 15 + [42], 1164) == "fused"
    assert h.route(1165, [10], 1164) == "fused"                                 # n > split_max
    assert h.route(10, [10], 327696) == "fused"                                 # no split path in the launch
    assert h.overflow_pass([64] * 16, 1001) == 15 and h.overflow_pass([64] * 15 + [41], 1001) is None


def test_passes_replay_the_twins_deflate_blocks():
    """filler of n bytes is n literals, and the replay's closes are the DEFLATE blocks the twin wrote (the issue's table)"""
    table = {"filler_32768": [32768], "filler_32769": [32768, 1], "filler_32832": [32768, 64], "filler_32833": [32768, 65],
             "filler_33000": [32768, 232], "filler_65536": [32768, 32768], "filler_65537": [32768, 32768, 1],
             "filler_65601": [32768, 32768, 65], "planted4": [32829, 136], "planted5": [32828, 136]}
    assert set(table) == set(h.B_INPUTS)
    for name in h.B_INPUTS:
        d = h.b_input(name)
        p = h.block_passes(d)
        assert p.closes == h.tokens(d)[1] == table[name], name
        if name.startswith("filler_"):
            assert p.total == len(d)
            assert set(p.kinds[:-1]) <= {"full"}                                # a close of filler has nothing queued
    for name, queued in (("planted4", 61), ("planted5", 60)):
        p = h.block_passes(h.b_input(name))
        k = p.kinds.index("close")
        assert p.counts[k] == queued and sum(p.counts[:k + 1]) == p.closes[0]
    blocks = list(h.case_a().blocks.values()) + [c.data for c in h.cases_b()] + list(dict.fromkeys(h.blocks_d()[0]))
    for d in blocks:
        assert h.block_passes(d).closes == h.tokens(d)[1], len(d)


def test_case_a_sits_on_the_capacity_line():
    a = h.case_a()
    ct = h.cap_tok(min(a.stride, a.cap))
    assert ct == 1001 and a.stride % 16 == 0 and a.stride >= a.cap
    assert len(a.blocks) == 11 and set(a.want) == set(a.blocks)
    over = []
    for n in h.A_FILLER:
        d = a.blocks["filler_%d" % n]
        p = h.block_passes(d)
        assert p.total == n == len(d)
        over.append(p.total - ct)
        k = h.overflow_pass(p.counts, ct)
        want, kind, count = h.A_EXPECT[n]
        assert (None, None) == (kind, count) if k is None else (p.kinds[k], p.counts[k]) == (kind, count), n
    assert over == [0, 1, 2, 63, 64, 65]
    for name, d in a.blocks.items():
        p = h.block_passes(d)
        assert h.route(len(d), p.counts, min(a.stride, a.cap)) == a.want[name], name
        for frame in (er.BGZF, er.RAW_FLUSH):
            assert _fits(d, frame, a.stride, a.cap), (name, frame)
    # the planted blocks: repeats of 4, 16 and 258 found as planted; one fits, one overflows, one is longer than the room
    assert h.block_passes(a.blocks["planted_fits"]).total == 1160 - 275 <= ct
    assert h.block_passes(a.blocks["planted_overflows"]).total == 1160 - 18 > ct
    assert h.block_passes(a.blocks["planted_long"]).total == 1290 - 275 > ct and len(a.blocks["planted_long"]) > a.cap
    m = h.tokens(a.blocks["planted_fits"])
    assert len(m[0]) == 885


def test_cases_b_sit_around_a_close():
    cs = h.cases_b()
    assert len(cs) == 46 and len({c.name for c in cs}) == 46
    assert collections.Counter(c.target for c in cs) == {"close": 10, "close-1": 10, "whole": 10, "whole-1": 6, "size": 10}
    where = collections.Counter()
    for c in cs:
        n, room = len(c.data), min(c.stride, c.cap)
        p = h.block_passes(c.data)
        assert c.stride % 16 == 0 and c.stride >= c.cap and h.cap_tok(room) == c.cap_tok, c.name
        assert h.route(n, p.counts, room) == c.want, c.name
        for frame in (er.RAW, er.RAW_FLUSH):
            assert _fits(c.data, frame, c.stride, c.cap), (c.name, frame)
        if c.target == "size":
            assert n > room and c.want == "fused"
            continue
        assert n <= room, c.name                                                 # the record's capacity decides, not the size
        k = h.overflow_pass(p.counts, c.cap_tok)
        assert abs(c.cap_tok - c.exact) <= 2 and k == h.overflow_pass(p.counts, c.exact), c.name
        assert (k is None) == (c.want == "split") == (c.target == "whole"), c.name
        if k is None:
            assert p.total == c.cap_tok                                          # the last slab entry
            where["fits"] += 1
            continue
        stored = sum(p.counts[:k])
        behind_close = any(stored == sum(p.closes[:j]) for j in range(1, len(p.closes)))
        where[(p.kinds[k], "behind a close" if behind_close else "")] += 1
        if c.target == "close":
            assert behind_close and stored <= c.cap_tok, c.name                  # the DEFLATE block fits, the next pass does not
        elif c.target == "close-1":
            assert not behind_close and stored + p.counts[k] in [sum(p.closes[:j]) for j in range(1, len(p.closes))], c.name
        else:
            assert p.total - c.cap_tok == 1, c.name
    print(dict(where))
    # the overflow inside step_boundary's own pass, on a full and on the short last pass right behind a close
    assert where[("close", "")] == 2 and where[("full", "behind a close")] >= 5 and where[("end", "behind a close")] >= 3
    assert where["fits"] == 10


def test_blocks_c_take_both_codecs():
    bl = h.blocks_c()
    assert len(bl) == 56 and not any(k.startswith("seg_") for k in bl)
    assert {"window_ring_edge", "runs_cut", "all_literals_70000", "random_ff00", "size_0", "size_65537"} <= set(bl)
    assert sorted(len(d) for d in bl.values())[-2:] == [ec.SEG_LIMIT, ec.SEG_LIMIT]
    assert len(bl) <= h.C_LAUNCH
    assert h.sub_batch(len(bl), h.C_SPLIT_ROOM) == len(bl) and h.sub_batch(len(bl), h.C_FUSED_ROOM) == 0
    assert h.C_SPLIT_ROOM == h.SPLIT_ROOM_MAX and h.C_FUSED_ROOM == h.SPLIT_ROOM_MAX + 16 and h.cap_tok(h.C_SPLIT_ROOM) == 245888
    for name, d in bl.items():
        # at most a token per byte: only the two longest blocks can come near the record's capacity
        assert len(d) <= h.cap_tok(h.C_SPLIT_ROOM) or h.block_passes(d).total <= h.cap_tok(h.C_SPLIT_ROOM), name
        assert h.route(len(d), [], h.C_FUSED_ROOM) == "fused"
        for frame in (er.RAW, er.RAW_FLUSH):
            assert _fits(d, frame, h.C_SPLIT_ROOM, h.C_SPLIT_ROOM), (name, frame)


def test_blocks_d_walk_the_fused_grid():
    data, kinds = h.blocks_d()
    assert len(data) == h.D_BLOCKS == 5160 and h.fused_grid(len(data)) == 2560
    assert h.sub_batch(len(data), h.D_CAP) == len(data) and h.cap_tok(h.D_CAP) == 884
    cnt = collections.Counter(kinds)
    assert cnt == {"over": 3421, "fit": 1712, "tiny": 27}
    for d, k in dict(zip(data, kinds)).items():
        p = h.block_passes(d)
        assert h.route(len(d), p.counts, h.D_CAP) == ("fused" if k == "over" else "split"), (k, len(d), p.total)
        assert (k != "over" or p.total >= 900) and (k != "tiny" or len(d) <= 1)
        assert _fits(d, er.RAW, h.up16(h.D_CAP), h.D_CAP), (k, len(d))
    # a persistent wavefront's successive blocks differ; 40 wavefronts take three, some of them one of each kind
    grid = h.fused_grid(len(data))
    orders = set()
    for w in range(grid):
        mine = list(range(w, len(data), grid))
        assert len(mine) == (3 if w < 40 else 2)
        assert len({data[i] for i in mine}) == len(mine)
        if len(mine) == 3 and len({kinds[i] for i in mine}) == 3:
            orders.add(tuple(kinds[i] for i in mine))
        if len(mine) == 3 and "tiny" not in [kinds[i] for i in mine]:
            assert sorted(kinds[i] for i in mine) == ["fit", "over", "over"] and len({len(data[i]) for i in mine}) > 1
    assert len(orders) >= 3, orders
    # ... and the fused kernel has work in every round: overflowing blocks at b, b + 2560 and b + 5120
    assert all(any(kinds[i] == "over" for i in range(r * grid, min((r + 1) * grid, len(data)))) for r in range(3))


def test_blocks_e_straddle_the_launch_pairs():
    sub = h.sub_batch(h.E_BLOCKS, h.E_ROOM)
    assert sub == 64512 and h.E_BLOCKS == 66000 and sub < h.E_BLOCKS < 2 * sub
    assert {sub - 1, sub, sub + 1, h.FUSED_SLOTS - 1, h.FUSED_SLOTS, 0, h.E_BLOCKS - 1} <= set(h.E_OVER)
    assert sum(1 for i in h.E_OVER if i >= sub) == 5                            # record index blockIdx.x != flag index b
    assert len(h.data_e()) == h.E_BLOCKS * h.E_BYTES
    chk = h.e_checked()
    assert len(chk) == 398 and set(h.E_OVER) <= set(chk)
    ct = h.cap_tok(h.E_ROOM)
    assert ct == 896
    for i in chk:
        d = h.block_e(i)
        p = h.block_passes(d)
        want = "fused" if i in h.E_OVER else "split"
        assert h.route(len(d), p.counts, h.E_ROOM) == want, i
        assert (p.total == h.E_BYTES) == (i in h.E_OVER)
        assert _fits(d, er.RAW, h.E_ROOM, h.E_ROOM), i
