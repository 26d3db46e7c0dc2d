"""tests/pipe_model.py against a brute-force restatement of the same sentences of include/hipdeflate.h: the block
table byte by byte, the slot rule slot by slot.  CPU only."""
import numpy as np
import pytest

import pipe_model as pm


def brute_blocks(B, nbytes):
    """byte k of a batch belongs to block k // B"""
    owner = [k // B for k in range(nbytes)]
    out = []
    for k, b in enumerate(owner):
        if b == len(out):
            out.append([k, 0])
        out[b][1] += 1
    return [tuple(x) for x in out]


class BruteSlots:
    """`depth` slots in a ring, each FREE, FILLING, PENDING or HELD; input() needs the next slot of the ring FREE"""
    FREE, FILLING, PENDING, HELD = range(4)

    def __init__(self, depth):
        self.st = [self.FREE] * depth
        self.n_in = self.n_out = 0

    def can_input(self):
        return self.st[self.n_in % len(self.st)] == self.FREE

    def input(self):
        self.st[self.n_in % len(self.st)] = self.FILLING

    def submit(self):
        k = self.n_in % len(self.st)
        if self.st[k] != self.FILLING:
            return pm.E_ARG
        self.st[k] = self.PENDING
        self.n_in += 1
        return 0

    def result(self):
        self.st = [self.FREE if s == self.HELD else s for s in self.st]
        k = self.n_out % len(self.st)
        if self.st[k] != self.PENDING:
            return pm.E_ARG
        self.st[k] = self.HELD
        self.n_out += 1
        return 0


def test_block_table_matches_brute_force_on_random_submit_sequences():
    rng = np.random.default_rng(7)
    for _ in range(300):
        B = int(rng.choice([16, 32, 48, 64, 80]))
        P = int(rng.integers(1, 6))
        sizes = [int(x) for x in rng.integers(0, P * B + 1, int(rng.integers(1, 12)))]
        tbl = pm.block_table(B, sizes)
        assert len(tbl) == len(sizes)
        for n, blocks in zip(sizes, tbl):
            assert blocks == brute_blocks(B, n)
            assert len(blocks) <= P and sum(ln for _, ln in blocks) == n


def test_block_table_by_hand():
    assert pm.batch_blocks(16, 0) == []
    assert pm.batch_blocks(16, 1) == [(0, 1)]
    assert pm.batch_blocks(16, 15) == [(0, 15)]
    assert pm.batch_blocks(16, 16) == [(0, 16)]
    assert pm.batch_blocks(16, 17) == [(0, 16), (16, 1)]
    assert pm.batch_blocks(16, 47) == [(0, 16), (16, 16), (32, 15)]
    assert pm.batch_blocks(16, 48) == [(0, 16), (16, 16), (32, 16)]
    assert pm.batch_blocks(0xff00, 0xff00 + 1) == [(0, 0xff00), (0xff00, 1)]


def test_expected_run_by_hand():
    assert pm.expected_run([]) == (b"", [], [])
    assert pm.expected_run([b"abc", b"", b"de"]) == (b"abcde", [3, 0, 2], [0, 3, 3])
    runs = pm.expected_runs([[b"x"], [], [b"yy", b"z"]])
    assert [r[0] for r in runs] == [b"x", b"", b"yyz"] and runs[2][2] == [0, 2]


def test_slot_rule_matches_brute_force_on_random_call_sequences():
    rng = np.random.default_rng(11)
    for _ in range(400):
        depth = int(rng.integers(2, 7))
        m, b = pm.Slots(depth), BruteSlots(depth)
        for _ in range(int(rng.integers(5, 80))):
            op = int(rng.integers(0, 3))
            if op == 0:
                assert m.can_input() == (b.can_input() and not m.filling), (depth, m.__dict__, b.st)
                if m.can_input():
                    m.input()
                    b.input()
            elif op == 1:
                assert m.submit() == b.submit()
            else:
                assert m.result() == b.result()
            assert m.pending == b.st.count(b.PENDING) and m.held == (b.HELD in b.st)
            assert 0 <= m.pending + m.held + m.filling <= depth


def test_slot_rule_by_hand():
    s = pm.Slots(2)
    assert s.result() == pm.E_ARG and s.submit() == pm.E_ARG
    s.input()
    assert not s.can_input()                 # input() twice
    assert s.submit() == 0 and s.can_input()
    s.input()
    assert s.submit() == 0 and not s.can_input()      # both slots pending
    assert s.result() == 0 and not s.can_input()      # one pending, one held
    assert s.result() == 0 and s.can_input()          # the first went back, one held
    assert s.result() == pm.E_ARG and not s.held      # a call that finds nothing still releases
    with pytest.raises(AssertionError):
        t = pm.Slots(2)
        t.input(), t.submit(), t.input(), t.submit(), t.input()


def test_schedules_by_hand_and_within_the_rule():
    assert pm.schedule("eager", 3, 2) == "SRSRSR"
    assert pm.schedule("lagged", 4, 3) == "SSRSRSRR"
    assert pm.schedule("lagged", 1, 4) == "SR"
    assert pm.schedule("fill_drain", 5, 2) == "SSRRSRSRSR"
    assert pm.schedule("fill_drain", 8, 3) == "SSSRRRSSRRSSRRSR"
    for order in pm.FETCH_ORDERS:
        for depth in (2, 3, 4, 16):
            for n in (0, 1, 2, 5, 48):
                ops = pm.schedule(order, n, depth)      # (schedule() asserts the rule at every 'S')
                assert ops.count("S") == ops.count("R") == n
    assert "S" * 4 in pm.schedule("fill_drain", 48, 4)  # all `depth` slots before the first fetch


def test_patterns_by_hand():
    B, P = 64, 3
    assert pm.pat_edges(B, P) == [0, 1, 63, 64, 65, 191, 192, 0, 0, 17]
    assert pm.pat_edges_reversed(B, P) == [17, 0, 0, 192, 191, 65, 64, 63, 1, 0]
    assert pm.pat_edges(B, 1) == [0, 1, 63, 64, 64, 63, 64, 0, 0, 17]
    z = pm.pat_zero_runs(B, P)
    assert z[:3] == [0, 0, 0] and z[-4:] == [0, 0, 0, 0] and any(z)
    f = pm.pat_full_ragged_tail(B, P)
    assert f[:-1] == [192] * 3 and 0 < f[-1] < 192 and f[-1] % B
    r = pm.pat_random(B, P)
    assert len(r) >= 40 and r == pm.pat_random(B, P) and 0 in r and P * B in r
    for B, P in ((64, 3), (0xff00, 3), (65536, 2), (4096, 4), (8192, 3)):
        pats = pm.patterns(B, P)
        assert set(pats) == {"full_ragged_tail", "edges", "edges_reversed", "zero_runs", "p1", "random"}
        assert pats["p1"][0] == 1
        for name, (p, sizes) in pats.items():
            assert all(0 <= n <= p * B for n in sizes), name
            assert all(len(blocks) <= p for blocks in pm.block_table(B, sizes)), name
