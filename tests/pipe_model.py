"""What include/hipdeflate.h promises about the streaming pipes (hipdeflate_pipe_*, hipdeflate_unpipe_*), restated in
plain Python: the block table of a submitted batch, the run a result consists of, and the slot rule that decides when
input() may be called.  Nothing here is taken from hd_api.hip; tests/test_pipe_model.py checks it against a
brute-force restatement, tests/test_gpu_pipes.py drives the real pipes by it.

The slot rule.  A pipe has `depth` slots.  input() takes a free one, submit() makes it pending, result() hands the
oldest pending one to the caller, and the slot stays with the caller -- its `data` is valid -- until the NEXT call of
result(), whatever that call answers.  So a slot is busy while it is pending or held, and a single thread may call
input() only while  pending + (1 if a result is held else 0) < depth;  otherwise input() waits for a result() that
the same thread can never make."""
import numpy as np

# ---- block table --------------------------------------------------------------------------------------------------


def batch_blocks(block_bytes, nbytes):
    """[(offset, length)] of the blocks of one batch of nbytes: blocks start at i * block_bytes, the last may be
    short, 0 bytes are 0 blocks"""
    assert block_bytes > 0 and nbytes >= 0
    nb = (nbytes + block_bytes - 1) // block_bytes
    return [(i * block_bytes, min(block_bytes, nbytes - i * block_bytes)) for i in range(nb)]


def block_table(block_bytes, sizes):
    """per submitted batch, its blocks"""
    return [batch_blocks(block_bytes, n) for n in sizes]


def expected_run(members):
    """members of one batch, in block order -> (run bytes, member sizes, exclusive offsets inside the run)"""
    sizes = [len(m) for m in members]
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += n
    return b"".join(members), sizes, offs


def expected_runs(members_per_batch):
    return [expected_run(ms) for ms in members_per_batch]


# ---- slot rule ----------------------------------------------------------------------------------------------------

E_ARG = "E_ARG"


class Slots:
    """The state of one pipe as a single thread sees it"""

    def __init__(self, depth):
        assert depth >= 2
        self.depth = depth
        self.pending = 0          # submitted, result not fetched
        self.held = False         # a fetched result is still with the caller
        self.filling = False      # input() called, submit() not yet

    def can_input(self):
        """input() returns without waiting (and not NULL)"""
        return not self.filling and self.pending + (1 if self.held else 0) < self.depth

    def input(self):
        assert self.can_input(), "input() here would wait for ever (or answer NULL)"
        self.filling = True

    def submit(self):
        if not self.filling:
            return E_ARG
        self.filling = False
        self.pending += 1
        return 0

    def result(self):
        """every call releases the held result first; E_ARG when nothing is pending"""
        self.held = False
        if not self.pending:
            return E_ARG
        self.pending -= 1
        self.held = True
        return 0


FETCH_ORDERS = ("eager", "lagged", "fill_drain")


def schedule(order, nbatches, depth):
    """The calls of one thread for nbatches batches: a string of 'S' (input + submit of the next batch) and 'R'
    (result of the oldest), every 'S' allowed by the slot rule.
      eager       one result right after each submit
      lagged      depth - 1 submits, then result and submit in turn, then the rest of the results
      fill_drain  submits until no slot is free (`depth` of them the first time, depth - 1 while a result is held),
                  then every result, and again"""
    s, ops, sub, got = Slots(depth), [], 0, 0

    def S():
        nonlocal sub
        s.input()
        assert s.submit() == 0
        ops.append("S")
        sub += 1

    def R():
        nonlocal got
        assert s.result() == 0
        ops.append("R")
        got += 1

    if order == "eager":
        while sub < nbatches:
            S()
            R()
    elif order == "lagged":
        while sub < min(depth - 1, nbatches):
            S()
        while sub < nbatches:
            R()
            S()
        while got < nbatches:
            R()
    elif order == "fill_drain":
        while got < nbatches:
            while sub < nbatches and s.can_input():
                S()
            while got < sub:
                R()
    else:
        raise ValueError(order)
    assert sub == got == nbatches
    return "".join(ops)


# ---- submit-size patterns -------------------------------------------------------------------------------------------
# each returns the list of submit sizes for a pipe of block_bytes B and blocks_per_batch P (every size <= P * B)


def pat_full_ragged_tail(B, P):
    """every batch full, then a ragged tail -- what pipe_compress feeds"""
    return [P * B, P * B, P * B, (P * B) // 2 + 1234 % B + 1]


def pat_edges(B, P):
    """what read() from a pipe gives: short batches in the middle of the stream"""
    return [0, 1, B - 1, B, min(B + 1, P * B), P * B - 1, P * B, 0, 0, 17]


def pat_edges_reversed(B, P):
    return pat_edges(B, P)[::-1]


def pat_zero_runs(B, P):
    """a run of 0-byte batches at the start and at the end"""
    return [0, 0, 0, P * B, B + 5 if P > 1 else B - 5, 1, 0, 0, 0, 0]


def pat_random(B, P, seed=20240611, n=48):
    """seeded random sizes in [0, P * B], the two ends forced in"""
    rng = np.random.default_rng(seed)
    v = [int(x) for x in rng.integers(0, P * B + 1, n)]
    v[3], v[7] = 0, P * B
    return v


def patterns(B, P):
    """name -> (blocks_per_batch, submit sizes): every pattern at P, and the edges once more at P = 1"""
    assert P > 1
    return {
        "full_ragged_tail": (P, pat_full_ragged_tail(B, P)),
        "edges": (P, pat_edges(B, P)),
        "edges_reversed": (P, pat_edges_reversed(B, P)),
        "zero_runs": (P, pat_zero_runs(B, P)),
        "p1": (1, pat_edges(B, 1) + pat_zero_runs(B, 1)),
        "random": (P, pat_random(B, P)),
    }
