"""The algebra behind the level-1 greedy scan (hd_device.hpp fn8_scan_state0, Fn8Ident), on the CPU.

A lane's transition is eight bytes {a,0,1,2 | 3,4,5,6}, a = jump - 1; the lanes the last step's match still covers are
literals (a = 0), not the identity.  Every map being elementary, a composite of k <= 4 of them has the upper dword
{4-k, 5-k, 6-k, 7-k}, so the upper dword that the stages row_shr:1, :2 and :4 would fetch from the lane d = 1, 2, 4
below is a function of the lane number, kept in Fn8Ident::hi[0..2], and those stages move the lower dword only.

Here a numpy model runs the six stages the way the kernel now does -- constant selectors in the first three, the
identity OR-ed in where a row_shr has no source, the two cross-row stages -- for every carry 0..63 over random jumps
1..8 (runs of eights among them), and holds
  * the start mask against a serial greedy parse,
  * the upper dword after the stages that shift by 1 and 2 to the stated lane constant,
  * the constant selector of each of the three stages to the upper dword a DPP fetch would have brought, and with it the
    upper dword behind the stage that shifts by 4 to the lookup with the fetched selector.
A selector constant that is off by one lane fails it (the last test)."""
import numpy as np

IDENT = np.arange(8, dtype=np.uint8)
TRIALS = 24


def _selector_consts():
    """Fn8Ident::init, as bytes: hi[s][lane] = {4-k..7-k}, k = lanes the map shifted in by stage s covers"""
    r = np.arange(64) & 15
    k0 = np.where(r < 1, 0, 1)
    k1 = np.where(r < 2, 0, np.where(r < 3, 1, 2))
    k2 = np.where(r < 4, 0, np.where(r < 7, r - 3, 4))
    return [(np.arange(4, 8)[None, :] - k[:, None]).astype(np.uint8) for k in (k0, k1, k2)]


def _compose(then, first):
    """(then o first)(r) = then[first(r)]: v_perm_b32 with `then` as the table and `first` as the selectors"""
    return np.take_along_axis(then, first, axis=-1)


def _row_shr(w, d):
    """[T, 64, 8] shifted up by d lanes inside each row of 16, and the mask of lanes that have a source"""
    src = (np.arange(64) & 15) >= d
    sh = np.zeros_like(w)
    sh[:, d:] = w[:, :-d]
    return sh, src


def _jumps(rng, trials):
    j = rng.integers(1, 9, (trials, 64))
    j[0] = 8                                            # a run of eights over the whole step
    j[1] = 1
    j[2, ::2] = 8                                       # runs of eights with a lane between
    j[3] = np.where(rng.random(64) < 0.8, 8, j[3])
    j[4] = np.where(rng.random(64) < 0.5, 8, 1)
    return j


def _model(jump, carry, consts, checks=True):
    """jump [T, 64] in 1..8, carry 0..63 -> start mask [T, 64] as the kernel's scan finds it"""
    T = jump.shape[0]
    live = np.arange(64) >= carry
    w = np.empty((T, 64, 8), dtype=np.uint8)
    w[:, :, 0] = np.where(live[None, :], jump - 1, 0)    # covered lanes: literals
    w[:, :, 1:] = np.arange(7, dtype=np.uint8)
    r = np.arange(64) & 15
    for s, d in enumerate((1, 2, 4)):
        sh, src = _row_shr(w, d)
        fetched = np.where(src[None, :, None], sh, IDENT)
        first = fetched.copy()
        first[:, :, 4:] = consts[s][None, :, :]          # the upper dword is not fetched
        if checks:
            assert np.array_equal(fetched[:, :, 4:], np.broadcast_to(consts[s], (T, 64, 4))), ("selector of stage", s)
        new = _compose(w, first)
        if checks:
            assert np.array_equal(new[:, :, 4:], _compose(w, fetched)[:, :, 4:]), ("upper dword behind stage", s)
            if d < 4:
                k = np.minimum(r + 1, 2 * d)
                want = (np.arange(4, 8)[None, :] - k[:, None]).astype(np.uint8)
                assert np.array_equal(new[:, :, 4:], np.broadcast_to(want, (T, 64, 4))), ("lane constant behind stage", s)
        w = new
    sh, src = _row_shr(w, 8)
    w = _compose(w, np.where(src[None, :, None], sh, IDENT))
    # row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3; the other rows: the identity
    x = np.broadcast_to(IDENT, w.shape).copy()
    x[:, 16:32] = w[:, 15:16]
    x[:, 48:64] = w[:, 47:48]
    w = _compose(w, x)
    x = np.broadcast_to(IDENT, w.shape).copy()
    x[:, 32:64] = w[:, 31:32]
    w = _compose(w, x)
    behind = w[:, :, 0] != 0                             # a state other than 0 BEHIND the lane
    entered = np.zeros_like(behind)
    entered[:, 1:] = behind[:, :-1]                      # ... one lane up; 0 enters lane 0
    return live[None, :] & ~entered


def _serial(jump, carry):
    out = np.zeros(jump.shape, dtype=bool)
    for t in range(jump.shape[0]):
        p = carry
        while p < 64:
            out[t, p] = True
            p += int(jump[t, p])
    return out


def test_selector_constants_are_elementary_composites():
    c = _selector_consts()
    r = np.arange(64) & 15
    # row_shr:1 -- one lane below, the identity at row lane 0
    assert all(bytes(c[0][l]) == (b"\x04\x05\x06\x07" if r[l] == 0 else b"\x03\x04\x05\x06") for l in range(64))
    # row_shr:2 -- identity at row lanes 0 and 1, one lane at row lane 2, two from row lane 3 on
    assert all(bytes(c[1][l]) == (b"\x04\x05\x06\x07" if r[l] < 2 else b"\x03\x04\x05\x06" if r[l] == 2 else b"\x02\x03\x04\x05")
               for l in range(64))
    # row_shr:4 -- identity at row lanes 0..3, then k = 1, 2, 3 at row lanes 4, 5, 6, then k = 4
    for l in range(64):
        k = 0 if r[l] < 4 else min(r[l] - 3, 4)
        assert list(c[2][l]) == [4 - k, 5 - k, 6 - k, 7 - k], l


def test_scan_with_constant_selectors_equals_the_serial_parse_at_every_carry():
    consts = _selector_consts()
    for carry in range(64):
        jump = _jumps(np.random.default_rng([13, carry]), TRIALS)
        got = _model(jump, carry, consts)
        assert np.array_equal(got, _serial(jump, carry)), carry


def test_covered_lanes_as_identity_give_the_same_starts():
    """the parent's form (identity on the covered lanes, every upper dword fetched) and this one agree on the starts"""
    for carry in (1, 7, 15, 16, 17, 33, 63):
        jump = _jumps(np.random.default_rng([14, carry]), 16)
        T = jump.shape[0]
        live = np.arange(64) >= carry
        f = np.empty((T, 64, 8), dtype=np.uint8)
        f[:, :, 0] = jump - 1
        f[:, :, 1:] = np.arange(7, dtype=np.uint8)
        f[:, ~live] = IDENT
        state, starts = np.zeros(T, dtype=np.int64), np.zeros((T, 64), dtype=bool)
        for l in range(64):
            starts[:, l] = live[l] & (state == 0)
            state = f[np.arange(T), l, state]
        assert np.array_equal(starts, _model(jump, carry, _selector_consts())), carry


def test_a_selector_off_by_one_lane_is_seen():
    good = _selector_consts()
    jump = _jumps(np.random.default_rng([15]), TRIALS)
    for s in range(3):
        for shift in (1, -1):
            bad = [c.copy() for c in good]
            bad[s] = np.roll(good[s], shift, axis=0)
            for carry in (0, 21):
                try:
                    _model(jump, carry, bad)
                    seen = False
                except AssertionError:
                    seen = True
                assert seen, (s, shift, carry)
                # and without the stage checks the starts themselves come out wrong
                assert not np.array_equal(_model(jump, carry, bad, checks=False), _serial(jump, carry)), (s, shift, carry)
