"""The dense auto-reset cases of tests/autoreset_support.py are what they claim to be, on the C
oracle alone: a pattern edited so that a case of test_gpu_autoreset_dense.py is no longer reached
fails here, without a GPU."""
import numpy as np
import pytest

import autoreset_support as A

T0S = (7, 2**32 - 1)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def _cases():
    return [(p, n) for p in A.PATTERNS for n in A.SIZES]


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("pattern,n", _cases())
def test_done_is_the_chosen_mask(pattern, n, t0):
    """Both steps of every case: done equals the mask, a finished env stands fresh on its new
    origin port, and the first step's ships start where the case says."""
    c = A.case(pattern, n, t0)
    assert (c.steps[0].before.x == A.START[0]).all() and (c.steps[0].before.y == A.START[1]).all()
    px, py = np.array(A.PORTS).T
    for k, s in enumerate(c.steps):
        np.testing.assert_array_equal(s.after.done != 0, s.mask, err_msg=f"step {k}")
        np.testing.assert_array_equal(s.mask, A.mask(s.pattern, n))
        d = s.mask
        assert (s.after.err[d] == 0).all()
        a = s.after
        assert (a.fuel[d] == 200.0).all() and (a.cargo[d] == 0).all() and (a.ep_len[d] == 0).all()
        assert (a.x[d] == px[a.origin[d]]).all() and (a.y[d] == py[a.origin[d]]).all()
        assert (a.dest[d] != a.origin[d]).all()
        np.testing.assert_array_equal(s.exp.env, np.nonzero(d)[0])
    assert c.steps[1].pattern == A.second_pattern(pattern) != pattern


def test_every_pattern_is_some_case_s_second_step():
    assert sorted(A.second_pattern(p) for p in A.PATTERNS) == sorted(A.PATTERNS)


@pytest.mark.parametrize("n", A.SIZES)
def test_per_wave_totals(n):
    waves = n // A.SEG
    per = lambda p: [int(A.mask(p, n)[w * A.SEG:(w + 1) * A.SEG].sum()) for w in range((n + A.SEG - 1) // A.SEG)]
    assert per("all")[:waves] == [256] * waves       # segments filled to their capacity
    assert per("none") == [0] * len(per("none"))
    assert per("counts")[:waves] == [128] * waves
    tot = per("totals")
    assert tuple(tot[:min(waves, 5)]) == A.WAVE_TOTALS[:min(waves, 5)]
    m = A.mask("totals", n)
    assert m[5 * A.SEG:].all()
    # the filler lengths 7, 1, 0, 7, 1 of the five full waves
    assert [(-t) % A.FILLER_RUN for t in A.WAVE_TOTALS] == [7, 1, 0, 7, 1]
    # wave 0: one record, from lane 63's last env (the one-lane shortcut at its last source
    # lane); wave 1: lanes 0 and 1 (the trees)
    assert np.nonzero(m[:A.SEG])[0].tolist() == [255]
    lanes = lambda w: set((np.nonzero(m[w * A.SEG:(w + 1) * A.SEG])[0] // 4).tolist())
    if waves > 1:
        assert lanes(1) == {0, 1}
    if waves > 4:
        assert lanes(4) == set(range(64))
    for p, lo, hi in (("random50", 0.4, 0.6), ("random5", 0.02, 0.09)):
        assert lo < A.mask(p, n).mean() < hi
        # some wave with no record or one only, and some quad with two or more
        q = A.mask(p, n)[:n & ~3].reshape(-1, 4).sum(1)
        assert (q >= 2).any()


@pytest.mark.parametrize("n", A.SIZES)
def test_counts_holds_all_16_quad_masks_in_every_full_wave(n):
    m = A.mask("counts", n)
    for w in range(n // A.SEG):
        q = m[w * A.SEG:(w + 1) * A.SEG].reshape(64, 4)
        codes = (q * (1 << np.arange(4))).sum(1)
        assert set(codes.tolist()) == set(range(16))
        assert set(q.sum(1).tolist()) == {0, 1, 2, 3, 4}
    q = A.mask("all", n)[:n & ~3].reshape(-1, 4)
    assert (q.sum(1) == 4).all()


def test_tail_groups():
    n = A.N_TAIL_APPENDS
    assert n == 4 * (64 * 5 + 17) + 2 and n % 4 == 2
    g = n >> 2
    assert g & 63 == 17  # the tail group's segment holds the records of 17 lanes before the tail's
    for p in ("all", "random50", "totals"):
        m = A.mask(p, n)
        seg = g >> 6
        assert m[seg * A.SEG:4 * g].sum() > 0, p   # records before the tail's
        assert m[4 * g:].sum() > 0, p              # and the tail dies
    assert A.mask("all", n)[4 * g:].all() and A.mask("totals", n)[4 * g:].all()
    n = A.N_TAIL_FRESH
    assert (n >> 2) & 63 == 0 and n % 4 == 3  # its tail group opens a fresh segment
    assert A.mask("all", n)[n & ~3:].all()
    assert A.N_RECORD % 4 == 0 and A.N_RECORD % A.SEG == 0


@pytest.mark.parametrize("pattern,n", _cases())
def test_losses_and_errors_run_beside_the_resets(pattern, n):
    c = A.case(pattern, n)
    s = c.steps[0]
    np.testing.assert_array_equal(s.before.cargo, np.array(A.CARGO)[np.arange(n) % 3])
    d = s.mask
    moved = (s.after.err == 0) & (s.actions < 4)
    assert moved[d].all()
    # a move on water: -1.0001, -10 out of fuel, closer +2 / farther -2, then -3 per unit of
    # cargo lost: the loss in units, read back from the reward
    r4 = np.rint(s.after.reward * 1e4).astype(np.int64) + np.where(d, 100000, 0) + 10001
    loss = np.where((r4 - 20000) % 30000 == 0, -(r4 - 20000) // 30000, -(r4 + 20000) // 30000)
    ok = moved & (((r4 - 20000) % 30000 == 0) | ((r4 + 20000) % 30000 == 0))
    np.testing.assert_array_equal(ok, moved)
    assert (loss[moved] >= 0).all() and (loss[moved] <= s.before.cargo[moved]).all()
    survivors = moved & ~d
    np.testing.assert_array_equal(s.after.cargo[survivors], (s.before.cargo - loss)[survivors])
    if d.any():
        assert (loss[d] > 0).any(), "some dying env also loses cargo in the same step"
        # two or more envs of one quad lose cargo: the LOSS ranks
        if pattern in ("all", "counts", "random50"):
            assert ((loss > 0)[:n & ~3].reshape(-1, 4).sum(1) >= 2).any()
    if (~d).sum() > 100:
        errs = set(np.unique(s.after.err[~d]).tolist())
        assert len(errs - {0}) >= 2, errs  # survivors show at least two distinct err codes
        assert (s.after.ep_len[~d] == s.before.ep_len[~d] + 1).all()


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("pattern,n", _cases())
def test_expected_records_sum_to_the_oracle_s_stats(pattern, n, t0):
    c = A.case(pattern, n, t0)
    start = c.start0
    for s in c.steps:
        e = s.exp
        assert s.stats[0] == A.sequential_sum(e.ret.astype(np.float64))
        assert s.stats[1] == len(e.env) == int(s.mask.sum())
        assert s.stats[2] == int(e.len.astype(np.int64).sum())
        assert (e.len >= 1).all() and (e.step.view(np.uint32) == s.t & 0xFFFFFFFF).all()
        np.testing.assert_array_equal(e.counts, np.bincount(np.nonzero(s.mask)[0] // A.SEG, minlength=len(e.counts)))
        # the stamps: t + 1 (mod 2^32) where done, untouched elsewhere; they give the oracle's lengths
        np.testing.assert_array_equal(e.start[~s.mask], start[~s.mask])
        t_next = (s.t + 1) & 0xFFFFFFFF
        assert (e.start.view(np.uint32)[s.mask] == t_next).all()
        np.testing.assert_array_equal((t_next - e.start.view(np.uint32).astype(np.int64)) & 0xFFFFFFFF, s.after.ep_len)
        start = e.start
    if t0 == 2**32 - 1:
        assert c.steps[0].exp.step[:1].tolist() in ([], [-1]) and (c.steps[1].t & 0xFFFFFFFF) == 0


def test_raw_half_layout():
    """raw_half: the records from each segment's start, the filler up to the next run of 8 past the
    full groups' records, the tail group's records over the filler, the sentinel elsewhere."""
    n = A.N_TAIL_APPENDS
    s = A.case("totals", n).steps[0]
    for pad in (False, True):
        half, counts = A.raw_half(s.exp, n, 8, s.t, pad)
        assert counts.tolist() == [1, 7, 8, 9, 255, 70, 0, 0]
        filler = (half[:, 0] == -1).reshape(8, A.SEG).sum(1)
        # segment 5: 68 records of 17 lanes, filler to 72, two of them under the tail's records
        assert filler.tolist() == ([7, 1, 0, 7, 1, 2, 0, 0] if pad else [0] * 8)
        sent = (half[:, 0] == A.SENTINEL).reshape(8, A.SEG).sum(1)
        np.testing.assert_array_equal(sent, A.SEG - counts - filler)
        assert (half[half[:, 0] == -1][:, 1:] == (0, 0, s.t)).all()
        np.testing.assert_array_equal(np.concatenate([half[k * A.SEG:k * A.SEG + c] for k, c in enumerate(counts)]),
                                      s.exp.recs)
