"""The draw contract's variates against the reference's probability laws (CPU, the C oracle).

The suite pins the kernels bit for bit to the oracle, and the oracle to the reference only in
replay mode, on the reference's own variates. What maps Philox words to variates (32-bit
uniforms, the median of three for Beta(2, 2), pick_other, the LOSS_r / RESET_r ranks within a
quad) is stated twice by one hand; these tests hold its outcome against the laws of what the
reference draws (tests/law_support.py), and against the reference's own rollouts
(tests/golden/law_rollouts.npz). tests/test_gpu_draw_laws.py runs the same scenarios on the GPU.

Part (a) shows that the checkers can tell: numpy samples (default_rng, fixed seed) from named
wrong laws go through the same checker calls at the same n = 2^18 and must be rejected, samples
from the right laws accepted. What each checker resolves at that n, at ALPHA = 1e-6: the deviation
whose non-centrality lambda = n sum (dp_k)^2 / p_k lifts the statistic's mean, dof + lambda, to the
critical value, so that it is rejected about half the time (twice the deviation, four times lambda,
practically always):

  fuel cost, KS               a CDF off by 2.69 / sqrt(n) = 0.0053 anywhere (the triangular
                              law's is off by 0.125)
  P(done) from low fuel       a probability off by 0.0051 at p = 0.5 (1 dof, critical value 27.5)
  loss amount, chi2           cargo 25, 25 dof, critical value 74.5, lambda 49.5: a gate probability
                              off by 0.008 (lambda = 3.25 n d^2; (c + 1) / 50 is off by 0.02);
                              loss-type bounds off by 0.005 (lambda = 7.95 n e^2; 0.2 / 0.8 are off
                              by 0.1); every partial-loss cell off by 2 % of itself (lambda = 0.4 n r^2)
  destinations, chi2          P = 5, 15 dof, critical value 57.4: one port's share among the other
                              four off by 0.0055 for every origin (lambda = 5.33 n d^2; the double
                              weight is off by 0.15); P = 64, 3968 dof, critical value 4406, 65
                              expected per cell: one port per origin off by 30 % of its 1 / 63
  independence, 8 x 8         49 dof, critical value 111.6: a correlation of about 0.016 between
                              two variates (lambda ~ n rho^2); between quad-mates (n / 4 quads) 0.03
"""
import numpy as np
import pytest

import law_support as LS

O = pytest.importorskip("oracle.oracle")

N = LS.N
COMBOS = [(1, 0), (1, 4_000_000_000), ((1 << 40) + 7, 0), ((1 << 40) + 7, 4_000_000_000), (12345, 5)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()


# ----------------------------------------------------------------- (a) the checkers have power

def rng():
    return np.random.default_rng(20240607)


def losses(r, n, c, *, gate=None, lo=0.1, hi=0.9, part="beta", u_gate=None, lt=None, B=None):
    """the loss of one move from cargo c under the reference's law, or a named variation"""
    g = LS.gate_p(c) if gate is None else gate
    ug = r.random(n) if u_gate is None else u_gate
    lt = r.random(n) if lt is None else lt
    if B is None:
        B = r.random(n) if part == "uniform" else r.beta(2, 2, n)
    partial = np.rint(B * c) if part == "round" else np.floor(B * c)
    loss = np.where(lt < lo, 0, np.where(lt > hi, c, partial))
    return np.where((ug <= g) & (c > 0), loss, 0).astype(np.int64)


def dests(r, n, P, double_weight=False):
    origin = r.integers(0, P, n)
    if double_weight:  # draw over all P, on a collision take the port after the origin
        d = r.integers(0, P, n)
        return origin, np.where(d == origin, (origin + 1) % P, d)
    k = r.integers(0, P - 1, n)
    return origin, k + (k >= origin)


def accepted(stats):
    return all(stat < crit for stat, crit in stats.values())


def test_critical_values():
    assert abs(LS.KS_CRIT - 2.69) < 0.005
    assert abs(LS.chi2_crit(25) - 74.5) < 0.3
    stats = pytest.importorskip("scipy.stats")
    assert abs(stats.norm.isf(LS.ALPHA) - LS.Z_ALPHA) < 1e-3
    # Wilson-Hilferty this far out in the tail: not below the exact value (to 1e-3), up to 15 %
    # above it at 1 dof (27.5 for 23.9), within 2 % from 19 dof on
    for k in (1, 2, 3, 7, 19, 25, 49, 399, 4031):
        ratio = LS.chi2_crit(k) / stats.chi2.isf(LS.ALPHA, k)
        assert 0.999 < ratio < (1.02 if k >= 19 else 1.16), (k, ratio)
    assert stats.kstwobign.sf(LS.KS_CRIT) < LS.ALPHA  # the DKW bound is the looser of the two


def test_exact_laws_are_laws():
    for c in (0, 1, 2, 25, 49, 50, 51, 80):
        assert abs(LS.loss_pmf(c).sum() - 1) < 1e-12 and abs(LS.step_loss_pmf(c).sum() - 1) < 1e-12
    assert LS.step_loss_pmf(0)[0] == 1.0
    assert abs(LS.step_loss_pmf(25)[25] - 0.5 * 0.1) < 1e-12 and abs(LS.step_loss_pmf(80)[80] - 0.1) < 1e-12
    T = LS.cargo_transition(40)
    assert np.allclose(T.sum(1), 1) and np.all(np.triu(T, 1) == 0)
    assert abs(LS.cargo_after(40, 9).sum() - 1) < 1e-12
    x = np.linspace(0, 9, 19)
    assert np.all(np.diff(LS.irwin_hall_cdf(x, 9)) >= 0) and abs(LS.irwin_hall_cdf(4.5, 9) - 0.5) < 1e-9
    assert abs(LS.irwin_hall_cdf(1.0, 2) - 0.5) < 1e-15 and abs(LS.irwin_hall_cdf(0.5, 2) - 0.125) < 1e-15
    # against numpy's own draws of the same laws
    r = rng()
    assert accepted({"ih": LS.ks_one_sample(0.9 * 9 + 0.2 * r.random((N, 9)).sum(1), LS.fuel_burnt_cdf(9))})
    c = np.full(N, 40)
    for _ in range(4):
        nxt = c.copy()
        for v in np.unique(c):
            nxt[c == v] = v - losses(r, int(np.sum(c == v)), int(v))
        c = nxt
    assert accepted({"T4": LS.chi2_gof(np.bincount(c, minlength=41), LS.cargo_after(40, 4))})


def test_right_laws_are_accepted():
    r = rng()
    assert accepted(LS.check_fuel(0.9 + 0.2 * r.random(N)))
    for c in LS.GATE_CARGOS:
        assert accepted(LS.check_loss(c, losses(r, N, c))), c
    assert accepted(LS.check_fuel_gate(r.random(N), losses(r, N, 25), 25))
    assert accepted(LS.check_mates(losses(r, N, 80), 80)) and accepted(LS.check_mates(losses(r, N, 25), 25))
    assert accepted(LS.check_lag(r.random(N), r.random(N)))
    for P in (2, 5, 64):
        assert accepted(LS.check_reset(*dests(r, N, P), P)), P


@pytest.mark.parametrize("c", [25, 80])
def test_rejects_partial_loss_from_a_uniform(c):
    assert LS.rejected(LS.check_loss(c, losses(rng(), N, c, part="uniform")), "chi2")


@pytest.mark.parametrize("c", [25, 80])
def test_rejects_partial_loss_rounded_not_truncated(c):
    assert LS.rejected(LS.check_loss(c, losses(rng(), N, c, part="round")), "chi2")


@pytest.mark.parametrize("c", [1, 2, 25, 49])
def test_rejects_gate_probability_of_cargo_plus_one(c):
    assert LS.rejected(LS.check_loss(c, losses(rng(), N, c, gate=(c + 1) / 50)), "chi2")


@pytest.mark.parametrize("c", [2, 25, 80])
def test_rejects_loss_type_bounds_02_08(c):
    assert LS.rejected(LS.check_loss(c, losses(rng(), N, c, lo=0.2, hi=0.8)), "chi2")


@pytest.mark.parametrize("P", [5, 64])
def test_rejects_double_weight_on_the_port_after_the_origin(P):
    origin, dest = dests(rng(), N, P, double_weight=True)
    assert LS.rejected(LS.check_dest(origin, dest, P), "dest")


def test_rejects_a_destination_equal_to_the_origin():
    origin, dest = dests(rng(), N, 5)
    dest[1000] = origin[1000]
    assert LS.rejected(LS.check_dest(origin, dest, 5), "collisions")


def test_rejects_triangular_fuel_noise():
    assert LS.rejected(LS.check_fuel(1.0 + rng().triangular(-0.1, 0.0, 0.1, N)), "ks")
    assert LS.rejected(LS.check_fuel(5.0 * (1.0 + rng().triangular(-0.1, 0.0, 0.1, N)), 5.0), "ks")


def test_rejects_gate_drawn_from_the_fuel_word():
    r = rng()
    u = r.random(N)
    stats = LS.check_fuel_gate(u, losses(r, N, 25, u_gate=u), 25)
    assert LS.rejected(stats, "lost") and LS.rejected(stats, "amount")


@pytest.mark.parametrize("c", [80, 25])
def test_rejects_quad_mates_sharing_a_loss_block(c):
    """LOSS rank & 1 in place of & 3: the third firing env of a quad takes the first one's block"""
    r = rng()
    q = N // 4
    fire = r.random((q, 4)) <= LS.gate_p(c)
    rank = np.cumsum(fire, 1) - fire
    lt, B = r.random((q, 4)), r.beta(2, 2, (q, 4))
    blk = rank & 1
    rows = np.arange(q)[:, None]
    loss = losses(r, (q, 4), c, u_gate=np.where(fire, 0.0, 2.0), lt=lt[rows, blk], B=B[rows, blk])
    stats = LS.check_mates(loss.reshape(-1), c)
    assert LS.rejected(stats, "kind02") and LS.rejected(stats, "amount02")


def test_rejects_draws_that_ignore_the_step_index():
    u = rng().random(N)
    stats = LS.check_lag(u, u.copy())
    assert LS.rejected(stats, "repeats") and LS.rejected(stats, "lag1")


def test_rejects_a_shifted_return_law():
    """two-sample KS at the end-to-end sizes: 20,000 against 2^16, returns 0.1 sigma apart"""
    r = rng()
    a, b = r.normal(0, 1, 20000), r.normal(0.1, 1, LS.ROLLOUTS)
    stat, crit = LS.ks_two_sample(a, b)
    assert stat >= crit
    stat, crit = LS.ks_two_sample(a, r.normal(0, 1, LS.ROLLOUTS))
    assert stat < crit


# ----------------------------------------------------------------- (b) the oracle obeys every law

Sim = LS.OracleSim


@pytest.mark.parametrize("seed,t", COMBOS)
def test_fuel_noise(seed, t):
    LS.verdict("fuel noise", LS.fuel_noise(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_fuel_noise_across_the_id_carry(seed, t):
    LS.verdict("fuel noise across the id carry", LS.fuel_noise(Sim, seed, t, base=LS.ID_CARRY_BASE),
               f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_out_of_fuel(seed, t):
    LS.verdict("out of fuel", LS.out_of_fuel(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("c", LS.GATE_CARGOS)
@pytest.mark.parametrize("seed,t", COMBOS)
def test_gate_and_loss(seed, t, c):
    LS.verdict("gate and loss", LS.gate_and_loss(Sim, seed, t, c), f"cpu seed={seed} t={t} cargo={c}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_fuel_independent_of_gate(seed, t):
    LS.verdict("FUEL vs GATE", LS.fuel_vs_gate(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("c", [80, 25])
@pytest.mark.parametrize("seed,t", COMBOS)
def test_quad_mates(seed, t, c):
    LS.verdict("quad-mates", LS.quad_mates(Sim, seed, t, c), f"cpu seed={seed} t={t} cargo={c}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_step_to_step(seed, t):
    LS.verdict("step to step", LS.step_to_step(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("P", [2, 5, 64])
@pytest.mark.parametrize("seed,t", COMBOS)
def test_arrival(seed, t, P):
    LS.verdict("arrival", LS.arrival(Sim, seed, t, P), f"cpu seed={seed} t={t} P={P}")


@pytest.mark.parametrize("seed,epoch", COMBOS)
def test_explicit_reset(seed, epoch):
    LS.verdict("explicit reset", LS.explicit_reset(Sim, seed, epoch), f"cpu seed={seed} epoch={epoch}")


@pytest.mark.parametrize("fuel", [0.5, 1.0])
@pytest.mark.parametrize("seed,t", COMBOS)
def test_auto_reset(seed, t, fuel):
    LS.verdict("auto-reset", LS.auto_reset(Sim, seed, t, fuel), f"cpu seed={seed} t={t} fuel={fuel}")


@pytest.mark.parametrize("K", [4, 9])
@pytest.mark.parametrize("seed,t", COMBOS)
def test_step_sequence(seed, t, K):
    LS.verdict("fused sequence", LS.fused_sequence(Sim, seed, t, K), f"cpu seed={seed} t={t} K={K}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_step_sequence_with_arrival(seed, t):
    LS.verdict("fused sequence with arrival", LS.fused_arrival(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_sample_actions(seed, t):
    LS.verdict("sample_actions", LS.sample_actions(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("seed,t", COMBOS)
def test_gen_actions(seed, t):
    LS.verdict("gen_actions", LS.gen_actions(Sim, seed, t), f"cpu seed={seed} t={t}")


@pytest.mark.parametrize("seed", [1, (1 << 40) + 7, 12345])
def test_rollout_first_step(seed):
    LS.verdict("rollout first step", LS.rollout_first_step(Sim, seed), f"cpu seed={seed}")


# ----------------------------------------------------------------- end to end against the reference

def test_law_fixture_is_what_the_tests_assume():
    g = LS.golden_rollouts()
    assert g["states"].shape == (LS.START_STATES, 6) and (g["states"][:, 5] >= 0).all() and (g["states"][:, 2] > 0).all()
    R = len(g["ret_0"])
    for k in range(LS.START_STATES):
        assert len(g[f"ret_{k}"]) == R and g[f"steps_done_{k}"].sum() == R
        assert (np.diff(g[f"ret_{k}"]) >= 0).all()
        sd = g[f"steps_done_{k}"]
        assert sd[0].sum() == 0 and sd[:LS.MAX_STEPS, 0].sum() == 0  # not done: all 100 steps counted
    assert g["steps_done_1"][:, 1].sum() > 0.9 * R  # fuel 40: nearly every rollout runs dry
    assert 0.2 * R < g["steps_done_4"][:, 1].sum() < 0.8 * R  # fuel 97: some do, some do not
    # the states are on water or a port of the fixture's map
    w = g["world"]
    for x, y, *_ in g["states"].tolist():
        assert w.water[x, y] != 0 or [x, y] in w.ports


@pytest.mark.parametrize("k", range(LS.START_STATES))
@pytest.mark.parametrize("seed", [1, (1 << 40) + 7])
def test_rollouts_vs_the_reference(seed, k):
    LS.verdict("se_rollout vs reference", LS.rollout_vs_reference(Sim, seed, k), f"cpu seed={seed} state={k}")


@pytest.mark.parametrize("k", range(LS.START_STATES))
@pytest.mark.parametrize("seed", [1, (1 << 40) + 7])
def test_policy_loop_vs_the_reference(seed, k):
    LS.verdict("policy loop vs reference", LS.policy_loop_vs_reference(Sim, seed, k),
               f"cpu seed={seed} state={k}")
