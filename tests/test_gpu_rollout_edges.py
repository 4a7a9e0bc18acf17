"""se_sample_actions and se_rollout against the C oracle, bit for bit, where the two kernels can
go wrong without tests/test_gpu_rollout.py noticing: every rollout status (ATTEMPTS and the zero
budgets among them), the retried steps, the second Philox block (beta uniforms and the arrival
redraw), batches that are no multiple of a wave, bad sources inside a wave, more items than the
grid has threads (the grid-stride loops), 64-bit rollout and env ids, and the world's edges
(P = 1, 64 and 254 ports, shared cells, an empty stock, x and y past 127, cargo past 2^21).

The actors come from tests/rollout_support.py; tests/test_rollout_cpu.py shows on the oracle's
rollout trace that they go through what they are named after. ret is compared as uint64."""
import numpy as np
import pytest

import rollout_support as RS
from step_seq_support import assert_same, device_rows, empty_state, load, oracle_trace, snapshot
from test_gpu_rollout import load_state, oracle_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

STATE = ("x", "y", "fuel", "cargo", "origin", "dest")
GRID_THREADS = 2048 * 256  # the most threads either kernel launches


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def table_env(name, reps=1, seed=RS.SEED, env_id_base=0):
    """(env, oracle world, oracle state) of the world's actor table."""
    w = RS.WORLDS[name]
    st = RS.table(O, name, reps)
    env = w.env(st.n, seed=seed, env_id_base=env_id_base)
    load_state(env, st)
    return env, w.oracle(O), st


def assert_rollout(env, world, st, src, ms, ma, base=0, what=""):
    """One rollout batch equals the oracle's in ret (bits), steps and status; returns the oracle's."""
    ret, steps, status = env.rollout(src, max_steps=ms, max_attempts=ma, rollout_base=base)
    want = O.rollout(world, st, src, max_steps=ms, max_attempts=ma, seed=env.seed, rollout_base=base)
    tag = f"{what} max_steps={ms} max_attempts={ma} base={base}"
    np.testing.assert_array_equal(status.cpu().numpy(), want[2], err_msg=f"{tag}: status")
    np.testing.assert_array_equal(steps.cpu().numpy(), want[1], err_msg=f"{tag}: steps")
    np.testing.assert_array_equal(ret.cpu().numpy().view(np.uint64), want[0].view(np.uint64), err_msg=f"{tag}: ret")
    return want


def assert_sample(env, world, st, t, env_id_base=0, what=""):
    got = [v.cpu().numpy() for v in env.sample_actions(t)]
    want = O.sample_actions(world, st, seed=env.seed, env_id_base=env_id_base, t=t)
    for g, r, f in zip(got, want, ("type", "a", "b")):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, r, err_msg=f"{what} t={t}: {f}")
    return want


def assert_unchanged(env, st, what=""):
    after = oracle_state(env)
    for f in STATE:
        g, w = getattr(after, f), getattr(st, f)
        if f == "fuel":
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: the rollout changed {f}")


# ----------------------------------------------------------------- the scenario tables
@pytest.mark.parametrize("name", list(RS.WORLDS))
def test_scenario_tables_at_every_budget(name):
    """Each world's table, 64 rollouts per actor, at max_steps 0, 1, 20 and max_attempts 0, 1,
    max_steps + 1 and 8 * max_steps: ATTEMPTS and its turn into MAX_STEPS after the loop, the zero
    budgets, RAISED at the first attempt, the retries and both Philox blocks."""
    env, world, st = table_env(name)
    src = RS.table_src(name)
    seen = set()
    for ms in (0, 1, 20):
        for ma in sorted({0, 1, ms + 1, 8 * ms}):
            want = assert_rollout(env, world, st, src, ms, ma, what=name)
            assert_unchanged(env, st, f"{name} {ms} {ma}")
            seen |= set(want[2].tolist())
            if ms == 0 and ma > 0:
                assert (want[2] == RS.MAX_STEPS).all()  # the loop's test comes before the sample
            if ma == 0:
                assert (want[2] == (RS.ATTEMPTS if ms else RS.MAX_STEPS)).all()
    if name == "open":
        assert seen == {RS.DONE, RS.MAX_STEPS, RS.RAISED, RS.ATTEMPTS}
    env.close()


@pytest.mark.parametrize("t", [0, 7, (1 << 32) - 1])
@pytest.mark.parametrize("name", list(RS.WORLDS))
def test_scenario_sample_actions(name, t):
    """The random policy on every actor in every lane (each actor 64 times in a row)."""
    env, world, st = table_env(name, reps=RS.REPS)
    ty = assert_sample(env, world, st, t, what=name)[0]
    for a, (label, _, claims) in enumerate(RS.actors(name)):
        for c in claims:
            if c[0] == "sample":
                assert (ty[a * RS.REPS:(a + 1) * RS.REPS] == c[1]).all(), label
    env.close()


# ----------------------------------------------------------------- the batch's shape
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_batch_sizes_shuffled_sources_and_bad_sources(m):
    """Batches around a wave and past a workgroup: sources drawn with repeats (so the lanes of a
    wave run different actors) and bad sources first, last and in the middle of a wave."""
    env, world, st = table_env("open")
    n = st.n
    rng = np.random.default_rng(m)
    src = rng.integers(0, n, m).astype(np.int32)
    assert_rollout(env, world, st, src, 20, 21, base=m, what=f"m={m}")
    bad = {0: -1, m - 1: n, m // 2: n + 7}
    if m > 128:
        bad.update({64 + 31: -(1 << 31), 63: (1 << 31) - 1})
    for k, v in bad.items():
        src[k] = v
    want = assert_rollout(env, world, st, src, 20, 160, base=m, what=f"m={m} with bad sources")
    where = np.array(sorted(bad))
    assert (want[2][where] == RS.BAD_SRC).all() and (want[1][where] == 0).all() and (want[0][where] == 0).all()
    assert ((want[2] == RS.BAD_SRC).sum()) == len(where)
    assert_unchanged(env, st, f"m={m}")
    env.close()


# ----------------------------------------------------------------- the grid-stride loops
def test_more_rollouts_than_threads():
    """2048 * 256 + 257 rollouts: the first 257 threads run two rollouts, the second from the
    world staged in LDS for the first."""
    env, world, st = table_env("open")
    labels = [a[0] for a in RS.actors("open")]
    four = np.array([labels.index(k) for k in ("next_to_dest", "loaded_60", "corner_last", "select_other_origin")], np.int32)
    m = GRID_THREADS + 257
    src = four[np.arange(m) % 4]
    src[[GRID_THREADS - 1, GRID_THREADS + 5]] = [st.n, -1]
    want = assert_rollout(env, world, st, src, 3, 24, base=11, what="grid stride")
    tail = want[2][GRID_THREADS:]
    assert (tail == RS.BAD_SRC).sum() == 1 and (tail == RS.MAX_STEPS).any()
    assert_unchanged(env, st, "grid stride")
    env.close()


def test_more_sampled_envs_than_threads():
    n = GRID_THREADS + 257
    base = RS.table(O, "open")
    idx = np.arange(n) % base.n
    st = O.OracleState(n)
    for f in STATE:
        getattr(st, f)[:] = getattr(base, f)[idx]
    env = RS.OPEN.env(n)
    load_state(env, st)
    ty = assert_sample(env, RS.OPEN.oracle(O), st, 7, what="grid stride")[0]
    assert len(set(ty[GRID_THREADS:].tolist())) >= 4  # moves, selects, takes and a raise in the second pass
    env.close()


# ----------------------------------------------------------------- the keys
@pytest.mark.parametrize("base", [0, (1 << 32) - 1, 1 << 32, (1 << 40) + 3])
def test_rollout_base_is_a_64_bit_id(base):
    """base 2^32 - 1: the ids carry into the high word inside the batch. Truncated to 32 bits,
    base 2^32 would draw what base 0 draws."""
    env, world, st = table_env("open")
    src = RS.table_src("open")
    want = assert_rollout(env, world, st, src, 20, 160, base=base, what="keys")
    other = O.rollout(world, st, src, max_steps=20, max_attempts=160, seed=env.seed, rollout_base=base ^ (1 << 32))
    assert not np.array_equal(want[0], other[0])
    env.close()


def test_rollout_sub_batch_equals_slice_and_bases_differ():
    env, world, st = table_env("open")
    src = RS.table_src("open")
    base = (1 << 32) - 100  # the sub-batch below starts past the carry
    whole = [v.cpu().numpy() for v in env.rollout(src, max_steps=20, max_attempts=160, rollout_base=base)]
    for a, b in ((0, 64), (130, 333), (len(src) - 1, len(src))):
        part = [v.cpu().numpy() for v in env.rollout(src[a:b].copy(), max_steps=20, max_attempts=160, rollout_base=base + a)]
        np.testing.assert_array_equal(part[0].view(np.uint64), whole[0][a:b].view(np.uint64))
        np.testing.assert_array_equal(part[1], whole[1][a:b])
        np.testing.assert_array_equal(part[2], whole[2][a:b])
    again = [v.cpu().numpy() for v in env.rollout(src, max_steps=20, max_attempts=160, rollout_base=base + 1)]
    assert not np.array_equal(again[0], whole[0]) and not np.array_equal(again[1], whole[1])
    env.close()


@pytest.mark.parametrize("k", [8, (1 << 34) + 8])
def test_sample_actions_of_a_shard(k):
    """An env made with env_id_base = k answers as the oracle's envs k .., and as rows k .. of
    the unsharded env where that one can be made."""
    env, world, st = table_env("open", reps=RS.REPS, env_id_base=k)
    for t in (0, 7, (1 << 32) - 1):
        want = assert_sample(env, world, st, t, env_id_base=k, what=f"shard {k}")
        zero = O.sample_actions(world, st, seed=env.seed, env_id_base=0, t=t)
        assert not np.array_equal(want[1], zero[1])  # the base takes part in the draw
    env.close()
    if k < 64:
        whole, _, st2 = table_env("open", reps=RS.REPS)
        part = RS.OPEN.env(st2.n - k, env_id_base=k)
        sub = O.OracleState(st2.n - k)
        for f in STATE:
            getattr(sub, f)[:] = getattr(st2, f)[k:]
        load_state(part, sub)
        for g, w in zip(part.sample_actions(3), whole.sample_actions(3)):
            np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy()[k:])
        part.close()
        whole.close()


# ----------------------------------------------------------------- the world's edges
_BIG = {}


def big_world(which):
    if which not in _BIG:
        _BIG[which] = RS.max_world() if which == "max" else RS.MANY
    return _BIG[which]


@pytest.mark.parametrize("which", ["max", "many"])
def test_rollouts_and_samples_in_the_largest_worlds(which):
    """256 x 256 cells with 254 ports (14 shared cells), and 64 ports: 257 envs after a reset and
    40 steps of the synthetic agent, 4 rollouts each; the sampler on the same states."""
    w = big_world(which)
    n, k, seed = 257, 4, 31
    env = w.env(n, seed=seed)
    world = w.oracle(O)
    env.reset()
    for t in range(40):
        env.step(env.gen_actions(t))
    st = oracle_state(env)
    if which == "max":
        assert ((st.x >= 128) | (st.y >= 128)).sum() > n // 4 and (st.x >= 128).any() and (st.y >= 128).any()
        assert st.origin.max() >= 128  # a port index past 127 too
    src = np.repeat(np.arange(n, dtype=np.int32), k)
    want = assert_rollout(env, world, st, src, 30, 240, base=7 * n, what=which)
    assert {RS.MAX_STEPS} <= set(want[2].tolist())
    _, _, _, log = O.rollout(world, st, src, max_steps=30, max_attempts=240, seed=seed, rollout_base=7 * n, trace=True)
    assert (log["used"] & RS.USED_BETA).any()
    if which == "many":  # ports are a step apart there
        assert (log["used"] & RS.USED_ARRIVE).any()
    assert_unchanged(env, st, which)
    for t in (0, (1 << 32) - 1):
        assert_sample(env, world, st, t, what=which)
    env.close()


# ----------------------------------------------------------------- cargo past 2^21 in the step kernels
def test_big_cargo_in_step_and_fused_step_seq():
    """beta_part's f64 branch (cargo >= 2^21) in se_step and in a fused se_step_seq of three
    steps (two state-only steps, then the full one), each against the oracle's step: the oracle
    shows a partial loss from cargo >= 2^21 in an inner step and in the last one. This proves
    that the f64 branch runs and agrees with the oracle. It does not pin the 2^21 threshold
    itself: the branch's two forms differ on a vanishing share of median words."""
    K, reps = 3, 67  # 5 * 67 = 335 envs: 83 full groups and a tail of 3
    cargos = [sh["cargo"] for label, sh, _ in RS.actors("heavy") if label.startswith("big_cargo")]
    assert min(cargos) == RS.BIG - 1 and RS.BIG in cargos and max(cargos) <= 1 << 28
    n = len(cargos) * reps
    init = empty_state(n)
    init["x"][:], init["y"][:] = 3, 4
    init["origin"][:], init["dest"][:] = 0, 1
    init["cargo"][:] = np.repeat(cargos, reps)
    init["fuel"][:] = 100.0 + 0.125 * np.arange(n)
    acts = np.random.default_rng(3).integers(0, 4, (K, n)).astype(np.int32)
    want = oracle_trace(O, RS.HEAVY, init, acts, seed=RS.SEED)
    before = [init] + want[:-1]
    partial = [(b["cargo"] >= RS.BIG) & (a["cargo"] > 0) & (a["cargo"] < b["cargo"]) & (a["origin"] == b["origin"])
               for b, a in zip(before, want)]
    assert partial[0].any() and partial[1].any() and partial[K - 1].any()
    assert all((s["err"] == 0).all() for s in want)

    env = RS.HEAVY.env(n)
    load(env, init)
    dev = device_rows(env, acts)
    for k in range(K):
        env.step(dev[k].contiguous())
        assert_same(snapshot(env), want[k], f"se_step, step {k}")
    load(env, init)
    env.step_seq(dev)
    assert_same(snapshot(env), want[K - 1], "se_step_seq")
    env.close()
