"""The step kernels at the edges of their arguments and variates (tests/golden/step_edges.npz,
recorded from the reference by tests/golden/make_step_edge_golden.py): maps of side 1 to 256,
moves up to +-2^31, cargo from negative to the int32 contract's bound, fuel from -0.0 to inf,
every variate on its comparison boundary.

* replay: se_step_replay and se_step_agent_replay over all records of a world in one launch
  (ragged batch sizes: whatever the record count is) against the reference's own outcome, bit
  for bit, tape.used included;
* production draws: se_step_typed, se_step and a two-step se_step_seq from the same pre-states
  against the C oracle on the same seed, with auto-reset off and on. The oracle is the reference
  there; test_step_edges_cpu.py pins it to the reference on this very domain.

Records outside the cargo contract (beyond_contract = 1, under 1 %) are skipped, by that column."""
import numpy as np
import pytest

import step_edge_support as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORLDS = range(S.n_worlds())
WITH_PORTS = [w for w in WORLDS if len(S.world(w)[1])]
SEED, T0 = 991, 5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from shippingenv_amd import build

    build.build(verbose=False)


def make_env(w, sel, **kw):
    from shippingenv_amd.vec import VecEnv

    water, px, py, pf, pc = S.world(w)
    env = VecEnv(len(sel), water=water, ports=[[int(a), int(b)] for a, b in zip(px, py)], port_fuel=pf,
                 port_cargo=pc, **kw)
    for f, v in S.pre_state(sel, u8_none=True).items():
        t = getattr(env, f)
        t.copy_(torch.from_numpy(np.ascontiguousarray(v).astype(t.cpu().numpy().dtype)))
    return env


def get_state(env):
    torch.cuda.synchronize()
    out = {}
    for f in S.FIELDS:
        v = getattr(env, f).cpu().numpy()
        out[f] = np.where(v == 255, -1, v.astype(np.int32)) if f in ("origin", "dest") else v
    return out


def assert_outcome(env, sel, what):
    z = S.fixture()
    S.assert_post(get_state(env), sel, what)
    np.testing.assert_array_equal(env.reward.cpu().numpy(), z["reward"][sel].astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(env.done.cpu().numpy().astype(np.int32), z["done"][sel], err_msg=what)
    np.testing.assert_array_equal(env.err.cpu().numpy().astype(np.int32), z["err"][sel], err_msg=what)


# ---------------------------------------------------------------- replay against the reference
@pytest.mark.parametrize("w", WORLDS)
def test_step_replay_matches_reference_edges(w):
    from shippingenv_amd.vec import TAPE_DTYPE

    z = S.fixture()
    sel = S.records(w)
    env = make_env(w, sel)
    env.step_replay(z["act_type"][sel], z["act_a"][sel], z["act_b"][sel], S.tape_of(TAPE_DTYPE, sel))
    assert_outcome(env, sel, f"se_step_replay world {w}")
    used = env._keep[3].cpu().numpy().view(TAPE_DTYPE)["used"]
    np.testing.assert_array_equal(used, z["used"][sel])
    env.close()


@pytest.mark.parametrize("w", WITH_PORTS)
def test_step_agent_replay_matches_reference_edges(w):
    """The agent-path kernel's replay instantiation on the records the reference's decode can
    express (unit moves, a port in range, amounts): agent_idx is the index it decodes from."""
    from shippingenv_amd.vec import TAPE_DTYPE

    z = S.fixture()
    sel = S.records(w, S.agent_expressible())
    assert len(sel) > 30
    P = len(S.world(w)[1])
    if P == 5:  # the inverse agrees with the reference's own decode table where one is recorded
        from test_gpu_parity import _reference_decode

        dec = _reference_decode(P)
        for i in sel[::7]:
            t, a, b = (int(z[k][i]) for k in ("act_type", "act_a", "act_b"))
            assert dec[int(z["agent_idx"][i])] == (t, a, b if t == 1 else 0)
    env = make_env(w, sel)
    _, _, _, tape = env.step_agent_replay(z["agent_idx"][sel], S.tape_of(TAPE_DTYPE, sel))
    assert_outcome(env, sel, f"se_step_agent_replay world {w}")
    np.testing.assert_array_equal(tape["used"], z["used"][sel])
    env.close()


# ---------------------------------------------------------------- production draws against the oracle
def _oracle(O, w, sel):
    st = O.OracleState(len(sel))
    for f, v in S.pre_state(sel).items():
        getattr(st, f)[:] = v
    return O.OracleWorld(*S.world(w)), st


def _assert_vs_oracle(env, st, what):
    got = get_state(env)
    for f in S.FIELDS:
        if f == "fuel":
            np.testing.assert_array_equal(got[f].view(np.int64), st.fuel.view(np.int64), err_msg=f"{what}: fuel bits")
        else:
            np.testing.assert_array_equal(got[f], getattr(st, f), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(env.reward.cpu().numpy(), st.reward.astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(env.done.cpu().numpy().astype(np.int32), st.done, err_msg=what)
    np.testing.assert_array_equal(env.err.cpu().numpy().astype(np.int32), st.err, err_msg=what)


def _cases():
    # auto-reset needs two ports to draw a destination from (se_create refuses fewer)
    return [(w, auto) for w in WORLDS for auto in (False, True) if not auto or len(S.world(w)[1]) >= 2]


@pytest.mark.parametrize("w,auto", _cases())
def test_step_typed_matches_oracle_on_edges(oracle_mod, w, auto):
    O = oracle_mod
    z = S.fixture()
    sel = S.records(w)
    env = make_env(w, sel, seed=SEED, auto_reset=auto)
    env.set_counters(T0, 0)
    world, st = _oracle(O, w, sel)
    env.step_typed(z["act_type"][sel], z["act_a"][sel], z["act_b"][sel])
    O.step(world, st, act_type=z["act_type"][sel], act_a=z["act_a"][sel], act_b=z["act_b"][sel], seed=SEED, t=T0)
    if auto:
        S.philox_autoreset(O, world, st, SEED, T0)
    _assert_vs_oracle(env, st, f"se_step_typed world {w} auto {auto}")
    if w in (3, 4) and not auto:  # the draws reached every branch
        assert st.done.sum() > 0 and (st.err == 0).sum() > 1000
    env.close()


@pytest.mark.parametrize("w,auto", [c for c in _cases() if c[0] in WITH_PORTS])
def test_step_and_step_seq_match_oracle_on_edges(oracle_mod, w, auto):
    """The agent-expressible records through se_step, and through a two-step se_step_seq (without
    auto-reset: a state-only step, then a full one) against two oracle steps."""
    O = oracle_mod
    z = S.fixture()
    sel = S.records(w, S.agent_expressible())
    idx = z["agent_idx"][sel]

    def ostep(world, st, acts, t):
        if auto:
            O.step_autoreset(world, st, acts, seed=SEED, t=t)
        else:
            O.step(world, st, actions=acts, seed=SEED, t=t)

    env = make_env(w, sel, seed=SEED, auto_reset=auto)
    env.set_counters(T0, 0)
    world, st = _oracle(O, w, sel)
    env.step(idx)
    ostep(world, st, idx, T0)
    _assert_vs_oracle(env, st, f"se_step world {w} auto {auto}")
    env.close()

    n = len(sel)
    ld = (n + 3) // 4 * 4
    rows = torch.zeros((2, ld), dtype=torch.int32, device="cuda")
    second = np.roll(idx, 1)
    rows[0, :n] = torch.from_numpy(idx).cuda()
    rows[1, :n] = torch.from_numpy(second).cuda()
    env = make_env(w, sel, seed=SEED, auto_reset=auto)
    env.set_counters(T0, 0)
    world, st = _oracle(O, w, sel)
    env.step_seq(rows[:, :n])
    ostep(world, st, idx, T0)
    ostep(world, st, second, T0 + 1)
    _assert_vs_oracle(env, st, f"se_step_seq world {w} auto {auto}")
    assert env.counters[0] == T0 + 2
    env.close()
