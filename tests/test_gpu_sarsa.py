"""se_sarsa_step / se_sarsa_choose / VecSARSAAgent against the Philox-driver restatement of the
reference's SARSA step (tests/sarsa_support.py), bit for bit: the env state, the pending
action, the episode counters, every per-call output and the whole table. tests/test_sarsa_cpu.py
shows the restatement equal to the reference itself on a recorded session. The worlds are the
hand-made ones of tests/rollout_support.py."""
import ctypes as C

import numpy as np
import pytest

import rollout_support as RS
import sarsa_support as SS
from rollout_support import MANY, ONE, OPEN, SHARED
from test_gpu_rollout import load_state, oracle_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

SEED = 13


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def ship(cell, origin, dest, cargo=0, fuel=100.0):
    return (cell[0], cell[1], fuel, cargo, origin, dest)


def ships_state(ships):
    st = O.OracleState(len(ships))
    for i, sh in enumerate(ships):
        st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = sh
    return st


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


class Pair:
    """A VecSARSAAgent on a VecEnv and the restatement beside it, from the same ships."""

    def __init__(self, world, ships, env_id_base=0, dense=None, **kw):
        from shippingenv_amd.sarsa import VecSARSAAgent

        self.world, self.ow = world, world.oracle(O)
        self.env = world.env(len(ships), seed=SEED, env_id_base=env_id_base)
        load_state(self.env, ships_state(ships))
        kw.setdefault("max_steps", 0)
        self.agent = VecSARSAAgent(self.env, **kw)
        self.layout = SS.Layout(self.ow)
        assert (self.agent.rows, self.agent.A, self.agent.cmax) == (self.layout.rows, self.layout.A, self.layout.cmax)
        if dense is not None:
            self.agent.q.view(-1).copy_(torch.as_tensor(dense, device=self.env.device))
        self.learner = SS.Learner(self.ow, lr=self.agent.lr, gamma=self.agent.gamma, max_steps=self.agent.max_steps,
                                  max_attempts=self.agent.max_attempts, dense=dense)
        self.envs = [SS.Env(sh) for sh in ships]
        self.driver = SS.PhiloxDriver(O, self.ow, SEED, env_id_base)
        self.outs = []  # the restatement's outputs, step by step

    def set_q(self, ship_, action, value):
        """One entry of both tables."""
        key = (SS.discretize(ship_), action)
        self.learner.q[key] = value
        self.agent.q.view(-1)[self.layout.entry(key)] = value

    def step(self, eps, learn=True, what=""):
        t = self.agent.t
        reward, ended, status = self.agent.step(learn=learn, epsilon=eps)
        want = self.learner.vector_step(self.envs, eps, learn, self.driver, t)
        self.outs.append(want)
        tag = f"{what} step {t}"
        got = {k: v.cpu().numpy() for k, v in (("reward", reward), ("ended", ended), ("status", status),
                                               ("fin_return", self.agent.fin_return), ("fin_len", self.agent.fin_len))}
        np.testing.assert_array_equal(got["status"], [o["status"] for o in want], err_msg=f"{tag}: status")
        np.testing.assert_array_equal(got["ended"], [int(o["ended"]) for o in want], err_msg=f"{tag}: ended")
        np.testing.assert_array_equal(bits(got["reward"]), bits([o["reward"] for o in want]), err_msg=f"{tag}: reward")
        np.testing.assert_array_equal(bits(got["fin_return"]), bits([o["fin_return"] for o in want]),
                                      err_msg=f"{tag}: fin_return")
        np.testing.assert_array_equal(got["fin_len"], [o["fin_len"] for o in want], err_msg=f"{tag}: fin_len")
        self.check_state(tag)
        return want

    def check_state(self, tag):
        st, a, envs = oracle_state(self.env), self.agent, self.envs
        for k, f in enumerate(("x", "y", "fuel", "cargo", "origin", "dest")):
            g, w = getattr(st, f), np.array([e.ship[k] for e in envs])
            if f == "fuel":
                g, w = bits(g), bits(w)
            np.testing.assert_array_equal(g, w, err_msg=f"{tag}: {f}")
        fresh = np.array([e.fresh for e in envs])
        np.testing.assert_array_equal(a.fresh.cpu().numpy() != 0, fresh, err_msg=f"{tag}: fresh")
        np.testing.assert_array_equal(a.ep_len.cpu().numpy(), [e.ep_len for e in envs], err_msg=f"{tag}: ep_len")
        np.testing.assert_array_equal(bits(a.ep_return.cpu().numpy()), bits([e.ep_return for e in envs]),
                                      err_msg=f"{tag}: ep_return")
        pend = np.stack([a.type.cpu().numpy(), a.a.cpu().numpy(), a.b.cpu().numpy()], 1)
        for i, e in enumerate(envs):  # a fresh env's pending action is chosen anew: not compared
            if not e.fresh:
                assert tuple(pend[i]) == e.pending, f"{tag}: env {i} pending {tuple(pend[i])} != {e.pending}"

    def dense_table(self):
        """The restatement's table as the flat array of the layout."""
        t = np.zeros(self.layout.rows * self.layout.A) if self.learner.dense is None else np.array(self.learner.dense)
        for key, v in self.learner.q.items():
            t[self.layout.entry(key)] = v
        return t

    def check_table(self, what=""):
        got = self.agent.q.view(-1).cpu().numpy()
        want = self.dense_table()
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"{what}: {bad.size} table entries differ, the first {self.layout.key(int(bad[0]))}: " \
                              f"{got[bad[0]]!r} != {want[bad[0]]!r}"

    def close(self):
        self.agent.close()
        self.env.close()


def seen(pair, field, value):
    return sum(1 for outs in pair.outs for o in outs if o[field] == value)


# ----------------------------------------------------------------- one env: the reference itself
@pytest.mark.parametrize("eps", [1.0, 0.5, 0.0])
def test_single_env_300_steps(eps):
    """n = 1 on OPEN from fuel 3: the first episode runs dry within a few moves (done, restart,
    a fresh first choice), and max_steps = 40 cuts the later ones."""
    p = Pair(OPEN, [ship((3, 3), 0, 1, fuel=3.0)], max_steps=40)
    if eps == 0.0:  # an untouched table answers SELECT 0 for ever: prefer a move where the ship starts
        p.set_q(p.envs[0].ship, (SS.MOVE, 0, 1), 0.5)
    for _ in range(300):
        p.step(eps, what=f"eps {eps}")
    p.check_table(f"eps {eps}")
    assert seen(p, "ended", True) >= 7
    assert any(o["ended"] and o["status"] == SS.OK and 0 < o["fin_len"] < 40 for outs in p.outs for o in outs), \
        "no episode ended by done"
    assert len(p.learner.q) > (3 if eps == 0.0 else 20)
    assert (p.learner.explored > 0) == (eps > 0.0)
    p.close()


# ----------------------------------------------------------------- a ragged wave
@pytest.mark.parametrize("name", ["open", "shared"])
def test_ragged_wave_60_steps(name):
    """n = 67 = one wave and three envs, env_id_base != 0, every hand-placed ship of the MCTS
    scenarios in turn: ports with and without destination, the empty port, a corner, low fuel,
    cargo aboard. Epsilon 0.5, so the envs meet on the ports' rows and some updates collide."""
    import mcts_support as MS

    world, rows = MS.SCENARIOS[name]
    base = [r[1] for r in rows]
    ships = [base[i % len(base)] for i in range(67)]
    p = Pair(world, ships, env_id_base=(1 << 33) + 64, max_steps=25)
    for _ in range(60):
        p.step(0.5, what=name)
    p.check_table(name)
    statuses = {o["status"] for outs in p.outs for o in outs}
    assert SS.OK in statuses and (name != "open" or SS.RAISED in statuses)
    assert p.learner.collisions > 0, "no two envs updated one entry in one step"
    assert seen(p, "ended", True) > 67
    p.close()


# ----------------------------------------------------------------- many envs, one entry
def crowd(n, env_id_base):
    """n envs in one state, loaded (the cargo-loss draws make their rewards differ), all greedy
    on one preferred move: every update of a step goes to one entry."""
    sh = ship((3, 4), 0, 1, cargo=30)
    p = Pair(OPEN, [sh] * n, env_id_base=env_id_base)
    p.set_q(sh, (SS.MOVE, 0, -1), 1.0)
    key = (SS.discretize(sh), (SS.MOVE, 0, -1))
    out = p.step(0.0, what=f"crowd {n}")
    p.check_table(f"crowd {n}")
    assert p.learner.collisions == n - 1
    rewards = [o["reward"] for o in out]
    assert len(set(rewards)) > 1 and any(r != rewards[0] for r in rewards[1:]), "the envs' updates do not differ"
    mine = 1.0 + p.agent.lr * (rewards[0] + p.agent.gamma * 0.0 - 1.0)  # env 0's: the new row is untouched
    stored = float(p.agent.q.view(-1)[p.layout.entry(key)].item())
    assert stored == p.learner.q[key] == mine
    p.close()
    return stored, rewards


@pytest.mark.parametrize("n", [4, 130])
def test_every_env_on_one_entry_lowest_index_wins(n):
    crowd(n, 0)


def test_the_winner_is_the_lowest_local_index():
    """Global envs 4..7 as locals 4..7 of a batch of 8 lose to local 0; as locals 0..3 of a
    batch at env_id_base 4 the same draws make global env 4 the winner."""
    whole, rw = crowd(8, 0)
    part, rp = crowd(4, 4)
    assert rp == rw[4:8]  # the same envs, the same draws
    assert rw[0] != rw[4] and whole != part


# ----------------------------------------------------------------- cuts and raises
def test_max_steps_cut():
    p = Pair(SHARED, [ship((4, 2), 0, 2)] * 5, max_steps=3)  # every port stocks cargo: no sample raises
    for k in range(7):
        out = p.step(1.0, what="max_steps")
        if k in (2, 5):
            assert all(o["ended"] and o["fin_len"] == 3 and o["status"] == SS.OK for o in out)
        else:
            assert not any(o["ended"] for o in out)
    p.check_table("max_steps")
    p.close()


def test_max_attempts_cut_at_a_corner():
    """max_attempts = 1 and a preferred move that leaves the map: CUT, a restart, no write."""
    sh = ship((0, 0), 0, 1)
    p = Pair(OPEN, [sh] * 3, max_attempts=1)
    p.set_q(sh, (SS.MOVE, 0, -1), 2.0)
    before = p.agent.q.clone()
    out = p.step(0.0, what="corner")
    assert all(o["status"] == SS.CUT and o["ended"] and o["fin_len"] == 0 for o in out)
    assert torch.equal(p.agent.q.view(torch.int64), before.view(torch.int64))
    for _ in range(3):  # the restarted envs go on as fresh ones
        p.step(0.0, what="corner")
    p.check_table("corner")
    p.close()


def test_retry_until_a_sampled_step_goes_through():
    """The same corner with attempts to spare: the key updated is the chosen move, not the
    sampled one that was stepped."""
    sh = ship((0, 0), 0, 1)
    p = Pair(OPEN, [sh] * 64, max_attempts=8)
    p.set_q(sh, (SS.MOVE, 0, -1), 2.0)
    out = p.step(0.0, what="retry")
    assert {o["status"] for o in out} <= {SS.OK, SS.CUT}  # two of the four sampled moves stay on the map
    assert sum(o["status"] == SS.OK for o in out) > 32
    key = (SS.discretize(sh), (SS.MOVE, 0, -1))
    assert p.learner.q[key] != 2.0
    p.check_table("retry")
    p.close()


@pytest.mark.parametrize("world,sh,status", [
    (OPEN, ship((5, 2), 0, 1), SS.RAISED),           # cargo 0 on the port without stock: randint(1, 0)
    (ONE, ship((2, 3), 0, SS.NONE), SS.NEVER_RETURNS),  # no other port to select
], ids=["raised", "never_returns"])
def test_raising_sample_action_restarts_and_writes_nothing(world, sh, status):
    p = Pair(world, [sh] * 5)
    out = p.step(1.0, what="raise")
    assert all(o["status"] == status and o["ended"] and o["fin_len"] == 0 and o["reward"] == 0.0 for o in out)
    assert not p.learner.q and int(torch.count_nonzero(p.agent.q)) == 0
    for _ in range(4):
        p.step(1.0, what="raise")
    p.check_table("raise")
    p.close()


def test_learn_0_leaves_the_table_bytes_unchanged():
    lay = SS.Layout(OPEN.oracle(O))
    dense = np.random.default_rng(3).normal(size=lay.rows * lay.A)
    import mcts_support as MS

    base = [r[1] for r in MS.SCENARIOS["open"][1]]
    p = Pair(OPEN, [base[i % len(base)] for i in range(67)], dense=dense, max_steps=6)
    before = p.agent.q.clone()
    for _ in range(12):
        p.step(0.3, learn=False, what="learn=0")
    assert torch.equal(p.agent.q.view(torch.int64), before.view(torch.int64))
    assert not p.learner.q
    acts = {e.pending[0] for e in p.envs if not e.fresh}
    assert len(acts) >= 2  # the random table makes the greedy choices differ
    p.close()


# ----------------------------------------------------------------- choose_action alone
def test_choose_at_every_fuel_class_boundary_and_past_20_in_stock():
    """A random table; ships at sea and on a port that stocks 25 cargo and 30 fuel, at both sides
    of every fuel-class boundary. Amounts past 20 are in the table (sample_action reaches them)
    but not in the greedy scan: a huge value there is not chosen."""
    world = RS.World(7, 9, ports=[(1, 1), (5, 6), (3, 7)], fuel=[30, 4, 7], cargo=[25, 6, 8])
    lay = SS.Layout(world.oracle(O))
    assert lay.cmax == 25
    dense = np.random.default_rng(5).normal(size=lay.rows * lay.A)
    fuels = [0.0, 9.99, 10.0, 19.99, 20.0, 29.99, 30.0, 39.99, 40.0, 59.99, 60.0, 79.99, 80.0, 200.0, -0.5]
    ships = [ship(cell, 0, dest, fuel=f) for f in fuels for cell, dest in (((3, 3), 1), ((1, 1), 1), ((1, 1), SS.NONE))]
    for sh in ships:
        if (sh[0], sh[1]) == (1, 1):
            for m in (21, 25):
                dense[lay.entry((SS.discretize(sh), (SS.TAKE_CARGO, m, 0)))] = 100.0
    p = Pair(world, ships, dense=dense)
    for eps in (0.0, 0.5):
        got = np.stack([v.cpu().numpy() for v in p.agent.choose_action(epsilon=eps)], 1)
        for i, sh in enumerate(ships):
            p.driver.begin(i, p.agent.t)
            want = p.learner.choose(sh, eps, p.driver, "first")
            assert tuple(got[i]) == want, f"eps {eps} ship {sh}: {tuple(got[i])} != {want}"
            assert not (want[0] == SS.TAKE_CARGO and want[1] > 20 and eps == 0.0)
    greedy = {tuple(r) for r in np.stack([v.cpu().numpy() for v in p.agent.choose_action(epsilon=0.0)], 1)}
    assert {a[0] for a in greedy} >= {SS.MOVE, SS.SELECT} and len(greedy) > 8
    p.check_state("choose changes nothing")
    p.close()


# ----------------------------------------------------------------- the largest table
def test_many_ports_once():
    """MANY (P = 64), n = 64, 5 steps: 3.7e8 entries. The table is compared through its
    non-zero entries."""
    from shippingenv_amd import _native as N

    ships = [ship((1 + i // 11, 1 + i % 11), i, (i * 7 + 3) % 64 if i % 3 else SS.NONE, fuel=200.0 - i) for i in range(64)]
    try:
        p = Pair(MANY, ships)
    except (N.ShipEnvError, torch.cuda.OutOfMemoryError) as e:
        if "memory" in str(e).lower():
            pytest.skip(f"no room for the P = 64 table: {e}")
        raise
    for _ in range(5):
        p.step(0.5, what="many")
    flat = p.agent.q.view(-1)
    idx = torch.nonzero(flat).view(-1)
    got = dict(zip(idx.cpu().tolist(), bits(flat[idx].cpu().numpy()).tolist()))
    want = {p.layout.entry(k): int(bits([v])[0]) for k, v in p.learner.q.items() if v != 0.0}
    assert got == want and len(want) > 50
    # q_items speaks the reference's keys: a move's value is its (dx, dy), any other's its number
    assert set(p.agent.q_items()) == {(st, (a[0], (a[1], a[2]) if a[0] == SS.MOVE else a[1]))
                                      for (st, a), v in p.learner.q.items() if v != 0.0}
    p.close()


# ----------------------------------------------------------------- the interface
def test_create_refusals_and_the_empty_batch():
    from shippingenv_amd import _native as N
    from shippingenv_amd.sarsa import VecSARSAAgent

    lib = N.lib()
    # n = 0: everything is a no-op
    empty = OPEN.env(0)
    agent = VecSARSAAgent(empty)
    assert all(v.numel() == 0 for v in agent.step()) and all(v.numel() == 0 for v in agent.choose_action())
    agent.close()
    empty.close()
    # P = 0
    bare = RS.World(5, 6, ports=[], fuel=[], cargo=[])
    env0 = bare.env(4)
    h = C.c_void_p()
    assert lib.se_sarsa_create(C.byref(h), env0._h, 1 << 40) == -1 and not h.value
    assert b"port" in lib.se_last_error()
    env0.close()
    # max_table_bytes too small: the message names the bytes needed
    env = OPEN.env(8, seed=SEED)
    lay = SS.Layout(OPEN.oracle(O))
    need = lay.rows * lay.A * 12
    assert lib.se_sarsa_create(C.byref(h), env._h, need - 1) == -1 and not h.value
    assert str(need).encode() in lib.se_last_error()
    with pytest.raises(N.ShipEnvError, match=str(need)):
        VecSARSAAgent(env, max_table_bytes=need - 1)
    assert lib.se_sarsa_create(None, env._h, need) == -1 and lib.se_sarsa_create(C.byref(h), None, need) == -1
    agent = VecSARSAAgent(env, max_table_bytes=need)
    # argument errors of the step
    out = [C.c_void_p(t.data_ptr()) for t in (agent.reward, agent.ended, agent.status, agent.fin_return, agent.fin_len)]

    def call(lr=0.1, gamma=0.9, eps=0.5, learn=1, ms=10, ma=8, outs=out, handle=agent._h):
        return lib.se_sarsa_step(handle, lr, gamma, eps, learn, ms, ma, 0, *outs, env._stream())

    for kw in (dict(lr=float("nan")), dict(gamma=float("nan")), dict(eps=float("nan")), dict(ms=-1), dict(ma=0),
               dict(ma=N.SARSA_MAX_ATTEMPTS + 1), dict(handle=None), dict(outs=[None] + out[1:]),
               dict(outs=out[:4] + [None])):
        assert call(**kw) == -1, kw
    step0 = env.counters[0]
    assert call(ma=N.SARSA_MAX_ATTEMPTS) == 0 and env.counters[0] == step0 + 1
    # se_set_ports: the layout is stale
    env.set_ports(OPEN.ports, OPEN.fuel_stock, [5, 6, 8, 30])
    assert call() == -3 and b"stale" in lib.se_last_error()
    ty = torch.zeros(env.n, dtype=torch.int32, device=env.device)
    assert lib.se_sarsa_choose(agent._h, 0.0, 0, *[C.c_void_p(ty.data_ptr())] * 3, env._stream()) == -3
    with pytest.raises(N.ShipEnvError):
        agent._bind()
    torch.cuda.synchronize()
    agent.close()
    env.close()


def test_agent_train_test_policy_save_load(tmp_path):
    """The Python surface on the default world is out of a test's size; OPEN stands in: train
    counts episodes and decays once per n of them, test_policy leaves the table alone, save /
    load round-trip the table and hyperparameters, q_items speaks the reference's keys."""
    from shippingenv_amd.sarsa import VecSARSAAgent

    env = OPEN.env(32, seed=SEED)
    env.reset()
    agent = VecSARSAAgent(env, max_steps=20)
    episodes, _ = agent.train(100, sync_every=25)
    assert episodes >= 32 * 4 and agent.t == 100
    decays = episodes // 32
    want = 1.0
    for _ in range(decays):
        want = max(0.0001, want * 0.999)
    assert agent.epsilon == want and agent._carry == episodes % 32
    before = agent.q.clone()
    means = agent.test_policy(40)
    assert torch.equal(agent.q.view(torch.int64), before.view(torch.int64))
    assert means and set(means) <= set(range(OPEN.P))
    items = agent.q_items()
    assert len(items) == int(torch.count_nonzero(agent.q))
    (state, action), _ = next(iter(items.items()))
    assert len(state) == 5 and len(state[0]) == 2 and action[0] in (1, 2, 3, 4)
    path = str(tmp_path / "sarsa.pt")
    agent.save(path)
    other = VecSARSAAgent(env, max_steps=20)
    other.load(path)
    assert torch.equal(other.q.view(torch.int64), agent.q.view(torch.int64)) and other.epsilon == agent.epsilon
    for a in (other, agent):
        a.close()
    env.close()
