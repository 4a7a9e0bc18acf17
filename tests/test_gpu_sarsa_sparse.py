"""The sparse SARSA table (se_sarsa_create_sparse, VecSARSAAgent(table="sparse")) against the
Philox-driver restatement of the reference's SARSA step (tests/sarsa_support.py) and against
the dense kind, bit for bit: every per-step output, the env state, the pending actions, the
episode counters and the table as a map {entry: value bits}. Where a row lies in the table is
not compared (it may depend on timing); that the table is a valid one is, after every learning
step (tests/sparse_sarsa_support.py: distinct keys in range, every key reachable from its home
before an empty slot, idle pages zero, `used` the occupied count)."""
import ctypes as C

import numpy as np
import pytest

import footprint_support as F
import mcts_support as MS
import rollout_support as RS
import sarsa_support as SS
import sparse_sarsa_support as SP
from conftest import golden_water
from rollout_support import MANY, OPEN
from test_gpu_rollout import load_state
from test_gpu_sarsa import Pair, bits, seen, ship, ships_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

SEED = 13
BASE = (1 << 33) + 64  # the ragged wave's env_id_base
i32, u8, f64, i64 = np.int32, np.uint8, np.float64, np.int64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def lib():
    from shippingenv_amd import _native as N

    return N.lib()


def sparse_agent(env, **kw):
    from shippingenv_amd.sarsa import VecSARSAAgent

    return VecSARSAAgent(env, table="sparse", **kw)


def pull(agent):
    """The agent's table on the host."""
    torch.cuda.synchronize()
    return agent.keys.cpu().numpy(), agent.pages.cpu().numpy()


def push(agent, table):
    """A restatement table (of the agent's capacity) into the agent's buffers; the bind counts it."""
    assert table.capacity == agent.capacity and table.A == agent.A
    agent.keys.copy_(torch.from_numpy(table.keys))
    agent.pages.copy_(torch.from_numpy(table.pages))
    agent._bind()


def valid_map(agent, rows):
    """The validity check, then the table as a map, and its stats."""
    st = agent.stats()
    keys, pages = pull(agent)
    SP.check_valid(keys, pages, rows, used=st["used"])
    return SP.as_map(keys, pages), st


class SparsePair(Pair):
    """test_gpu_sarsa.Pair with a sparse agent: its step() compares the outputs, the env state, the
    pending actions and the episode counters; here every learning step also holds the table to
    the validity check and, as a map, to the restatement's. preload: a restatement Table the
    agent starts from; dense: the same content as the flat array the restatement reads."""

    def __init__(self, world, ships, env_id_base=0, capacity=None, preload=None, dense=None, **kw):
        self.world, self.ow = world, world.oracle(O)
        self.env = world.env(len(ships), seed=SEED, env_id_base=env_id_base)
        load_state(self.env, ships_state(ships))
        kw.setdefault("max_steps", 0)
        self.agent = sparse_agent(self.env, capacity=capacity, **kw)
        self.layout = SS.Layout(self.ow)
        assert (self.agent.rows, self.agent.A, self.agent.cmax) == (self.layout.rows, self.layout.A, self.layout.cmax)
        held = ()
        if preload is not None:
            push(self.agent, preload)
            held = preload.keys[preload.keys != SP.EMPTY].tolist()
            assert self.agent.stats()["used"] == len(held)
        self.learner = SP.TrackingLearner(self.ow, held=held, lr=self.agent.lr, gamma=self.agent.gamma,
                                          max_steps=self.agent.max_steps, max_attempts=self.agent.max_attempts, dense=dense)
        self.envs = [SS.Env(sh) for sh in ships]
        self.driver = SS.PhiloxDriver(O, self.ow, SEED, env_id_base)
        self.outs = []
        self.check_tables = True

    def set_q(self, ship_, action, value):
        key = (SS.discretize(ship_), action)
        self.learner.q[key] = value
        keys, pages = pull(self.agent)
        t = SP.Table(self.agent.capacity, self.agent.A)
        t.keys[:], t.pages[:] = keys, pages
        row, slot = divmod(self.layout.entry(key), self.layout.A)
        assert t.set(row, slot, value)
        self.learner.held.add(row)
        push(self.agent, t)

    def step(self, eps, learn=True, what=""):
        want = super().step(eps, learn=learn, what=what)
        if learn and self.check_tables:
            self.check_table(f"{what} step {self.agent.t - 1}")
        return want

    def check_table(self, what=""):
        got, st = valid_map(self.agent, self.layout.rows)
        want = SP.learner_map(self.learner, self.layout)
        if got != want:
            bad = sorted(set(got) ^ set(want) | {e for e in set(got) & set(want) if got[e] != want[e]})
            raise AssertionError(f"{what}: {len(bad)} table entries differ, the first {self.layout.key(bad[0])}: "
                                 f"{got.get(bad[0])} != {want.get(bad[0])}")
        return st


def rows_of(learner):
    """The rows the restatement's table holds a key of (a key written 0.0 still took a page)."""
    return {learner.lay.entry(k) // learner.lay.A for k in learner.q}


# ----------------------------------------------------------------- 1. one env: the reference itself
@pytest.mark.parametrize("eps", [1.0, 0.5, 0.0])
def test_single_env_300_steps(eps):
    """n = 1 on OPEN from fuel 3, as the dense test: 300 steps write at most 300 rows."""
    p = SparsePair(OPEN, [ship((3, 3), 0, 1, fuel=3.0)], max_steps=40, capacity=1024)
    if eps == 0.0:  # an untouched table answers SELECT 0 for ever: prefer a move where the ship starts
        p.set_q(p.envs[0].ship, (SS.MOVE, 0, 1), 0.5)
    for _ in range(300):
        p.step(eps, what=f"eps {eps}")
    st = p.check_table(f"eps {eps}")
    assert st["dropped"] == 0 and st["used"] == len(p.learner.held) >= len(rows_of(p.learner)) and st["capacity"] == 1024
    assert seen(p, "ended", True) >= 7
    assert len(p.learner.q) > (3 if eps == 0.0 else 20)
    assert (p.learner.explored > 0) == (eps > 0.0)
    p.close()


# ----------------------------------------------------------------- 2, 3. a ragged wave
def wave_ships(name):
    world, rows = MS.SCENARIOS[name]
    base = [r[1] for r in rows]
    return world, [base[i % len(base)] for i in range(67)]


_SCOUT = {}


def scout(name):
    """The restatement alone over the ragged wave's 60 steps (once per world, left unchanged): what
    the run touches decides the capacity before the GPU has run."""
    if name not in _SCOUT:
        world, ships = wave_ships(name)
        ow = world.oracle(O)
        learner = SP.TrackingLearner(ow, max_steps=25)
        envs, driver = [SS.Env(sh) for sh in ships], SS.PhiloxDriver(O, ow, SEED, BASE)
        for t in range(60):
            learner.vector_step(envs, 0.5, True, driver, t)
        _SCOUT[name] = learner
    return _SCOUT[name]


@pytest.mark.parametrize("name", ["open", "shared"])
def test_ragged_wave_60_steps(name):
    """n = 67 at env_id_base 2^33 + 64, epsilon 0.5, max_steps 25, in a table of the smallest
    capacity >= twice the rows the run touches: nothing can be dropped."""
    world, ships = wave_ships(name)
    touched = scout(name).rows_written
    capacity = SP.pow2_at_least(2 * len(touched))
    p = SparsePair(world, ships, env_id_base=BASE, max_steps=25, capacity=capacity)
    for _ in range(60):
        p.step(0.5, what=name)
    st = p.check_table(name)
    assert st["dropped"] == 0 and st["used"] == len(touched) == len(p.learner.rows_written)
    assert p.learner.collisions > 0, "no two envs updated one entry in one step"
    assert p.learner.shared_inserts > 0, "no step inserted one new row from more than one env"
    assert seen(p, "ended", True) > 67
    p.close()


def rows_with_home(h, capacity, rows, count, skip=()):
    """The first `count` rows of the layout whose home bucket is h, by se_sarsa_sparse_home."""
    out = []
    for row in range(rows):
        if row not in skip and lib().se_sarsa_sparse_home(row, capacity) == h:
            out.append(row)
            if len(out) == count:
                return out
    raise AssertionError(f"fewer than {count} rows have the home {h}")


def state_of(lay, row, fuel_of_class=(5.0, 15.0, 25.0, 35.0, 50.0, 70.0, 90.0)):
    """A ship whose discretised state is the row."""
    ((x, y), _, _, origin, dest), _ = lay.key(row * lay.A)
    cls = (row // ((lay.P + 1) ** 2)) % 7
    return (x, y, fuel_of_class[cls], 0, origin, dest)


@pytest.mark.parametrize("name", ["open", "shared"])
def test_probe_chains_wrap_around_the_last_bucket(name):
    """The same run from a table the restatement built: three rows whose home is capacity - 2 and
    three whose home is capacity - 1, inserted in that order, lie in the slots capacity - 2,
    capacity - 1, 0, 1, 2, 3 and hold random pages. The run goes on as the restatement's from that
    table; afterwards ships put into those six states choose greedily what the restatement does
    (the values lie behind the wrap), and a state whose home is slot 0 but whose row is absent
    probes through the whole chain to SELECT 0."""
    world, ships = wave_ships(name)
    lay = SS.Layout(world.oracle(O))
    capacity = SP.pow2_at_least(2 * len(scout(name).rows_written))
    chain = rows_with_home(capacity - 2, capacity, lay.rows, 3) + rows_with_home(capacity - 1, capacity, lay.rows, 3)
    dense = np.zeros(lay.rows * lay.A)
    rng = np.random.default_rng(17)
    for row in chain:
        dense[row * lay.A:(row + 1) * lay.A] = rng.normal(size=lay.A)
    table = SP.from_dense(dense, lay.A, capacity, first=chain)
    assert [table.find(r) for r in chain] == [capacity - 2, capacity - 1, 0, 1, 2, 3]
    p = SparsePair(world, ships, env_id_base=BASE, max_steps=25, capacity=capacity, preload=table, dense=dense)
    for _ in range(60):
        p.step(0.5, what=f"{name} preloaded")
    st = p.check_table(f"{name} preloaded")
    assert st["dropped"] == 0 and st["used"] == len(p.learner.rows_written | set(chain))
    keys, _ = pull(p.agent)
    assert keys[[capacity - 2, capacity - 1, 0, 1, 2, 3]].tolist() == chain  # nothing moves a row
    # greedy choices from the chain's states, and from an absent row that has to pass the chain
    absent = rows_with_home(0, capacity, lay.rows, 1, skip=set(keys[keys >= 0].tolist()))[0]
    probes = [state_of(lay, r) for r in chain + [absent]]
    state = ships_state(probes + ships[len(probes):])
    load_state(p.env, state)
    got = np.stack([v.cpu().numpy() for v in p.agent.choose_action(epsilon=0.0)], 1)
    for i, sh in enumerate(probes):
        assert SS.discretize(sh) == lay.key((chain + [absent])[i] * lay.A)[0]
        p.driver.begin(i, p.agent.t)
        assert tuple(got[i]) == p.learner.choose(sh, 0.0, p.driver, "first"), f"probe {i}"
    assert tuple(got[len(chain)]) == (SS.SELECT, 0, 0)
    assert len({tuple(g) for g in got[:len(chain)]}) > 1  # the random pages make the choices differ
    p.close()


# ----------------------------------------------------------------- 4. many envs, one new row
@pytest.mark.parametrize("n", [4, 130])
def test_every_env_inserts_one_new_row_lowest_index_wins(n):
    """n envs in one state with one pending move, loaded (the cargo-loss draws make their rewards
    differ): the row is new, every env's update goes to one entry of it in the same step."""
    sh = ship((3, 4), 0, 1, cargo=30)
    move = (SS.MOVE, 0, -1)
    p = SparsePair(OPEN, [sh] * n, capacity=64)
    for e in p.envs:
        e.pending, e.fresh = move, False
    a = p.agent
    a.type.fill_(move[0]), a.a.fill_(move[1]), a.b.fill_(move[2]), a.fresh.zero_()
    out = p.step(0.0, what=f"crowd {n}")
    st = p.agent.stats()
    assert st["used"] == 1 and st["dropped"] == 0
    assert p.learner.collisions == n - 1 and p.learner.shared_inserts == 1
    rewards = [o["reward"] for o in out]
    assert all(o["status"] == SS.OK for o in out) and len(set(rewards)) > 1 and any(r != rewards[0] for r in rewards[1:])
    key = (SS.discretize(sh), move)
    mine = 0.0 + a.lr * (rewards[0] + a.gamma * 0.0 - 0.0)  # env 0's: both rows are absent
    got, _ = valid_map(a, p.layout.rows)
    assert got == {p.layout.entry(key): int(bits([mine])[0])} and p.learner.q[key] == mine
    p.close()


# ----------------------------------------------------------------- 5, 6. the dense twin
STATE = ("x", "y", "fuel", "cargo", "origin", "dest")
LEARNER = ("type", "a", "b", "fresh", "ep_len", "ep_return")
OUTS = ("reward", "ended", "status", "fin_return", "fin_len")


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                      b.contiguous().view(torch.uint8))


def twins(n, capacity, **kw):
    from shippingenv_amd.sarsa import VecSARSAAgent

    envs = [OPEN.env(n, seed=SEED) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs, VecSARSAAgent(envs[0], **kw), sparse_agent(envs[1], capacity=capacity, **kw)


def assert_twins(envs, dense, sparse, what):
    for f in STATE:
        assert same_bytes(getattr(envs[0], f), getattr(envs[1], f)), f"{what}: {f}"
    for f in LEARNER + OUTS:
        assert same_bytes(getattr(dense, f), getattr(sparse, f)), f"{what}: {f}"
    assert same_bytes(dense.q, sparse.to_dense()), f"{what}: the table"


@pytest.mark.parametrize("grow", [False, True], ids=["fixed", "grow"])
def test_dense_twin_257_envs_40_steps(grow):
    """Two envs of equal seed, a dense and a sparse agent, epsilon 0.3. 257 envs write at most
    2570 rows in 10 steps: capacity 4096 holds steps 0..9, 8192 steps 10..19, and 65536 the
    layout's 11025 rows, so nothing is dropped whether the table grows (to twice at step 10, to
    eight times at step 20) or starts large. The buffers a grow leaves behind stay as they were."""
    envs, dense, sparse = twins(257, 4096 if grow else 16384)
    assert dense.rows == 11025
    left = []
    for t in range(40):
        if grow and t in (10, 20):
            old = (sparse.keys, sparse.pages)
            sparse.grow(sparse.capacity * (2 if t == 10 else 8))
            torch.cuda.synchronize()
            left.append((old, tuple(v.clone() for v in old)))
            assert sparse.keys is not old[0] and sparse.capacity == sparse.keys.numel() == (8192 if t == 10 else 65536)
            _, st = valid_map(sparse, sparse.rows)
            assert int((old[0] >= 0).sum()) == st["used"]
        for a in (dense, sparse):
            a.step(epsilon=0.3)
        assert_twins(envs, dense, sparse, f"step {t}")
    _, st = valid_map(sparse, sparse.rows)
    # a page is taken by an update that wrote 0.0 too
    assert st["dropped"] == 0 and st["used"] >= int((dense.q != 0).any(1).sum()) > 100
    assert len(left) == (2 if grow else 0)
    for old, copy in left:
        assert all(same_bytes(o, c) for o, c in zip(old, copy)), "a later step touched the buffers a grow left"
    for a in (dense, sparse):
        a.close()
    for e in envs:
        e.close()


# ----------------------------------------------------------------- 7. learn = 0
def test_learn_0_leaves_keys_and_pages_unchanged():
    """The random dense table of the dense test with every third row zeroed, as a sparse image
    (absent rows among the present ones): 12 steps at epsilon 0.3 change no byte of it."""
    lay = SS.Layout(OPEN.oracle(O))
    dense = np.random.default_rng(3).normal(size=lay.rows * lay.A)
    dense.reshape(lay.rows, lay.A)[::3] = 0.0
    table = SP.from_dense(dense, lay.A, 16384)
    assert table.used == lay.rows - len(range(0, lay.rows, 3))
    _, ships = wave_ships("open")
    p = SparsePair(OPEN, ships, capacity=16384, preload=table, dense=dense, max_steps=6)
    before = (p.agent.keys.clone(), p.agent.pages.clone())
    for _ in range(12):
        p.step(0.3, learn=False, what="learn=0")
    assert same_bytes(p.agent.keys, before[0]) and same_bytes(p.agent.pages, before[1])
    st = p.agent.stats()
    assert st["used"] == table.used and st["dropped"] == 0 and not p.learner.q
    acts = {e.pending[0] for e in p.envs if not e.fresh}
    assert len(acts) >= 2  # the random table makes the greedy choices differ
    p.close()


# ----------------------------------------------------------------- 8. choose_action alone
def test_choose_at_every_fuel_class_boundary_with_absent_rows():
    """The dense choose test's world, table and ships from a sparse image; the rows of the ships
    at sea with fuel >= 40 are zero, that is, absent: they answer SELECT 0 at epsilon 0."""
    world = RS.World(7, 9, ports=[(1, 1), (5, 6), (3, 7)], fuel=[30, 4, 7], cargo=[25, 6, 8])
    lay = SS.Layout(world.oracle(O))
    assert lay.cmax == 25
    dense = np.random.default_rng(5).normal(size=lay.rows * lay.A)
    fuels = [0.0, 9.99, 10.0, 19.99, 20.0, 29.99, 30.0, 39.99, 40.0, 59.99, 60.0, 79.99, 80.0, 200.0, -0.5]
    ships = [ship(cell, 0, dest, fuel=f) for f in fuels for cell, dest in (((3, 3), 1), ((1, 1), 1), ((1, 1), SS.NONE))]
    absent = [i for i, sh in enumerate(ships) if (sh[0], sh[1]) == (3, 3) and sh[2] >= 40.0]
    for i, sh in enumerate(ships):
        row = lay.entry((SS.discretize(sh), (SS.SELECT, 0, 0))) // lay.A
        if i in absent:
            dense[row * lay.A:(row + 1) * lay.A] = 0.0
        if (sh[0], sh[1]) == (1, 1):
            for m in (21, 25):
                dense[lay.entry((SS.discretize(sh), (SS.TAKE_CARGO, m, 0)))] = 100.0
    table = SP.from_dense(dense, lay.A, 8192)
    p = SparsePair(world, ships, capacity=8192, preload=table, dense=dense)
    held = set(table.keys[table.keys >= 0].tolist())
    assert len(absent) == 6 and all(lay.entry((SS.discretize(ships[i]), (SS.SELECT, 0, 0))) // lay.A not in held
                                    for i in absent)
    before = (p.agent.keys.clone(), p.agent.pages.clone())
    for eps in (0.0, 0.5):
        got = np.stack([v.cpu().numpy() for v in p.agent.choose_action(epsilon=eps)], 1)
        for i, sh in enumerate(ships):
            p.driver.begin(i, p.agent.t)
            want = p.learner.choose(sh, eps, p.driver, "first")
            assert tuple(got[i]) == want, f"eps {eps} ship {sh}: {tuple(got[i])} != {want}"
            assert not (want[0] == SS.TAKE_CARGO and want[1] > 20 and eps == 0.0)
            if eps == 0.0 and i in absent:
                assert want == (SS.SELECT, 0, 0)
    greedy = {tuple(r) for r in np.stack([v.cpu().numpy() for v in p.agent.choose_action(epsilon=0.0)], 1)}
    assert {a[0] for a in greedy} >= {SS.MOVE, SS.SELECT} and len(greedy) > 8
    p.check_state("choose changes nothing")
    assert same_bytes(p.agent.keys, before[0]) and same_bytes(p.agent.pages, before[1])
    p.close()


# ----------------------------------------------------------------- 9. a full table
def test_full_table_drops_counts_and_returns():
    """Capacity 64 and 130 ships in 130 distinct states at sea, bound for a port: the first step's
    updates go to more than 64 rows. 64 of them take the pages, the others are dropped and
    counted; keys and pages lie inside larger buffers whose margins stay as they were; the step's
    outputs and the env state are the restatement's, whose table the device's is a part of."""
    water = [(x, y) for x in range(7) for y in range(9) if (x, y) != (2, 5) and [x, y] not in OPEN.ports]
    ships = [ship(water[i % len(water)], i % 4, (i % 4 + 1 + i // len(water)) % 4, fuel=(95.0, 55.0, 35.0)[i // len(water)])
             for i in range(130)]
    assert len({SS.discretize(sh) for sh in ships}) == 130
    p = SparsePair(OPEN, ships, capacity=64)
    p.check_tables = False
    margin, A = 512, p.agent.A
    big_keys = torch.full((64 + 2 * margin,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=p.env.device)
    big_pages = torch.full(((64 + 2 * margin) * A,), 0x7FF8DEADBEEF0001, dtype=torch.int64, device=p.env.device)
    big_keys[margin:margin + 64] = -1
    big_pages[margin * A:(margin + 64) * A] = 0
    p.agent.keys = big_keys[margin:margin + 64]
    p.agent.pages = big_pages[margin * A:(margin + 64) * A].view(torch.float64).view(64, A)
    p.agent._bind()
    p.step(1.0, what="full table")  # returns: the probe is bounded by the capacity
    want_rows = p.learner.first_step_rows
    assert len(want_rows) > 64
    st = p.agent.stats()
    assert st["used"] == 64 and st["capacity"] == 64 and st["dropped"] >= len(want_rows) - 64 > 0
    torch.cuda.synchronize()
    for big, lo, hi, fill in ((big_keys, margin, margin + 64, 0x5A5A5A5A5A5A5A5A),
                              (big_pages, margin * A, (margin + 64) * A, 0x7FF8DEADBEEF0001)):
        assert bool((big[:lo] == fill).all()) and bool((big[hi:] == fill).all()), "a margin was written"
    keys, pages = pull(p.agent)
    SP.check_valid(keys, pages, p.layout.rows, used=64)
    assert set(keys.tolist()) <= want_rows
    got, want = SP.as_map(keys, pages), SP.learner_map(p.learner, p.layout)
    assert got and all(want.get(e) == b for e, b in got.items()), "an entry that is not the restatement's"
    held = set(keys.tolist())
    assert {e for e in want if e // A in held} == set(got)  # of the rows it holds it lost nothing
    p.close()


# ----------------------------------------------------------------- 10. many ports
def test_many_ports_without_a_memory_skip():
    """MANY (P = 64), the 64 ships of the dense test_many_ports_once, in a table of 1024 pages."""
    ships = [ship((1 + i // 11, 1 + i % 11), i, (i * 7 + 3) % 64 if i % 3 else SS.NONE, fuel=200.0 - i) for i in range(64)]
    p = SparsePair(MANY, ships, capacity=1024)
    for _ in range(5):
        p.step(0.5, what="many")
    st = p.check_table("many")
    assert st["dropped"] == 0 and st["bytes"] == 1024 * (p.agent.A * 12 + 8) < 2**21
    want = {(s, (a[0], (a[1], a[2]) if a[0] == SS.MOVE else a[1])) for (s, a), v in p.learner.q.items() if v != 0.0}
    assert set(p.agent.q_items()) == want and len(want) > 50
    assert {k: bits([v])[0] for k, v in p.agent.q_items().items()} == \
        {(s, (a[0], (a[1], a[2]) if a[0] == SS.MOVE else a[1])): bits([v])[0] for (s, a), v in p.learner.q.items() if v != 0.0}
    p.close()


def test_default_map_with_64_ports():
    """The 100 x 100 map with 64 water ports: 2.96e8 rows of 108 entries, 383 GB dense. 4096 envs
    take 20 learning steps at epsilon 1 in a table of 2^17 pages (20 * 4096 updates fit)."""
    from shippingenv_amd.vec import VecEnv, random_water_ports

    env = VecEnv(4096, ports=random_water_ports(golden_water(), 64, seed=3), seed=SEED)
    env.reset()
    agent = sparse_agent(env, capacity=1 << 17, max_table_bytes=1 << 30)
    assert (agent.rows, agent.A) == (100 * 100 * 7 * 65 * 65, 108)
    with pytest.raises(ValueError, match="max_table_bytes"):
        sparse_agent(env, capacity=1 << 17, max_table_bytes=(1 << 17) * (108 * 12 + 8) - 1)
    for _ in range(20):
        agent.step(epsilon=1.0)
    got, st = valid_map(agent, agent.rows)
    assert st["dropped"] == 0 and 4096 <= st["used"] <= 20 * 4096 and len(got) > 4096
    assert bool((agent.status == SS.OK).any())
    with pytest.raises(ValueError, match="max_table_bytes"):  # 255 GB
        agent.to_dense()
    agent.close()
    env.close()


# ----------------------------------------------------------------- 11. the interface
def test_refusals_the_empty_batch_and_stale_ports():
    from shippingenv_amd import _native as N
    from shippingenv_amd.sarsa import VecSARSAAgent

    L = lib()
    env = OPEN.env(8, seed=SEED)
    h = C.c_void_p()
    for capacity in (0, 63, 96, -64, 1 << 62):
        assert L.se_sarsa_create_sparse(C.byref(h), env._h, capacity) == -1 and not h.value, capacity
    assert b"capacity" in L.se_last_error() or b"overflow" in L.se_last_error()
    assert L.se_sarsa_create_sparse(None, env._h, 64) == -1 and L.se_sarsa_create_sparse(C.byref(h), None, 64) == -1
    bare = RS.World(5, 6, ports=[], fuel=[], cargo=[]).env(4)
    assert L.se_sarsa_create_sparse(C.byref(h), bare._h, 64) == -1 and b"port" in L.se_last_error()
    bare.close()
    for bad in (63, 96, 0):
        with pytest.raises(N.ShipEnvError):
            sparse_agent(env, capacity=bad)
    with pytest.raises(ValueError):
        VecSARSAAgent(env, table="hashed")
    with pytest.raises(ValueError):
        VecSARSAAgent(env, capacity=64)
    dense, sparse = VecSARSAAgent(env), sparse_agent(env, capacity=64)
    hundred = OPEN.env(100)
    by_default = sparse_agent(hundred)
    assert sparse.capacity == 64 and by_default.capacity == 512  # the smallest power of two >= 4 n
    by_default.close()
    hundred.close()
    st = C.byref(sparse._state)
    keys, pages = C.c_void_p(sparse.keys.data_ptr()), C.c_void_p(sparse.pages.data_ptr())
    # the wrong kind
    assert L.se_sarsa_bind(sparse._h, pages, st) == -1 and b"sparse" in L.se_last_error()
    assert L.se_sarsa_bind_sparse(dense._h, keys, pages, C.byref(dense._state)) == -1
    cap, used, dropped = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.se_sarsa_sparse_stats(dense._h, C.byref(cap), C.byref(used), C.byref(dropped), env._stream()) == -1
    assert L.se_sarsa_sparse_grow(dense._h, keys, pages, 64, env._stream()) == -1
    for call in (dense.grow, ):
        with pytest.raises(ValueError):
            call()
    # null buffers and handles
    assert L.se_sarsa_bind_sparse(sparse._h, None, pages, st) == -1 and L.se_sarsa_bind_sparse(sparse._h, keys, None, st) == -1
    assert L.se_sarsa_bind_sparse(sparse._h, keys, pages, None) == -1 and L.se_sarsa_bind_sparse(None, keys, pages, st) == -1
    assert L.se_sarsa_sparse_stats(None, None, None, None, env._stream()) == -1
    assert L.se_sarsa_sparse_stats(sparse._h, None, None, None, env._stream()) == 0
    assert L.se_sarsa_sparse_grow(sparse._h, None, pages, 128, env._stream()) == -1
    assert L.se_sarsa_sparse_grow(sparse._h, keys, None, 128, env._stream()) == -1
    for capacity in (0, 96, -128):
        assert L.se_sarsa_sparse_grow(sparse._h, keys, pages, capacity, env._stream()) == -1
    # grow to less than the rows held need
    env.reset()
    for _ in range(7):  # 8 envs: at most 56 rows
        sparse.step(epsilon=1.0)
    held = sparse.stats()
    assert held["dropped"] == 0 and 56 >= held["used"] > 0
    big = sparse_agent(env, capacity=256)
    hundred = SP.Table(256, big.A)
    for row in range(100):
        assert hundred.set(row * 97, row % big.A, 1.0 + row)
    push(big, hundred)
    assert big.stats()["used"] == 100
    with pytest.raises(N.ShipEnvError, match="100 rows"):
        big.grow(64)
    assert big.capacity == 256 and big.stats()["capacity"] == 256
    before, _ = valid_map(big, big.rows)
    big.grow(128)  # smaller, and room for the 100: legal
    after, st2 = valid_map(big, big.rows)
    assert after == before == SP.as_map(hundred.keys, hundred.pages) and st2["used"] == 100 and st2["capacity"] == 128
    # se_set_ports: the layout is stale, through every new call
    env.set_ports(OPEN.ports, OPEN.fuel_stock, [5, 6, 8, 30])
    assert L.se_sarsa_bind_sparse(sparse._h, keys, pages, st) == -3 and b"stale" in L.se_last_error()
    assert L.se_sarsa_sparse_stats(sparse._h, C.byref(cap), C.byref(used), C.byref(dropped), env._stream()) == -3
    assert L.se_sarsa_sparse_grow(sparse._h, keys, pages, 128, env._stream()) == -3
    with pytest.raises(N.ShipEnvError):
        sparse.step()
    with pytest.raises(N.ShipEnvError):
        sparse.choose_action()
    torch.cuda.synchronize()
    for a in (dense, sparse, big):
        a.close()
    env.close()
    # n = 0: every call is a no-op
    empty = OPEN.env(0)
    agent = sparse_agent(empty)
    assert agent.capacity == 64
    assert all(v.numel() == 0 for v in agent.step()) and all(v.numel() == 0 for v in agent.choose_action())
    assert agent.stats() == {"table": "sparse", "capacity": 64, "used": 0, "dropped": 0, "bytes": 64 * (agent.A * 12 + 8)}
    agent.grow()
    assert agent.stats()["capacity"] == 128 and agent.q_items() == {} and int(torch.count_nonzero(agent.to_dense())) == 0
    assert agent.train(3) == (0, 0.0)
    agent.close()
    empty.close()


def test_save_and_load_between_the_kinds(tmp_path):
    from shippingenv_amd.sarsa import VecSARSAAgent

    env = OPEN.env(32, seed=SEED)
    env.reset()
    sparse = sparse_agent(env, capacity=4096, max_steps=20)
    for _ in range(60):
        sparse.step(epsilon=0.7)
    sparse.epsilon = 0.25
    table, st = valid_map(sparse, sparse.rows)
    assert st["dropped"] == 0 and len(table) > 100
    path = str(tmp_path / "sparse.pt")
    sparse.save(path)
    # sparse -> sparse, into a table of another capacity (it grows to hold the rows below half load)
    other = sparse_agent(env, capacity=64, max_steps=20)
    other.load(path)
    got, st2 = valid_map(other, other.rows)
    assert got == table and st2["used"] == st["used"] and 2 * st2["used"] <= st2["capacity"] and other.epsilon == 0.25
    # sparse -> dense
    dense = VecSARSAAgent(env, max_steps=20)
    dense.load(path)
    assert SP.dense_map(dense.q.view(-1).cpu().numpy()) == table and dense.epsilon == 0.25
    assert dense.q_items() == sparse.q_items() and len(sparse.q_items()) == len(table)
    # dense -> sparse: the rows with a non-zero entry
    dpath = str(tmp_path / "dense.pt")
    dense.save(dpath)
    third = sparse_agent(env, capacity=64, max_steps=20)
    third.load(dpath)
    got, st3 = valid_map(third, third.rows)
    assert got == table and st3["used"] == len({e // third.A for e in table})
    assert same_bytes(third.to_dense(), dense.q)
    # the loaded learners go on alike
    for a in (sparse, other, third):
        a.t = 100
    acts = [torch.stack(a.choose_action(epsilon=0.0)) for a in (sparse, other, third, dense)]
    dense.t = 100
    acts[3] = torch.stack(dense.choose_action(epsilon=0.0))
    assert all(torch.equal(acts[0], x) for x in acts[1:])
    for a in (sparse, other, third, dense):
        a.close()
    env.close()


def test_train_grows_by_itself_to_the_dense_twins_table():
    envs, dense, sparse = twins(32, 64, max_steps=20)
    assert sparse.capacity == 64
    got_d, got_s = dense.train(100, sync_every=25), sparse.train(100, sync_every=25)
    assert got_d == got_s and got_d[0] >= 32 * 4 and dense.epsilon == sparse.epsilon and dense.t == sparse.t == 100
    _, st = valid_map(sparse, sparse.rows)
    assert st["dropped"] == 0 and st["capacity"] > 64 and 2 * st["used"] <= st["capacity"]
    assert_twins(envs, dense, sparse, "after train")
    before = (sparse.keys.clone(), sparse.pages.clone())
    assert dense.test_policy(30) == sparse.test_policy(30)
    assert same_bytes(sparse.keys, before[0]) and same_bytes(sparse.pages, before[1])
    small = sparse_agent(envs[1], capacity=64, max_steps=20, max_table_bytes=256 * (sparse.A * 12 + 8))
    with pytest.raises(ValueError, match="max_table_bytes"):  # 25 * 32 rows of room is more than 256 pages
        small.train(100, sync_every=25)
    for a in (dense, sparse, small):
        a.close()
    for e in envs:
        e.close()


# ----------------------------------------------------------------- 12. the footprint
@pytest.mark.parametrize("n", [1, 63, 65])
def test_footprint_of_every_sparse_call(n):
    """keys, pages, the se_sarsa_state fields, the five outputs, choose's three and a grow target
    carved out of a guarded arena at exactly their documented sizes, beside an ordinary twin: a
    learning step, a learn = 0 step, a choose, a grow and a step after it leave every guard as it
    was, change nothing they only read, and give the twin's outputs and table."""
    from shippingenv_amd import _native as N

    cap, cap2 = 256, 512
    g, t = OPEN.env(n, seed=SEED), OPEN.env(n, seed=SEED)
    probe = sparse_agent(t, capacity=cap, max_steps=3, max_attempts=4)
    A = probe.A
    learner = [("type", i32), ("a", i32), ("b", i32), ("fresh", u8), ("ep_len", i32), ("sarsa_return", f64)]
    outs = [("s_reward", f64), ("ended", u8), ("status", i32), ("fin_return", f64), ("fin_len", i32)]
    extra = ([("keys", i64, cap), ("pages", f64, (cap, A))] + [(k, dt, n) for k, dt in learner + outs] +
             [(k, i32, n) for k in ("ctype", "ca", "cb")] + [("gkeys", i64, cap2), ("gpages", f64, (cap2, A))])
    a = F.guard_env(g, extra)
    for e in (g, t):
        e.reset()
    a.set("keys", -1), a.set("pages", 0.0), a.set("gkeys", -1), a.set("gpages", 0.0)
    for k, v in (("type", 0), ("a", 0), ("b", 0), ("fresh", 1), ("ep_len", 0), ("sarsa_return", 0.0)):
        a.set(k, v)
    ag = sparse_agent(g, capacity=cap, max_steps=3, max_attempts=4)
    sst = N.SeSarsaState(*[a.ptr(k) for k, _ in learner])
    torch.cuda.synchronize()
    N.check(lib().se_sarsa_bind_sparse(ag._h, a.cptr("keys"), a.cptr("pages"), C.byref(sst)))
    state, names, onames = tuple(F.BIND_ORDER), tuple(k for k, _ in learner), tuple(k for k, _ in outs)

    def step(learn, tt, table):
        N.check(lib().se_sarsa_step(ag._h, 0.1, 0.9, 0.3, learn, 3, 4, tt, *[a.cptr(k) for k in onames], g._stream()))
        probe.t = tt
        probe.step(learn=bool(learn), epsilon=0.3)
        image = a.host()
        for k, want in zip(STATE + names + onames,
                           [getattr(t, f) for f in STATE] + [probe.type, probe.a, probe.b, probe.fresh, probe.ep_len,
                                                             probe.ep_return, probe.reward, probe.ended, probe.status,
                                                             probe.fin_return, probe.fin_len]):
            np.testing.assert_array_equal(a.get(k, image).reshape(-1).view(u8), want.cpu().numpy().reshape(-1).view(u8),
                                          err_msg=f"n={n} t={tt}: {k}")
        keys, pages = a.get(table[0], image), a.get(table[1], image)
        SP.check_valid(keys, pages, probe.rows)
        assert SP.as_map(keys, pages) == valid_map(probe, probe.rows)[0], f"n={n} t={tt}: the table"
        return image

    lists = ("done_recs", "done_count")
    for tt, learn in ((0, 1), (1, 1), (2, 0)):
        a.fill_out(*onames)
        a.snapshot()
        image = step(learn, tt, ("keys", "pages"))
        a.assert_clean(unchanged=lists + ("gkeys", "gpages") + (() if learn else ("keys", "pages")), image=image,
                       what=f"se_sarsa_step n={n} t={tt} learn={learn}")
    a.snapshot()
    N.check(lib().se_sarsa_choose(ag._h, 0.3, 5, a.cptr("ctype"), a.cptr("ca"), a.cptr("cb"), g._stream()))
    probe.t = 5
    image = a.host()
    a.assert_clean(unchanged=state + names + onames + ("keys", "pages", "gkeys", "gpages"), image=image,
                   what=f"se_sarsa_choose n={n}")
    for k, want in zip(("ctype", "ca", "cb"), probe.choose_action(epsilon=0.3)):
        np.testing.assert_array_equal(a.get(k, image), want.cpu().numpy(), err_msg=f"choose {k}")
    a.snapshot()
    N.check(lib().se_sarsa_sparse_grow(ag._h, a.cptr("gkeys"), a.cptr("gpages"), cap2, g._stream()))
    probe.grow(cap2)
    image = a.host()
    a.assert_clean(unchanged=state + names + onames + ("ctype", "ca", "cb", "keys", "pages"), image=image,
                   what=f"se_sarsa_sparse_grow n={n}")
    assert SP.as_map(a.get("gkeys", image), a.get("gpages", image)) == SP.as_map(a.get("keys", image), a.get("pages", image))
    cap_, used_ = C.c_int64(), C.c_int64()
    N.check(lib().se_sarsa_sparse_stats(ag._h, C.byref(cap_), C.byref(used_), None, g._stream()))
    assert cap_.value == cap2 and used_.value == SP.check_valid(a.get("gkeys", image), a.get("gpages", image), probe.rows)
    a.fill_out(*onames)
    a.snapshot()
    image = step(1, 6, ("gkeys", "gpages"))
    a.assert_clean(unchanged=lists + ("keys", "pages"), image=image, what=f"the step after the grow n={n}")
    for x in (ag, probe):
        x.close()
    for e in (g, t):
        e.close()
