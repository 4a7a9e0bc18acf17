"""se_mcts_choose / VecMCTSAgent against the Philox-driver restatement of choose_action
(tests/mcts_support.py), bit for bit: the chosen action, the status, tree_count and every node
(parent, action, visits; total_reward as f64 bits). The scenarios are hand-placed ships in the
hand-made worlds of tests/rollout_support.py, each 64 times in a row so that it sits in every
lane of a wave, plus three envs past the last whole wave; tests/test_mcts_cpu.py shows on the
restatement that they go through what they are named after. Then the law of the choice word."""
import ctypes as C

import numpy as np
import pytest

import law_support as L
import mcts_support as MS
from test_gpu_rollout import load_state, oracle_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

STATE = ("x", "y", "fuel", "cargo", "origin", "dest")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def ships_state(ships):
    st = O.OracleState(len(ships))
    for i, sh in enumerate(ships):
        st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = sh
    return st


def make(world, ships, S, env_id_base=0, **kw):
    """(env, agent, oracle state) with the ships loaded; the agent's handle holds S simulations."""
    from shippingenv_amd.mcts import VecMCTSAgent

    st = ships_state(ships)
    env = world.env(st.n, seed=MS.SEED, env_id_base=env_id_base)
    load_state(env, st)
    kw.setdefault("max_rollout_steps", MS.MAX_STEPS)
    kw.setdefault("max_attempts", MS.MAX_ATTEMPTS)
    return env, VecMCTSAgent(env, num_simulations=S, **kw), st


def scenario(name, S, **kw):
    return make(MS.SCENARIOS[name][0], MS.scenario_ships(name), S, **kw)


def choose(agent, S, base):
    """One decision batch with S simulations at mcts_base `base`, as numpy."""
    agent.num_simulations, agent.mcts_base = S, base
    ty, a, b, status, tree = agent.choose_action(return_tree=True)
    out = {k: v.cpu().numpy() for k, v in (("type", ty), ("a", a), ("b", b), ("status", status))}
    out["tree"] = {f: getattr(tree, f).cpu().numpy() for f in tree._fields}
    assert out["tree"]["parent"].shape == (agent.env.n, S + 1)
    return out


def assert_decisions(got, want, what=""):
    """The GPU's batch equals the restatement's decisions env by env."""
    t = got["tree"]
    for i, d in enumerate(want):
        tag = f"{what} env {i}"
        assert got["status"][i] == d.status, f"{tag}: status {got['status'][i]} != {d.status}"
        assert (got["type"][i], got["a"][i], got["b"][i]) == d.action, f"{tag}: action"
        assert t["count"][i] == len(d.nodes), f"{tag}: tree_count {t['count'][i]} != {len(d.nodes)}"
        for j, nd in enumerate(d.nodes):
            act = nd.action or (0, 0, 0)
            have = (t["parent"][i, j], t["type"][i, j], t["a"][i, j], t["b"][i, j], t["visits"][i, j])
            assert have == (nd.parent,) + act + (nd.visits,), f"{tag} node {j}: {have}"
            assert t["total_reward"][i, j].view(np.uint64) == np.float64(nd.total).view(np.uint64), \
                f"{tag} node {j}: total_reward {t['total_reward'][i, j]!r} != {nd.total!r}"


def assert_unchanged(env, st, what=""):
    after = oracle_state(env)
    for f in STATE:
        g, w = getattr(after, f), getattr(st, f)
        if f == "fuel":
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: the decision changed {f}")


# ----------------------------------------------------------------- the scenario tables
@pytest.mark.parametrize("name", sorted(MS.SCENARIOS))
def test_scenarios_bit_for_bit(name):
    """n = 64 k + 3, S = 1, 4, 5 (below the handle's size) and 17 (= max_simulations): the
    root's four moves fill and a second level opens; SELECT and TAKE_CARGO children, abandoned
    expansions, selections broken on done, raises, the fallback, and rollouts cut on some envs
    and not on others."""
    env, agent, st = scenario(name, max(MS.SIMS))
    assert env.n % 64 == MS.TAIL
    for S in MS.SIMS:
        assert_decisions(choose(agent, S, 0), MS.decisions(O, name, S), f"{name} S={S}")
        assert_unchanged(env, st, f"{name} S={S}")
    agent.close()
    env.close()


def test_single_env_every_actor():
    """n = 1: each actor of the open world alone, as env 0 of its own batch."""
    world, rows = MS.SCENARIOS["open"]
    for label, sh, _ in rows:
        env, agent, _ = make(world, [sh], 5)
        want = MS.decide(O, world.oracle(O), sh, seed=MS.SEED, id0=0, S=5, c=1.4, max_steps=MS.MAX_STEPS,
                         max_attempts=MS.MAX_ATTEMPTS)
        assert_decisions(choose(agent, 5, 0), [want], label)
        agent.close()
        env.close()


def test_world_image_past_64_kib():
    """The 256 x 256, 254-port world of rollout_support.max_world: its cell codes alone are
    64 KiB, so the image is past the dynamic LDS a launch gets without asking for more and
    se_mcts_choose has to ask. n = 5 (a wave's first lanes), 3 simulations, short rollouts, from
    the ships a reset and eight steps of the synthetic agent leave."""
    import rollout_support as RS
    from shippingenv_amd.mcts import VecMCTSAgent

    w = RS.max_world()
    env = w.env(5, seed=MS.SEED)
    env.reset()
    for t in range(8):
        env.step(env.gen_actions(t))
    st = oracle_state(env)
    ships = [(int(st.x[i]), int(st.y[i]), float(st.fuel[i]), int(st.cargo[i]), int(st.origin[i]), int(st.dest[i]))
             for i in range(env.n)]
    agent = VecMCTSAgent(env, num_simulations=3, max_rollout_steps=4, max_attempts=8)
    ow = w.oracle(O)
    want = [MS.decide(O, ow, sh, seed=MS.SEED, id0=i * 3, S=3, c=1.4, max_steps=4, max_attempts=8)
            for i, sh in enumerate(ships)]
    assert_decisions(choose(agent, 3, 0), want, "max world")
    assert any(len(d.nodes) > 1 for d in want)  # trees grew: their steps read the staged image
    assert_unchanged(env, st, "max world")
    agent.close()
    env.close()


def test_more_than_64_possible_actions():
    """Fuel 0 on an origin port that stocks 100: TAKE_CARGO 1..100, past the 64 action indices
    the kernel keeps as a bit mask, so the untried action is found by counting. With
    max_rollout_steps = 0 the rollouts draw nothing (with cargo aboard their sample_action
    would raise) and the tree grows: 17 of the root's 100 children, at indices on both sides of
    64."""
    import rollout_support as RS

    world = RS.World(7, 9, ports=[(1, 1), (5, 6), (3, 7)], fuel=[9, 4, 7], cargo=[100, 6, 8])
    ships = [MS.ship((1, 1), 0, 1, fuel=0.0)] * 67
    env, agent, st = make(world, ships, 17, max_rollout_steps=0, max_attempts=0)
    ow = world.oracle(O)
    want = [MS.decide(O, ow, sh, seed=MS.SEED, id0=i * 17, S=17, c=1.4, max_steps=0, max_attempts=0)
            for i, sh in enumerate(ships)]
    assert_decisions(choose(agent, 17, 0), want, "100 actions")
    taken = {d.nodes[j].action[1] for d in want for j in d.nodes[0].children}
    assert min(taken) <= 64 < max(taken) and all(d.status == MS.OK and len(d.nodes) == 18 for d in want)
    assert max(d.depth for d in want) == 1  # a root with 100 actions is not fully expanded by 17
    assert_unchanged(env, st, "100 actions")
    agent.close()
    env.close()


def test_wide_ids_and_base():
    """A 64-bit mcts_base and env_id_base: the simulation id fills both words of the key."""
    base, eb = (1 << 40) + 5, (1 << 33) + 64
    env, agent, _ = scenario("shared", 5, env_id_base=eb)
    assert_decisions(choose(agent, 5, base), MS.decisions(O, "shared", 5, mcts_base=base, env_id_base=eb), "wide ids")
    agent.close()
    env.close()


def test_reference_defaults_on_the_default_world():
    """Fresh resets on the default map and five ports, S = 50 and c = 1.4 as the reference's
    defaults, a 20-step rollout and the default max_attempts: the depth a real search reaches."""
    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.vec import VecEnv

    env = VecEnv(67, seed=21)
    env.reset()
    torch.cuda.synchronize()
    st = oracle_state(env)
    world = O.OracleWorld(env.water, env.port_x, env.port_y, env.port_fuel, env.port_cargo)
    agent = VecMCTSAgent(env, max_rollout_steps=20)
    assert (agent.num_simulations, agent.exploration_param, agent.max_rollout_steps, agent.max_attempts) == \
        (50, 1.4, 20, 160)
    got = choose(agent, 50, 0)
    want = [MS.decide(O, world, MS.PhiloxDriver._ship(_one(st, i)), seed=21, id0=i * 50, S=50, c=1.4, max_steps=20,
                      max_attempts=160) for i in range(env.n)]
    assert_decisions(got, want, "defaults")
    assert max(d.depth for d in want) >= 3
    assert_unchanged(env, st, "defaults")
    agent.close()
    env.close()


def _one(st, i):
    one = O.OracleState(1)
    for f in STATE:
        getattr(one, f)[0] = getattr(st, f)[i]
    return one


# ----------------------------------------------------------------- the interface
def test_without_tree_same_bases_and_stride():
    env, agent, _ = scenario("open", 5)
    full = choose(agent, 5, 0)
    agent.mcts_base = 0
    plain = [v.cpu().numpy().copy() for v in agent.choose_action()]
    for f, v in zip(("type", "a", "b", "status"), plain):
        np.testing.assert_array_equal(v, full[f], err_msg=f"return_tree=False: {f}")
    assert agent.mcts_base == env.n * 5 and agent.calls == 2  # advanced by stride * S, stride = n
    again = choose(agent, 5, 0)
    for f in ("type", "a", "b", "status"):
        np.testing.assert_array_equal(again[f], full[f], err_msg=f"same base: {f}")
    np.testing.assert_array_equal(again["tree"]["total_reward"].view(np.uint64),
                                  full["tree"]["total_reward"].view(np.uint64))
    other = choose(agent, 5, env.n * 5)
    assert (other["tree"]["total_reward"][:, 0] != full["tree"]["total_reward"][:, 0]).any()
    agent.stride = 1000
    agent.mcts_base = 7
    agent.choose_action()
    assert agent.mcts_base == 7 + 1000 * 5
    agent.close()
    env.close()


def test_shard_equals_the_same_ids_of_the_whole_run():
    world, ships = MS.SCENARIOS["open"][0], MS.scenario_ships("open")
    env, agent, _ = make(world, ships, 5)
    whole = choose(agent, 5, 11)
    lo, hi = 132, 132 + 131  # a multiple of 4 (se_create), no multiple of a wave at either end
    senv, sagent, _ = make(world, ships[lo:hi], 5, env_id_base=lo)
    part = choose(sagent, 5, 11)
    for f in ("type", "a", "b", "status"):
        np.testing.assert_array_equal(part[f], whole[f][lo:hi], err_msg=f"shard: {f}")
    for f in ("parent", "type", "a", "b", "visits", "count"):
        np.testing.assert_array_equal(part["tree"][f], whole["tree"][f][lo:hi], err_msg=f"shard tree: {f}")
    np.testing.assert_array_equal(part["tree"]["total_reward"].view(np.uint64),
                                  whole["tree"]["total_reward"][lo:hi].view(np.uint64))
    for a, e in ((agent, env), (sagent, senv)):
        a.close()
        e.close()


def test_empty_batch_and_argument_errors():
    from shippingenv_amd import _native as N
    from shippingenv_amd.mcts import VecMCTSAgent

    world = MS.SCENARIOS["open"][0]
    empty = world.env(0)
    agent = VecMCTSAgent(empty, num_simulations=4)
    out = agent.choose_action(return_tree=True)
    assert all(v.numel() == 0 for v in out[:4]) and out[4].count.numel() == 0
    agent.close()
    empty.close()

    env, agent, _ = scenario("one", 4)
    lib, h = N.lib(), C.c_void_p()
    for bad in (0, -1, N.MCTS_MAX_SIMULATIONS + 1):
        assert lib.se_mcts_create(C.byref(h), env._h, bad) == -1 and not h.value
    assert lib.se_mcts_create(C.byref(h), env._h, N.MCTS_MAX_SIMULATIONS) == 0
    lib.se_mcts_destroy(h)
    assert lib.se_mcts_create(None, env._h, 4) == -1
    assert lib.se_mcts_create(C.byref(h), None, 4) == -1

    bufs = [torch.zeros(env.n, dtype=torch.int32, device=env.device) for _ in range(5)]
    tree = torch.zeros((env.n, 5, 8), dtype=torch.int32, device=env.device)
    p = [C.c_void_p(t.data_ptr()) for t in bufs]

    def call(S=4, c=1.4, ms=6, ma=8, base=0, out=None, tr=None, cnt=None, handle=agent._h):
        o = p[:4] if out is None else out
        return lib.se_mcts_choose(handle, S, c, ms, ma, base, *o, tr, cnt, env._stream())

    assert call() == 0 and call(tr=C.c_void_p(tree.data_ptr()), cnt=p[4]) == 0
    for kw in (dict(S=0), dict(S=5), dict(c=float("nan")), dict(ms=-1), dict(ma=-1), dict(base=-1),
               dict(base=(1 << 63) - 1), dict(base=(1 << 63) - env.n * 4), dict(handle=None),
               dict(out=[None] + p[1:4]), dict(out=p[:3] + [None]), dict(tr=C.c_void_p(tree.data_ptr())),
               dict(cnt=p[4]), dict(out=[C.c_void_p(p[0].value + 4)] + p[1:4])):
        assert call(**kw) == -1, kw
        assert lib.se_last_error()
    assert call(base=(1 << 63) - 1 - env.n * 4) == 0  # the last id is 2^63 - 2
    with pytest.raises(N.ShipEnvError):
        VecMCTSAgent(env, num_simulations=0)
    torch.cuda.synchronize()
    agent.close()
    env.close()


def test_agent_step_is_choose_step_sample_step():
    """VecMCTSAgent.step() against the same calls made by hand on a twin env: where the first
    step raised (or the choice did: fuel_zero's type is SAMPLE_RAISES) the sampled action's step
    counts, elsewhere the first."""
    env, agent, _ = scenario("open", 5)
    twin, tagent, _ = scenario("open", 5)
    reward, done, err = (v.cpu().numpy() for v in agent.step())

    ty, a, b, status = (v.clone() for v in tagent.choose_action())
    r1, d1, e1 = (v.clone() for v in twin.step_typed(ty, a, b))
    failed = e1 != 0
    assert failed.any() and not failed.all()
    assert (failed.cpu().numpy() >= (status.cpu().numpy() >= MS.RAISED)).all()
    sty, sa, sb = twin.sample_actions(0)
    zero = torch.zeros_like(sty)
    r2, d2, e2 = twin.step_typed(torch.where(failed, sty, zero), torch.where(failed, sa, zero),
                                 torch.where(failed, sb, zero))
    np.testing.assert_array_equal(reward, torch.where(failed, r2, r1).cpu().numpy())
    np.testing.assert_array_equal(done, torch.where(failed, d2, d1).cpu().numpy())
    np.testing.assert_array_equal(err, torch.where(failed, e2, e1).cpu().numpy())
    assert (err[failed.cpu().numpy()] == 0).any(), "no sampled step went through"
    assert_unchanged(env, oracle_state(twin), "step() vs the calls by hand")
    for x in (agent, tagent, env, twin):
        x.close()


# ----------------------------------------------------------------- the choice word's law
def test_choice_word_is_uniform_and_independent_of_the_fuel_word():
    """2^16 envs on the same root with four untried moves, S = 1: the expanded action is word 0
    of the step's block and uniform over the four; the step's fuel word (word 1) decides
    whether the move runs out of fuel (fuel 1.0 against a cost of 0.9 .. 1.1: done, a reward
    below -5, half the time), and the two are independent."""
    from shippingenv_amd.mcts import VecMCTSAgent

    n = 1 << 16
    lw = L.water_world(5)
    from shippingenv_amd.vec import VecEnv

    env = VecEnv(n, water=lw.water, ports=lw.ports, port_fuel=lw.fuel_stock, port_cargo=lw.cargo_stock, seed=77)
    st = ships_state([MS.ship((50, 50), 0, 1, fuel=1.0)])
    for f in STATE:
        setattr(st, f, np.repeat(getattr(st, f), n))
    st.n = n
    load_state(env, st)
    agent = VecMCTSAgent(env, num_simulations=1, max_rollout_steps=0)
    ty, a, b, status, tree = agent.choose_action(return_tree=True)
    assert (tree.count == 2).all() and (status == MS.OK).all() and (ty == MS.MOVE).all()
    move = {m: k for k, m in enumerate(MS.MOVES)}
    k = np.array([move[(int(x), int(y))] for x, y in zip(a.cpu().numpy(), b.cpu().numpy())])
    reward = tree.total_reward[:, 1].cpu().numpy()  # the child's reward: the rollout adds 0.0
    dead = (reward < -5.0).astype(np.int64)
    stats = dict(L.check_uniform_int(k, 0, 3))
    stats["fuel_word"] = L.chi2_gof(np.bincount(dead, minlength=2), [0.5, 0.5])
    stats["independent"] = L.chi2_independence(L.table(k, dead, 4, 2))
    L.verdict("mcts_choice", stats)
    agent.close()
    env.close()
