"""se_mcts_choose_nav / VecMCTSAgent(navigator=...) against the restatement of
tests/mcts_nav_support.py, bit for bit: the chosen action, the status, tree_count and every node
(parent, action, visits; total_reward as f64 bits). Two scenario tables (mcts_support's and one on
nav_support's worlds), each actor 64 times in a row plus three envs past the last whole wave;
tests/test_mcts_nav_cpu.py shows on the restatement what they reach. Then the kernel against the
kernels it shares its code with: se_mcts_choose without playout steps, and se_rollout_nav."""
import ctypes as C

import numpy as np
import pytest

import mcts_nav_support as MN
import mcts_support as MS
import rollout_support as RS
from test_gpu_mcts import assert_decisions, assert_unchanged, choose, ships_state
from test_gpu_rollout import load_state, oracle_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
POISON = -77
TREE_FIELDS = ("parent", "type", "a", "b", "visits", "count")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def make(world, ships, S, env_id_base=0, navigator=True, refuel_below=MN.REFUEL_BELOW, load=MN.LOAD, **kw):
    """(env, navigator, agent, oracle state) with the ships loaded; the agent's handle holds S
    simulations and plays the navigator (navigator=False: the random policy)."""
    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.nav import VecNavigator

    st = ships_state(ships)
    env = world.env(st.n, seed=MN.SEED, env_id_base=env_id_base)
    load_state(env, st)
    nav = VecNavigator(env, refuel_below=refuel_below, load=load)
    kw.setdefault("max_rollout_steps", MN.MAX_STEPS)
    agent = VecMCTSAgent(env, num_simulations=S, exploration_param=MN.C_PARAM,
                         navigator=nav if navigator else None, **kw)
    return env, nav, agent, st


def close(*things):
    for x in things:
        x.close()


def assert_same_batch(got, want, what, rows=slice(None)):
    for f in ("type", "a", "b", "status"):
        np.testing.assert_array_equal(got[f], want[f][rows], err_msg=f"{what}: {f}")
    for f in TREE_FIELDS:
        np.testing.assert_array_equal(got["tree"][f], want["tree"][f][rows], err_msg=f"{what}: tree {f}")
    np.testing.assert_array_equal(got["tree"]["total_reward"].view(np.uint64),
                                  want["tree"]["total_reward"][rows].view(np.uint64), err_msg=f"{what}: total_reward")


# ----------------------------------------------------------------- 1. the scenario tables
@pytest.mark.parametrize("name", list(MN.SCENARIOS))
def test_scenarios_bit_for_bit(name):
    """n = 64 k + 3; S = 1, 4, 5 (below the handle's size) and 17 (= max_simulations). The env's
    state and counters are only read."""
    env, nav, agent, st = make(MN.SCENARIOS[name][0], MN.scenario_ships(name), max(MN.SIMS))
    assert env.n % 64 == MN.TAIL
    counters = env.counters
    for S in MN.SIMS:
        assert_decisions(choose(agent, S, 0), MN.decisions(O, name, S), f"{name} S={S}")
        assert_unchanged(env, st, f"{name} S={S}")
        assert env.counters == counters
    close(agent, nav, env)


# ----------------------------------------------------------------- 2. n = 1
def test_single_env_every_lake_actor():
    world, rows = MN.NAV_SCENARIOS["lake"]
    seen = set()
    for label, sh in rows:
        env, nav, agent, _ = make(world, [sh], 5)
        want = MN.decide(O, world, sh, seed=MN.SEED, id0=0, S=5)
        assert_decisions(choose(agent, 5, 0), [want], label)
        seen.add(want.status)
        close(agent, nav, env)
    assert MN.STUCK in seen and MN.OK in seen


# ----------------------------------------------------------------- 3. the shared tree path
@pytest.mark.parametrize("name", ["open", "many"])
def test_without_positions_equals_the_random_instantiation(name):
    """max_rollout_steps = 0: neither playout draws or adds anything, so se_mcts_choose_nav and
    se_mcts_choose(max_rollout_steps=0, max_attempts=1) write the same bytes."""
    ships = MS.scenario_ships(name)
    env, nav, agent, _ = make(MS.SCENARIOS[name][0], ships, 17, max_rollout_steps=0)
    renv, rnav, ragent, _ = make(MS.SCENARIOS[name][0], ships, 17, navigator=False, max_rollout_steps=0,
                                 max_attempts=1)
    got, want = choose(agent, 17, 0), choose(ragent, 17, 0)
    assert_same_batch(got, want, f"{name}: nav vs random without positions")
    assert (got["tree"]["count"] > 1).any()
    assert_decisions(got, MN.decisions(O, name, 17, max_steps=0), f"{name} without positions")
    close(agent, nav, env, ragent, rnav, renv)


# ----------------------------------------------------------------- 4. kernel against kernel
@pytest.mark.parametrize("name,label", [("open", "select"), ("shared", "shared_select"), ("many", "wide")])
def test_single_simulation_playout_is_se_rollout_nav(name, label):
    """Ships on a port without destination, S = 1: the only node is a SELECT q child, whose step
    is drawn but deterministic (reward 0, dest := q), so its total_reward is the playout's return.
    A second env holds the same ships with dest = q: se_rollout_nav under the simulations' ids
    returns the same bits."""
    world, rows = MS.SCENARIOS[name]
    sh = next(s for lb, s, _ in rows if lb == label)
    base, eb, n = (1 << 40) + 5, 132, 67
    env, nav, agent, st = make(world, [sh] * n, 1, env_id_base=eb)
    got = choose(agent, 1, base)
    t = got["tree"]
    assert (t["count"] == 2).all() and (t["type"][:, 1] == MS.SELECT).all() and (got["status"] == MN.OK).all()
    q = t["a"][:, 1]
    assert len(set(q.tolist())) > 1 or world.P - 1 == 1
    st.dest[:] = q
    twin = world.env(n, seed=MN.SEED, env_id_base=eb)
    load_state(twin, st)
    from shippingenv_amd.nav import VecNavigator

    tnav = VecNavigator(twin, refuel_below=MN.REFUEL_BELOW, load=MN.LOAD)
    ids = torch.as_tensor(base + eb + np.arange(n, dtype=np.int64))
    res = tnav.rollout(steps=MN.MAX_STEPS, ids=ids)
    ret = res.ret.cpu().numpy()
    assert (res.steps.cpu().numpy() > 0).all() and (ret != 0).any()
    np.testing.assert_array_equal(t["total_reward"][:, 1].view(np.uint64), ret.view(np.uint64))
    np.testing.assert_array_equal(t["total_reward"][:, 0].view(np.uint64), ret.view(np.uint64))
    assert (t["visits"][:, :2] == 1).all()
    close(agent, nav, env, tnav, twin)


# ----------------------------------------------------------------- 5. shards
def test_shards_equal_the_whole_run_with_ids_past_2_32():
    """One env of 2 * 64 + 3 ships against two envs that split it (env_id_base is a multiple of 4:
    0 and 68, no multiple of a wave), mcts_base = 2^40."""
    world = MN.NAV_SCENARIOS["lake"][0]
    ships = MN.scenario_ships("lake")[160:160 + 131]  # outside, walled_in and pocket_select
    base, cut = 1 << 40, 68
    env, nav, agent, _ = make(world, ships, 5)
    whole = choose(agent, 5, base)
    assert {MN.OK, MN.STUCK} <= set(whole["status"].tolist())
    for lo, hi in ((0, cut), (cut, len(ships))):
        senv, snav, sagent, _ = make(world, ships[lo:hi], 5, env_id_base=lo)
        assert_same_batch(choose(sagent, 5, base), whole, f"shard {lo}:{hi}", slice(lo, hi))
        close(sagent, snav, senv)
    want = [MN.decide(O, world, sh, seed=MN.SEED, id0=base + i * 5, S=5) for i, sh in enumerate(ships)]
    assert_decisions(whole, want, "wide ids")
    close(agent, nav, env)


# ----------------------------------------------------------------- 6. misuse
def test_argument_errors_stale_and_foreign_navigators_and_no_envs():
    from shippingenv_amd import _native as N
    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.nav import VecNavigator

    lib = N.lib()
    world = MS.SCENARIOS["open"][0]
    ships = MS.scenario_ships("open")[:67]
    env, nav, agent, st = make(world, ships, 4)
    other = world.env(env.n, seed=MN.SEED)
    onav = VecNavigator(other, refuel_below=MN.REFUEL_BELOW, load=MN.LOAD)
    bufs = [torch.full((env.n,), POISON, dtype=torch.int32, device=env.device) for _ in range(5)]
    tree = torch.full((env.n, 5, 8), POISON, dtype=torch.int32, device=env.device)
    p = [C.c_void_p(t.data_ptr()) for t in bufs]
    tp = C.c_void_p(tree.data_ptr())

    def call(m=agent._h, nv=nav._h, rb=MN.REFUEL_BELOW, load=MN.LOAD, S=4, c=1.4, ms=6, base=0, out=None, tr=None,
             cnt=None):
        o = p[:4] if out is None else out
        return lib.se_mcts_choose_nav(m, nv, rb, load, S, c, ms, base, *o, tr, cnt, env._stream())

    def untouched():
        torch.cuda.synchronize()
        return all((t == POISON).all() for t in bufs + [tree])

    bad = (dict(m=None), dict(nv=None), dict(load=-1), dict(c=float("nan")), dict(ms=-1), dict(base=-1), dict(S=0),
           dict(S=5), dict(base=(1 << 63) - 1), dict(base=(1 << 63) - env.n * 4),
           dict(out=[C.c_void_p(p[0].value + 4)] + p[1:4]), dict(tr=tp), dict(cnt=p[4]),
           dict(out=[None] + p[1:4]), dict(out=p[:3] + [None]), dict(nv=onav._h))
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.se_last_error()
    assert untouched(), "a refused call launched something"
    # a stale navigator: SE_ESTATE through the C call, misuse still SE_EINVAL, nothing launched
    moved = RS.World(7, 9, ports=[(5, 6), (1, 1), (5, 2)], fuel=[2, 3, 4], cargo=[1, 0, 9], ground=[(2, 5)])
    env.set_ports(moved.ports, moved.fuel_stock, moved.cargo_stock)
    assert call(tr=tp, cnt=p[4]) == ESTATE and "se_nav_rebuild" in lib.se_last_error().decode()
    for kw in bad:
        assert call(**kw) == EINVAL, ("stale", kw)
    assert untouched(), "a stale handle launched something"
    # ... and rebuilt by VecMCTSAgent
    got = choose(agent, 4, 0)
    want = [MN.decide(O, moved, sh, seed=MN.SEED, id0=i * 4, S=4) for i, sh in enumerate(ships)]
    assert_decisions(got, want, "after set_ports")
    assert call(tr=tp, cnt=p[4]) == 0  # the handle is current again
    assert call(base=(1 << 63) - 1 - env.n * 4, rb=float("nan"), load=0) == 0  # the last id is 2^63 - 2
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tree[:, 0, 0].cpu().numpy(), -1)
    with pytest.raises(ValueError):
        VecMCTSAgent(env, num_simulations=4, navigator=onav)
    close(agent, nav, onav, other, env)

    empty = world.env(0)
    enav = VecNavigator(empty, refuel_below=MN.REFUEL_BELOW, load=MN.LOAD)
    eagent = VecMCTSAgent(empty, num_simulations=4, navigator=enav)
    assert lib.se_mcts_choose_nav(eagent._h, enav._h, 3.0, 3, 4, 1.4, 6, 0, None, None, None, None, None, None,
                                  empty._stream()) == 0
    out = eagent.choose_action(return_tree=True)
    assert all(v.numel() == 0 for v in out[:4]) and out[4].count.numel() == 0
    close(eagent, enav, empty)


# ----------------------------------------------------------------- 7. VecMCTSAgent
def test_agent_equals_the_raw_call_and_advances_its_base():
    from shippingenv_amd import _native as N

    name, S = "wall", 5
    env, nav, agent, _ = make(MN.SCENARIOS[name][0], MN.scenario_ships(name), S)
    agent.mcts_base = 7
    got = choose(agent, S, 7)
    assert agent.mcts_base == 7 + env.n * S and agent.calls == 1  # advanced by stride * S, stride = n
    bufs = [torch.zeros(env.n, dtype=torch.int32, device=env.device) for _ in range(5)]
    raw = torch.zeros((env.n, S + 1, 8), dtype=torch.int32, device=env.device)
    rc = N.lib().se_mcts_choose_nav(agent._h, nav._h, nav.refuel_below, nav.load, S, agent.exploration_param,
                                    agent.max_rollout_steps, 7, *[C.c_void_p(t.data_ptr()) for t in bufs[:4]],
                                    C.c_void_p(raw.data_ptr()), C.c_void_p(bufs[4].data_ptr()), env._stream())
    assert rc == 0
    for f, t in zip(("type", "a", "b", "status"), bufs):
        np.testing.assert_array_equal(got[f], t.cpu().numpy(), err_msg=f)
    raw = raw.cpu().numpy()
    for k, f in enumerate(("parent", "type", "a", "b", "visits")):
        np.testing.assert_array_equal(got["tree"][f], raw[:, :, k], err_msg=f)
    np.testing.assert_array_equal(got["tree"]["count"], bufs[4].cpu().numpy())
    np.testing.assert_array_equal(got["tree"]["total_reward"].view(np.uint64),
                                  np.ascontiguousarray(raw[:, :, 6:8]).view(np.uint64).reshape(env.n, S + 1))
    plain = [v.cpu().numpy().copy() for v in agent.choose_action()]  # without the tree, at the next base
    assert agent.mcts_base == 7 + 2 * env.n * S and agent.calls == 2
    nxt = MN.decisions(O, name, S, mcts_base=7 + env.n * S)
    np.testing.assert_array_equal(plain[3], [d.status for d in nxt])
    np.testing.assert_array_equal(np.stack(plain[:3], 1), np.array([d.action for d in nxt], np.int32))
    agent.stride, agent.mcts_base = 1000, 7
    agent.choose_action()
    assert agent.mcts_base == 7 + 1000 * S
    close(agent, nav, env)


def test_agent_step_is_choose_step_sample_step_on_the_oracle():
    """VecMCTSAgent.step() with a navigator, restated: the restatement's decision, the oracle's
    typed step, and where that raised (or the choice did) the oracle's sample_action and a second
    step; the env ends in the oracle's state."""
    name, S = "open", 5
    world = MS.SCENARIOS[name][0]
    env, nav, agent, st = make(world, MS.scenario_ships(name), S)
    ow = world.oracle(O)
    t0 = env.counters[0]
    reward, done, err = (v.cpu().numpy() for v in agent.step())

    want = MN.decisions(O, name, S)
    act = np.array([d.action for d in want], np.int32)
    O.step(ow, st, act_type=act[:, 0], act_a=act[:, 1], act_b=act[:, 2], seed=MN.SEED, t=t0)
    r1, d1, e1 = st.reward.copy(), st.done.copy(), st.err.copy()
    failed = e1 != 0
    assert failed.any() and not failed.all()
    assert (failed >= np.array([d.status in (MN.RAISED, MN.NEVER_RETURNS) for d in want])).all()
    sty, sa, sb = O.sample_actions(ow, st, seed=MN.SEED, t=0)
    O.step(ow, st, act_type=np.where(failed, sty, 0), act_a=np.where(failed, sa, 0), act_b=np.where(failed, sb, 0),
           seed=MN.SEED, t=t0 + 1)
    np.testing.assert_array_equal(reward, np.where(failed, st.reward, r1).astype(np.float32))
    np.testing.assert_array_equal(done.astype(np.int32), np.where(failed, st.done, d1))
    np.testing.assert_array_equal(err.astype(np.int32), np.where(failed, st.err, e1))
    assert (err[failed] == 0).any(), "no sampled step went through"
    assert_unchanged(env, st, "step() vs the oracle")
    assert env.counters[0] == t0 + 2
    close(agent, nav, env)


def test_without_a_navigator_nothing_changes():
    name, S = "shared", 5
    from shippingenv_amd.mcts import VecMCTSAgent

    st = ships_state(MS.scenario_ships(name))
    env = MS.SCENARIOS[name][0].env(st.n, seed=MS.SEED)
    load_state(env, st)
    agent = VecMCTSAgent(env, num_simulations=S, max_rollout_steps=MS.MAX_STEPS, max_attempts=MS.MAX_ATTEMPTS,
                         navigator=None)
    assert_decisions(choose(agent, S, 0), MS.decisions(O, name, S), "navigator=None")
    close(agent, env)
