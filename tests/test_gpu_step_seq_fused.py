"""se_step_seq without auto-reset runs a sequence as fused launches (step_seq_kernel: the
state stays in registers from step to step, stored once with the last step's outputs).
Every comparison here is exact: against K VecEnv.step calls on a twin env, against the C
oracle, and against the unsplit run wherever the run is cut (the timer mark, the per-launch
step cap, several groups per thread, the per-step baseline)."""
import numpy as np
import pytest

from conftest import golden_water
from step_seq_support import assert_same, environ, gpu_lib, snapshot  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]


def make_env(n, ports64=False, seed=22, auto=False, **env):
    from shippingenv_amd.vec import VecEnv, random_water_ports

    ports = random_water_ports(golden_water(), 64, seed=3) if ports64 else None
    with environ(**env):
        return VecEnv(n, seed=seed, ports=ports, auto_reset=auto)


def action_rows(env, rows, pad=8):
    """[rows, n] views of gen_actions rows at a padded stride ld > n (a multiple of 4)."""
    n = env.n
    ld = ((n + 3) & ~3) + pad
    buf = torch.full((rows, ld), -99, dtype=torch.int32, device=env.device)  # padding: a bad index if ever read
    for t in range(rows):
        env.gen_actions(t, out=buf[t, :n])
    return buf[:, :n]


def step_calls(env, acts, lo, hi):
    for t in range(lo, hi):
        env.step(acts[t].contiguous())


@pytest.mark.parametrize("ports64,nt", [(False, "1"), (False, "0"), (True, "1"), (True, "0")])
@pytest.mark.parametrize("K", [1, 2, 33])
@pytest.mark.parametrize("n", [3, 4, 7, 4099, 50003])
def test_fused_equals_step_calls(n, K, ports64, nt):
    """n: the tail alone, one group, group + tail, 4 workgroups + a tail of 3, a ragged last
    workgroup. Then 3 plain steps on both: the step counter advanced by K."""
    a = make_env(n, ports64, SHIPENV_NT_LOADS=nt)
    b = make_env(n, ports64, SHIPENV_NT_LOADS=nt)
    acts = action_rows(a, K + 3)
    a.reset()
    b.reset()
    step_calls(a, acts, 0, K)
    r, d, e = b.step_seq(acts[:K])
    assert r.data_ptr() == b.reward.data_ptr() and d.data_ptr() == b.done.data_ptr() and e.data_ptr() == b.err.data_ptr()
    assert_same(snapshot(b), snapshot(a), f"after the fused run of {K}")
    assert b.counters[0] == a.counters[0] == K
    step_calls(a, acts, K, K + 3)
    step_calls(b, acts, K, K + 3)
    assert_same(snapshot(b), snapshot(a), "3 plain steps later")
    a.close()
    b.close()


def test_fused_long_run_through_out_of_fuel():
    """K = 260 from reset, mostly moves: 200 fuel at ~1 per move takes ships through out of
    fuel, negative fuel and done inside one fused run, next to the takes, selects, cargo
    losses and arrivals of the generated mix."""
    n, K = 4099, 260
    a, b = make_env(n), make_env(n)
    acts = action_rows(a, K + 3)
    g = torch.Generator(device="cpu").manual_seed(5)
    moves = torch.randint(0, 4, (K + 3, n), generator=g, dtype=torch.int32).to(a.device)
    keep = (torch.rand((K + 3, n), generator=g) < 0.1).to(a.device)
    acts.copy_(torch.where(keep, acts, moves))
    a.reset()
    b.reset()
    seen_done = 0
    for t in range(K):
        _, d, _ = a.step(acts[t].contiguous())
        seen_done += int(d.sum().item())
    b.step_seq(acts[:K])
    want = snapshot(a)
    assert seen_done > 0 and (a.fuel < 0).any().item()  # the run did go through out of fuel
    assert_same(snapshot(b), want, "after 260 fused steps")
    step_calls(a, acts, K, K + 3)
    step_calls(b, acts, K, K + 3)
    assert_same(snapshot(b), snapshot(a), "3 plain steps later")
    a.close()
    b.close()


def test_fused_vs_oracle(oracle_mod):
    O = oracle_mod
    seed, n, K = 77, 4099, 64
    env = make_env(n, seed=seed)
    world = O.OracleWorld(env.water, env.port_x, env.port_y, env.port_fuel, env.port_cargo)
    st = O.OracleState(n)
    acts = action_rows(env, K)
    host = acts.cpu().numpy()
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    for t in range(K):
        O.step(world, st, actions=np.ascontiguousarray(host[t]), seed=seed, t=t)
    env.step_seq(acts)
    got = snapshot(env)
    for f in ("x", "y", "cargo", "done", "err"):
        np.testing.assert_array_equal(got[f].astype(np.int32), getattr(st, f), err_msg=f)
    for f in ("origin", "dest"):
        np.testing.assert_array_equal(np.where(got[f] == 255, -1, got[f].astype(np.int32)), getattr(st, f), err_msg=f)
    np.testing.assert_array_equal(got["fuel"].view(np.int64), st.fuel.view(np.int64), err_msg="fuel bits")
    np.testing.assert_array_equal(got["reward"], st.reward.astype(np.float32), err_msg="reward")
    env.close()


SPLIT_N, SPLIT_K = 4099, 33


@pytest.fixture(scope="module")
def unsplit():
    """One fused launch of 33 steps from reset at n = 4099 (read-only, shared)."""
    env = make_env(SPLIT_N)
    acts = action_rows(env, SPLIT_K)
    env.reset()
    env.step_seq(acts)
    want = snapshot(env)
    env.close()
    for v in want.values():
        v.setflags(write=False)
    return want


@pytest.mark.parametrize("mark_after", [0, 5, 33])
def test_split_at_the_mark(unsplit, mark_after):
    env = make_env(SPLIT_N)
    acts = action_rows(env, SPLIT_K)
    env.reset()
    ev, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    env.step_seq(acts, mark=ev, mark_after=mark_after)
    end.record()
    torch.cuda.synchronize()
    assert ev.elapsed_time(end) >= 0.0
    assert_same(snapshot(env), unsplit, f"mark_after={mark_after}")
    assert env.counters[0] == SPLIT_K
    env.close()


@pytest.mark.parametrize("var,value", [("SHIPENV_SEQ_MAX_STEPS", "8"),  # five launches: 8 + 8 + 8 + 8 + 1
                                       ("SHIPENV_STEP_BLOCKS", "2"),    # 3 groups per thread
                                       ("SHIPENV_SEQ_FUSE", "0")])      # a launch per step
def test_split_by_setting(unsplit, var, value):
    env = make_env(SPLIT_N, **{var: value})
    acts = action_rows(env, SPLIT_K)
    env.reset()
    env.step_seq(acts)
    assert_same(snapshot(env), unsplit, f"{var}={value}")
    assert env.counters[0] == SPLIT_K
    env.close()


def test_autoreset_sequence_stays_per_step():
    """Auto-reset keeps a launch per step: its step_seq equals its step calls, the last
    step's done list and the episode statistics included."""
    n, K = 515, 12
    a, b = make_env(n, True, auto=True), make_env(n, True, auto=True)
    acts = action_rows(a, K)
    # mostly moves from a low tank, so episodes end inside the run
    g = torch.Generator(device="cpu").manual_seed(6)
    moves = torch.randint(0, 4, (K, n), generator=g, dtype=torch.int32).to(a.device)
    acts.copy_(torch.where((torch.rand((K, n), generator=g) < 0.1).to(a.device), acts, moves))
    for env in (a, b):
        env.reset()
        env.fuel.fill_(3.0)
    step_calls(a, acts, 0, K)
    b.step_seq(acts)
    assert_same(snapshot(b), snapshot(a), "auto-reset")
    for f in ("ep_return", "ep_len"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    sa, sb = a.episode_stats().clone(), b.episode_stats().clone()
    assert torch.equal(sa, sb) and sa[1].item() > 0
    for u, v in zip(a.done_list(), b.done_list()):
        assert torch.equal(u, v)
    a.close()
    b.close()


def test_empty_batch():
    env = make_env(0)
    env.reset()
    env.step_seq(torch.empty((3, 0), dtype=torch.int32, device=env.device))
    torch.cuda.synchronize()
    assert env.counters[0] == 3
    env.close()
