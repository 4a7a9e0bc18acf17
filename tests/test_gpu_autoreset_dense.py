"""The auto-reset step at every done density, bit for bit against the C oracle.

The other suites run SE_FLAG_AUTO_RESET where about 1 env in 240 finishes per step, so a lane of
4 envs almost never finishes two. Here a case chooses its finishing envs (tests/autoreset_support.py;
test_autoreset_dense_cpu.py holds the cases to their claims), which reaches: wave_compact's three
bit-planes at every lane count 0..4, segments filled to 256 records, the filler at every length,
the tail group appending to a part-filled and to a fresh segment; the RESET ranks 0..3 of both
rank blocks (se_step and se_step_typed); each record's ep_return and ep_len, not only their
sums; the statistics slab's one-lane shortcut from lane 63 and its trees; the episode-start
stamps, untouched where no env of the lane finished, across the 2^32 wrap of the step counter;
and se_step_record's own slab path and stamp loads.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import autoreset_support as A

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

T_WRAP = 2**32 - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


_OPEN = []


@pytest.fixture(autouse=True)
def _close_after():
    yield
    while _OPEN:  # buffers before their env, also when the test failed
        _OPEN.pop().close()


def make_env(n, monkeypatch, blocks=None, pad=None):
    from shippingenv_amd.vec import VecEnv

    for name, v in (("SHIPENV_STEP_BLOCKS", blocks), ("SHIPENV_DONE_PAD", pad)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    env = VecEnv(n, water=A.water(), ports=[list(p) for p in A.PORTS], port_fuel=A.PORT_FUEL,
                 port_cargo=A.PORT_CARGO, seed=A.SEED, auto_reset=True)
    _OPEN.append(env)
    assert env.done_seg == A.SEG and env.done_segments == 4 * ((n + 1023) // 1024)
    return env


def _put(t, a, dtype):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).astype(dtype)))


def load_case(env, c):
    """The case's state and running episodes at step counter t0; both halves of the done list
    and every count prefilled with the sentinel (set_counters clears the counts, so after it)."""
    env.set_counters(c.t0, 0)
    b = c.steps[0].before
    for f, dt in (("x", np.uint8), ("y", np.uint8), ("cargo", np.int32), ("origin", np.uint8), ("dest", np.uint8)):
        _put(getattr(env, f), getattr(b, f), dt)
    _put(env.ep_return, b.ep_return, np.float32)
    _put(env.ep_start, c.start0, np.int32)
    env.done_recs.fill_(A.SENTINEL)
    env.done_count.fill_(A.SENTINEL)
    env.reward.fill_(-77.0)
    env.done.fill_(9)
    env.err.fill_(-9)


def refuel(env, step):
    _put(env.fuel, step.fuel, np.float64)


def actions_of(env, step):
    return torch.from_numpy(np.array(step.actions, np.int32)).to(env.device)


def raw_lists(env):
    """(records [2, segments * 256, 4], counts [2, segments], the half the last step wrote)."""
    from shippingenv_amd import _native as N

    ro, co = C.c_int64(), C.c_int64()
    N.check(N.lib().se_done_list(env._h, C.byref(ro), C.byref(co)))
    nseg, seg = env.done_segments, env.done_seg
    torch.cuda.synchronize()
    recs = env.done_recs.cpu().numpy().reshape(2, nseg * seg, 4)
    counts = env.done_count.cpu().numpy()[:2 * nseg].reshape(2, nseg)
    assert ro.value % (nseg * seg) == 0 and ro.value // (nseg * seg) == co.value // nseg
    return recs, counts, ro.value // (nseg * seg)


def check_state(env, step, what):
    a = step.after
    torch.cuda.synchronize()
    for f in ("x", "y", "cargo", "origin", "dest", "done", "err"):
        np.testing.assert_array_equal(getattr(env, f).cpu().numpy().astype(np.int32), getattr(a, f),
                                      err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(env.fuel.cpu().numpy().view(np.int64), a.fuel.view(np.int64), err_msg=f"{what}: fuel")
    np.testing.assert_array_equal(env.reward.cpu().numpy(), a.reward.astype(np.float32), err_msg=f"{what}: reward")
    np.testing.assert_array_equal(env.ep_return.cpu().numpy(), a.ep_return, err_msg=f"{what}: ep_return")
    np.testing.assert_array_equal(env.ep_start.cpu().numpy(), step.exp.start, err_msg=f"{what}: ep_start")
    np.testing.assert_array_equal(env.ep_len.cpu().numpy(), a.ep_len, err_msg=f"{what}: ep_len")


def check_done_list(env, step, what):
    e = step.exp
    ids, ret, length, st = (v.cpu().numpy() for v in env.done_list())
    np.testing.assert_array_equal(ids, e.env, err_msg=f"{what}: done_list ids")
    np.testing.assert_array_equal(ret.view(np.int32), e.ret.view(np.int32), err_msg=f"{what}: done_list ep_return")
    np.testing.assert_array_equal(length, e.len, err_msg=f"{what}: done_list ep_len")
    np.testing.assert_array_equal(st, e.step, err_msg=f"{what}: done_list step")


def check_raw(env, step, pad, other_recs, other_counts, what):
    """The half this step wrote, record for record; the other half as it was."""
    recs, counts, half = raw_lists(env)
    assert half == (step.t & 1), what
    want, want_counts = A.raw_half(step.exp, env.n, env.done_segments, step.t, pad)
    np.testing.assert_array_equal(counts[half], want_counts, err_msg=f"{what}: segment counts")
    seg = env.done_seg
    t32 = np.array(step.t & 0xFFFFFFFF, np.uint32).view(np.int32)
    for s in range(env.done_segments):
        k = want_counts[s]
        np.testing.assert_array_equal(recs[half][s * seg:s * seg + k], want[s * seg:s * seg + k],
                                      err_msg=f"{what}: records of segment {s}")
        rest = recs[half][s * seg + k:(s + 1) * seg]
        sentinel = (rest == A.SENTINEL).all(1)
        filler = (rest[:, 0] == -1) & (rest[:, 3] == t32)
        if not pad:
            assert sentinel.all(), f"{what}: segment {s} written past its count"
        assert (sentinel | filler).all(), f"{what}: segment {s} holds neither sentinel nor filler past its count"
    # and exactly: the filler from the full groups' count to the next run of 8, no further
    np.testing.assert_array_equal(recs[half], want, err_msg=f"{what}: the half this step wrote")
    np.testing.assert_array_equal(recs[1 - half], other_recs, err_msg=f"{what}: the other half's records")
    np.testing.assert_array_equal(counts[1 - half], other_counts, err_msg=f"{what}: the other half's counts")
    return recs[half].copy(), counts[half].copy()


def check_stats(env, steps, what):
    """Episodes and lengths exactly. The returns: the slab adds exactly representable f32 terms
    in f64 in some fixed order; any order of k - 1 f64 additions of k such terms is within
    (k - 1) 2^-53 sum |ret| (1 + O(2^-53)) of the exact sum, which k 2^-52 sum |ret| covers;
    k is the number of terms or the number of envs, whichever is smaller (two steps finish at
    most 2 n episodes, and (2 n - 1) 2^-53 < n 2^-52)."""
    got = env.episode_stats().cpu().numpy()
    rets = np.concatenate([s.exp.ret for s in steps]).astype(np.float64)
    lens = np.concatenate([s.exp.len for s in steps]).astype(np.int64)
    assert got[1] == len(rets), f"{what}: episodes"
    assert got[2] == int(lens.sum()), f"{what}: sum of lengths"
    exact = math.fsum(rets.tolist())
    bound = min(len(rets), env.n) * 2.0**-52 * math.fsum(np.abs(rets).tolist())
    print(f"STATS {what}: sum of returns {got[0]!r} exact {exact!r} diff {abs(got[0] - exact):.3e} bound {bound:.3e}")
    assert abs(got[0] - exact) <= bound, f"{what}: sum of returns {got[0]!r} vs {exact!r}, bound {bound:.3e}"


def run_case(env, c, pad, step_fn, what):
    load_case(env, c)
    nseg, seg = env.done_segments, env.done_seg
    other_recs = np.full((nseg * seg, 4), A.SENTINEL, np.int32)
    other_counts = np.full(nseg, A.SENTINEL, np.int32)
    for k, step in enumerate(c.steps):
        w = f"{what} step {k} ({step.pattern}, t={step.t})"
        refuel(env, step)
        step_fn(env, step)
        assert env.counters[0] == step.t + 1
        check_state(env, step, w)
        check_done_list(env, step, w)
        # the second step leaves the first step's half as the first step wrote it
        other_recs, other_counts = check_raw(env, step, pad, other_recs, other_counts, w)
    check_stats(env, c.steps, what)


def agent_step(env, step):
    r, d, e = env.step(actions_of(env, step))
    assert r.data_ptr() == env.reward.data_ptr()


@pytest.mark.parametrize("t0", [7, T_WRAP])
@pytest.mark.parametrize("pad", [None, "1"])
@pytest.mark.parametrize("blocks", [None, "1"])
@pytest.mark.parametrize("n", [A.N_TAIL_APPENDS, A.N_TAIL_FRESH])
@pytest.mark.parametrize("pattern", A.PATTERNS)
def test_dense_step_vs_oracle(monkeypatch, pattern, n, blocks, pad, t0):
    """One se_step finishing the pattern's envs, then one finishing second_pattern's, against the
    oracle: every state and output tensor, ep_return, the ep_start tensor bit for bit, ep_len,
    done_list(), the raw list of each step (counts, records, filler, sentinel; the other half
    untouched) and episode_stats(). blocks="1": one workgroup, two groups per thread. pad="1":
    the records padded with filler to whole lines. t0 = 2^32 - 1: the first step stamps t + 1 = 0
    and the second runs at counter 2^32."""
    env = make_env(n, monkeypatch, blocks, pad)
    c = A.case(pattern, n, t0)
    run_case(env, c, pad is not None, agent_step, f"{pattern} n={n} blocks={blocks} pad={pad} t0={t0}")


@pytest.mark.parametrize("pattern", ["all", "counts", "random50"])
def test_typed_step_with_auto_reset_equals_the_agent_step(monkeypatch, pattern):
    """se_step_typed on an auto-reset env (step_group's RESET-rank block) with O.decode_agent of
    the same agent indices: the twin equals the agent-path env, and both the oracle, in every
    tensor and in the done list. Every index the cases use decodes to a typed action (the
    synthetic agent's indices are all in range; what raises, raises inside the step), so the
    survivors' actions are not restricted."""
    n = A.N_TAIL_APPENDS
    c = A.case(pattern, n, 7)
    what = f"typed {pattern}"

    def typed_step(env, step):
        ty, a, b, err = O.decode_agent(step.actions, len(A.PORTS))
        assert (err == 0).all()
        env.step_typed(ty, a, b)

    envs = [make_env(n, monkeypatch), make_env(n, monkeypatch)]
    run_case(envs[0], c, False, agent_step, what + " (agent twin)")
    run_case(envs[1], c, False, typed_step, what)
    for f in ("x", "y", "fuel", "cargo", "origin", "dest", "reward", "done", "err", "ep_return", "ep_start",
              "done_recs", "done_count"):
        assert torch.equal(getattr(envs[0], f), getattr(envs[1], f)), f"{what}: {f}"
    assert torch.equal(envs[0].episode_stats(), envs[1].episode_stats())


@pytest.mark.parametrize("max_steps", [0, 3])
@pytest.mark.parametrize("pattern", ["all", "counts", "totals"])
def test_step_record_dense_equals_step_then_end_reset(monkeypatch, pattern, max_steps):
    """se_step_record in one launch (n = 1024, ring capacity 4096: its own slab path with
    atomics, and the stamps loaded for every lane) against se_step + se_replay_end_reset on a
    twin, over the case's two steps: state, cut, ep_len, ep_return, the done list, the bits of
    episode_stats() and the whole ring through a minibatch of every stored transition. The
    first step of the one-launch side also against the oracle: the done list, and with
    max_steps = 0 (cut = the step raised) everything else, as step_autoreset then
    reset(mask=cut) at the reset epoch leave it."""
    from shippingenv_amd.dqn import MiniBatch, ReplayBuffer

    n = A.N_RECORD
    c = A.case(pattern, n, 7)
    envs, rbs, cuts = [], [], []
    for _ in range(2):
        env = make_env(n, monkeypatch)
        rb = ReplayBuffer(env, 4096)
        _OPEN.append(rb)
        load_case(env, c)
        envs.append(env)
        rbs.append(rb)
        cuts.append(torch.full((n,), 5, dtype=torch.uint8, device=env.device))
    fields = ("x", "y", "fuel", "cargo", "origin", "dest", "ep_len", "ep_return", "ep_start", "done", "err", "reward")
    for k, step in enumerate(c.steps):
        what = f"record {pattern} max_steps={max_steps} step {k}"
        acts = [actions_of(e, step) for e in envs]
        for e in envs:
            refuel(e, step)
        rbs[0].begin(acts[0])
        rbs[0].step_end(acts[0], cuts[0], max_steps)
        rbs[1].begin(acts[1])
        envs[1].step(acts[1])
        rbs[1].end(cuts[1], max_steps, reset=True)
        torch.cuda.synchronize()
        assert torch.equal(cuts[0], cuts[1]), what
        for f in fields:
            assert torch.equal(getattr(envs[0], f), getattr(envs[1], f)), f"{what}: {f}"
        for u, v in zip(envs[0].done_list(), envs[1].done_list()):
            assert torch.equal(u, v), what
        if k == 0:
            check_done_list(envs[0], step, what)
            cut = cuts[0].cpu().numpy()
            a = step.after
            raised = a.err != 0
            too_long = (a.ep_len >= max_steps) if max_steps > 0 else np.zeros(n, bool)
            np.testing.assert_array_equal(cut, (raised | too_long).astype(np.uint8), err_msg=f"{what}: cut")
            if max_steps == 0:
                st = O.OracleState(n)
                for f in A.FIELDS:
                    getattr(st, f)[:] = getattr(a, f)
                O.reset(A.oracle_world(O), st, mask=cut, seed=A.SEED, epoch=0)
                keep = cut == 0
                want = RestartedStep(st, a, keep, step)
                check_state(envs[0], want, what + " vs oracle")
    assert envs[0].counters == envs[1].counters == (c.t0 + 2, 2)
    s0, s1 = envs[0].episode_stats().clone(), envs[1].episode_stats().clone()
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64))
    assert rbs[0].size == rbs[1].size == 2 * n
    B = rbs[0].size
    for t in (0, 5):
        outs = [MiniBatch(B, envs[0].obs_size, envs[0].device) for _ in range(2)]
        for rb, out in zip(rbs, outs):
            rb.sample(out, t=t)
        torch.cuda.synchronize()
        for name in ("obs", "next_obs", "act", "rew", "done", "weight"):
            assert torch.equal(getattr(outs[0], name), getattr(outs[1], name)), (t, name)
        assert float(outs[0].weight.sum()) > 0


class RestartedStep:
    """check_state's view of a recorded step: the oracle's step, then the cut envs restarted
    (state from reset; ep_return, length, reward, done and err cleared; stamped t + 1)."""

    def __init__(self, st, after, keep, step):
        self.after = SimpleNamespace(
            **{f: getattr(st, f).copy() for f in A.FIELDS},
            reward=np.where(keep, after.reward, 0.0), done=np.where(keep, after.done, 0),
            err=np.where(keep, after.err, 0), ep_return=np.where(keep, after.ep_return, np.float32(0)),
            ep_len=np.where(keep, after.ep_len, 0))
        t_next = np.array((step.t + 1) & 0xFFFFFFFF, np.uint32).view(np.int32)
        self.exp = SimpleNamespace(start=np.where(keep, step.exp.start, t_next).astype(np.int32))
