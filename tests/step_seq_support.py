"""What the test_gpu_step_seq_*.py files share: the error codes and field names, the env
variables' context manager, host-side states, snapshots and their exact comparison, and the
method of the state-only step's suites: a twin env stepped by K VecEnv.step calls (recorded step
by step), the same trace from the C oracle, and one step_seq call that must end in the same bits,
with TAIL plain steps after it. A `world` is anything with env(n, seed=, env_id_base=, **environ)
and oracle(O): the golden map of test_gpu_step_seq_lean or the hand-built map of
test_gpu_step_seq_trim."""
import contextlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

STATE = ("x", "y", "fuel", "cargo", "origin", "dest")
OUTPUTS = ("reward", "done", "err")
NONE = 255
OK, OOB, SAME_PORT, NOT_AT_PORT, AMOUNT, NO_DEST, NO_PORTS, BAD_INDEX = 0, 1, 2, 4, 5, 6, 8, 9
TAIL = 2  # plain steps after the fused run


@pytest.fixture(scope="module")
def gpu_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from shippingenv_amd import build

    build.build(verbose=False)


@contextlib.contextmanager
def environ(**kv):
    """Set variables the library reads at se_create; put the old values back afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def empty_state(n):
    return {"x": np.zeros(n, np.int32), "y": np.zeros(n, np.int32), "fuel": np.zeros(n, np.float64),
            "cargo": np.zeros(n, np.int32), "origin": np.full(n, NONE, np.int32), "dest": np.full(n, NONE, np.int32)}


def load(env, st, t0=0):
    """Write the env's tensors and put its step counter at t0."""
    for f, dt in (("x", np.uint8), ("y", np.uint8), ("fuel", np.float64), ("cargo", np.int32),
                  ("origin", np.uint8), ("dest", np.uint8)):
        getattr(env, f).copy_(torch.from_numpy(st[f].astype(dt)))
    env.reward.zero_()
    env.done.zero_()
    env.err.zero_()
    env.set_counters(t0, 0)


def snapshot(env):
    """Every field a step writes, as host arrays: integers as int32, fuel f64, reward f32."""
    torch.cuda.synchronize()
    out = {f: getattr(env, f).cpu().numpy() for f in STATE + OUTPUTS}
    return {f: (v if f in ("fuel", "reward") else v.astype(np.int32)) for f, v in out.items()}


def assert_same(got, want, what):
    """Exact, fuel by its bits."""
    for f in STATE + OUTPUTS:
        g, w = (got[f].view(np.int64), want[f].view(np.int64)) if f == "fuel" else (got[f], want[f])
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {f}")


def device_rows(env, acts):
    """[rows, n] device view of the host rows at a padded stride ld > n (a multiple of 4)."""
    rows, n = acts.shape
    ld = ((n + 3) & ~3) + 8
    buf = torch.full((rows, ld), -99, dtype=torch.int32, device=env.device)  # padding: a bad index if ever read
    buf[:, :n].copy_(torch.from_numpy(acts))
    return buf[:, :n]


def twin_trace(world, init, acts, seed=22, env_id_base=0, t0=0):
    """trace[k]: the snapshot after step k of len(acts) VecEnv.step calls from init."""
    env = world.env(len(init["x"]), seed=seed, env_id_base=env_id_base)
    load(env, init, t0)
    dev = device_rows(env, acts)
    trace = []
    for k in range(len(acts)):
        env.step(dev[k].contiguous())
        trace.append(snapshot(env))
    env.close()
    for s in trace:
        for v in s.values():
            v.setflags(write=False)
    return trace


def oracle_trace(O, world, init, acts, seed=22, env_id_base=0, t0=0):
    """The same trace from the C oracle's stepper (origin / dest None is -1 there)."""
    n = len(init["x"])
    w = world.oracle(O)
    st = O.OracleState(n)
    for f in STATE:
        getattr(st, f)[:] = np.where(init[f] == NONE, -1, init[f]) if f in ("origin", "dest") else init[f]
    trace = []
    for k in range(len(acts)):
        O.step(w, st, actions=np.ascontiguousarray(acts[k]), seed=seed, env_id_base=env_id_base, t=(t0 + k) & 0xffffffff)
        s = {f: getattr(st, f).copy() for f in STATE + ("done", "err")}
        for f in ("origin", "dest"):
            s[f] = np.where(s[f] < 0, NONE, s[f]).astype(np.int32)
        s["reward"] = st.reward.astype(np.float32)
        trace.append(s)
    return trace


def run_fused(b, init, dev, trace, K, mark_after, what, t0=0):
    """One step_seq of rows 0 .. K-1 from init (counter t0) equals the twin after K steps, and
    after TAIL plain steps more."""
    load(b, init, t0)
    if mark_after is None:
        r, d, e = b.step_seq(dev[:K])
    else:
        ev = torch.cuda.Event(enable_timing=True)
        r, d, e = b.step_seq(dev[:K], mark=ev, mark_after=mark_after)
    assert r.data_ptr() == b.reward.data_ptr() and d.data_ptr() == b.done.data_ptr() and e.data_ptr() == b.err.data_ptr()
    assert_same(snapshot(b), trace[K - 1], f"{what} K={K} mark_after={mark_after}: after the fused run")
    assert b.counters[0] == t0 + K
    for k in range(K, K + TAIL):
        b.step(dev[k].contiguous())
    assert_same(snapshot(b), trace[K + TAIL - 1], f"{what} K={K} mark_after={mark_after}: {TAIL} plain steps later")


def steps_before_last(init, acts, trace, K):
    """(k, before, action row, after) of the inner steps k < K - 1."""
    for k in range(K - 1):
        yield k, (init if k == 0 else trace[k - 1]), acts[k], trace[k]
