"""The replay ring, its sampler and the update that draws its own batch, at every edge, bit for bit
against the C oracle (O.ReplayMemory, O.replay_pick).

The other suites read the ring at two shapes, once, after seven steps. Here scripted scenarios
(tests/replay_support.py; test_replay_support_cpu.py holds them to their claims) choose which envs
raise and which finish, and tag every stored transition through its fuel, which reaches:

* every writer of the ring (se_replay_begin, se_policy_record, se_policy_record_f32 for s;
  se_replay_end, its 4-wide kernel, se_replay_end_reset and se_step_record in one launch and in its
  two-launch fallback for s') at rings of cap == n, cap == n + 1, n < 4, a wrap inside a pass at
  every step, a cut mask that is not 4-byte aligned and none at all, 8 and 9 groups per thread of
  the step kernel; the whole ring is read after every step, so a stale half of an overwritten
  slot shows at the step where it happens;
* the sampler at the 4^k Feistel domain edges +-1, from an empty ring up, with B not a multiple
  of 64 and beyond the ring's size, part-filled rings, both ends of the key range from the host
  and from the device, a full LDS port table (P = 254), and flag patterns that send every row to
  its second, fourth or no try;
* se_qtrain_step_replay on such rings against se_replay_sample + se_qtrain_step(_policy), and
  the update of a batch whose every weight is 0: loss 0, Adam on a zero gradient.

No tolerances: every comparison is exact.
"""
import numpy as np
import pytest

import replay_support as R

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

NAMES = ("obs", "next_obs", "act", "rew", "done", "weight")
STATE = ("x", "y", "fuel", "cargo", "origin", "dest", "ep_start", "ep_return", "done", "err", "reward")


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
    while _OPEN:  # agents / buffers before their env, also when the test failed
        _OPEN.pop().close()


def make_env(monkeypatch, n, P=5, auto_reset=False, blocks=None, nt=None, order=None):
    from shippingenv_amd.vec import VecEnv

    for name, v in (("SHIPENV_STEP_BLOCKS", blocks), ("SHIPENV_NT_LOADS", nt), ("SHIPENV_POLICY_ORDER", order)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    env = VecEnv(n, auto_reset=auto_reset, **R.world(P).env_kwargs())
    _OPEN.append(env)
    env.reset()
    return env


def make_ring(env, cap):
    from shippingenv_amd.dqn import ReplayBuffer

    rb = ReplayBuffer(env, cap)
    _OPEN.append(rb)
    return rb


def rows(world, env):
    """preprocess_state rows of the env's current state, from the oracle."""
    torch.cuda.synchronize()
    st = O.OracleState(env.n)
    st.x[:] = env.x.cpu().numpy()
    st.y[:] = env.y.cpu().numpy()
    st.fuel[:] = env.fuel.cpu().numpy()
    for f in ("origin", "dest"):
        v = getattr(env, f).cpu().numpy().astype(np.int32)
        getattr(st, f)[:] = np.where(v == 255, -1, v)
    return O.observe(world, st)


def put_fuel(env, fuel):
    env.fuel.copy_(torch.from_numpy(np.array(fuel, np.float64)))  # a copy: the script's arrays are read-only


def actions_of(env, acts):
    return torch.from_numpy(np.array(acts, np.int32)).to(env.device)


F_GUARD, I_GUARD, SPARE = -12345.0, -77, 64


class Guarded:
    """MiniBatch's tensors as the leading B rows of buffers with 64 more rows of a sentinel: a
    sampler that wrote past row B (the rest of its last 64-row workgroup) would show."""

    def __init__(self, B, width, device):
        self.batch = B
        self._full = {}
        for name in NAMES:
            shape = (B + SPARE, width) if name in ("obs", "next_obs") else (B + SPARE,)
            fill, dtype = (I_GUARD, torch.int64) if name == "act" else (F_GUARD, torch.float32)
            full = torch.full(shape, fill, dtype=dtype, device=device)
            self._full[name] = full
            setattr(self, name, full[:B])

    def host(self):
        torch.cuda.synchronize()
        for name in NAMES:
            full = self._full[name]
            fill = I_GUARD if name == "act" else F_GUARD
            assert bool((full[self.batch:] == fill).all()), f"{name}: written past row {self.batch}"
        return {name: getattr(self, name).cpu().numpy() for name in NAMES}


def read(rb, env, B, t, dev_t=False):
    """A minibatch of B rows under key t, from the host or from a device counter (uint32 viewed
    as int32, beside a host t that must then be ignored)."""
    out = Guarded(B, env.obs_size, env.device)
    if dev_t:
        ctr = torch.from_numpy(np.array([t], np.uint32).view(np.int32)).to(env.device)
        rb.sample(out, t=12345, t_dev=ctr)
    else:
        rb.sample(out, t=t)
    return out.host()


def check_batch(got, mem, B, t, what):
    want = mem.sample(B, seed=R.SEED, t=t)
    for name, w in zip(NAMES, want):
        np.testing.assert_array_equal(got[name], w, err_msg=f"{what}: {name}")
    dead = got["weight"] == 0
    assert bool(((got["weight"] == 1) | dead).all()), what
    for name in NAMES[:5]:  # a weight-0 row is zeros throughout, the port block included
        assert not got[name][dead].any(), f"{what}: {name} of a weight-0 row"


def full_read(rb, mem, env, t, what):
    """Every stored transition once: B = size rows; the flagged slots give weight-0 rows."""
    assert rb.size == mem.size, what
    if mem.size:
        check_batch(read(rb, env, mem.size, t), mem, mem.size, t, f"{what}: full read")


# ---------------------------------------------------------------------- 1. every writer, every geometry
def cut_buffer(env, mode):
    if mode == "none":
        return None
    if mode == "odd":  # one byte into its buffer: not 4-byte aligned
        buf = torch.full((env.n + 1,), 7, dtype=torch.uint8, device=env.device)
        cut = buf[1:1 + env.n]
        assert cut.data_ptr() % 4 == 1
        return cut
    cut = torch.full((env.n,), 7, dtype=torch.uint8, device=env.device)
    assert cut.data_ptr() % 4 == 0
    return cut


def run_ring(monkeypatch, n, cap, writer, *, max_steps, auto_reset, cut_mode="aligned", blocks=None, nt=None,
             segments=None):
    """The scripted scenario through `writer` on one env and through se_step + reset(cut) on a
    shadow env that feeds the oracle's memory; everything compared after every step."""
    sc = R.scenario(5, n, R.steps_for(n, cap), auto_reset=auto_reset, max_steps=max_steps,
                    reset_cut=cut_mode != "none")
    env = make_env(monkeypatch, n, auto_reset=auto_reset, blocks=blocks, nt=nt)
    shadow = make_env(monkeypatch, n, auto_reset=auto_reset)
    if segments is not None:  # 4 waves x groups per thread, of the one workgroup
        assert env.done_segments == segments
    world = R.world(5).oracle(O)
    rb = make_ring(env, cap)
    mem = O.ReplayMemory(cap, env.obs_size)
    cut = cut_buffer(env, cut_mode)
    for s in sc:
        what = f"{writer} n={n} cap={cap} max_steps={max_steps} cut={cut_mode} step {s.t}"
        for e in (env, shadow):
            put_fuel(e, s.fuel)
        a = actions_of(env, s.actions)
        s_rows = rows(world, shadow)
        rb.begin(a)
        if writer == "end_then_reset":
            env.step(a)
            rb.end(cut, max_steps)
            if cut is not None:
                env.reset(cut)
        elif writer == "end_reset":
            env.step(a)
            rb.end(cut, max_steps, reset=True)
        else:
            rb.step_end(a, cut, max_steps)
        shadow.step(a)
        torch.cuda.synchronize()
        r, d, e = (getattr(shadow, f).cpu().numpy() for f in ("reward", "done", "err"))
        want_cut = e != 0
        if max_steps > 0:
            want_cut = want_cut | (shadow.ep_len.cpu().numpy() >= max_steps)
        # the script's claims hold on the device as they do on the oracle
        np.testing.assert_array_equal(e != 0, s.role == R.RAISE, err_msg=f"{what}: raise")
        np.testing.assert_array_equal(d != 0, s.role == R.FINISH, err_msg=f"{what}: finish")
        np.testing.assert_array_equal(want_cut, s.cut, err_msg=f"{what}: the script's cut")
        mem.push(s_rows, s.actions, r, rows(world, shadow), d, e != 0)
        if cut is not None:
            np.testing.assert_array_equal(cut.cpu().numpy(), want_cut.astype(np.uint8), err_msg=f"{what}: cut")
            shadow.reset(torch.from_numpy(want_cut.astype(np.uint8)))
        torch.cuda.synchronize()
        for f in STATE:
            assert torch.equal(getattr(env, f), getattr(shadow, f)), f"{what}: {f}"
        full_read(rb, mem, env, s.t, what)
    assert rb.size == cap


def _id(g):
    return f"{g[0]}x{g[1]}"


@pytest.mark.parametrize("max_steps", [0, 2])
@pytest.mark.parametrize("writer", ["end_then_reset", "end_reset"])
@pytest.mark.parametrize("geometry", R.SCALAR + R.WIDE, ids=_id)
def test_begin_step_end_at_every_geometry(monkeypatch, geometry, writer, max_steps):
    """se_replay_begin + se_step + se_replay_end then reset(cut), and + se_replay_end_reset: the
    scalar kernel's rings and the 4-wide kernel's. max_steps = 2 runs on the auto-reset env (it
    needs the episode-start stamps), max_steps = 0 on the plain one."""
    n, cap = geometry
    assert R.takes_wide_kernel(n, cap) == (geometry in R.WIDE)
    run_ring(monkeypatch, n, cap, writer, max_steps=max_steps, auto_reset=max_steps > 0)


@pytest.mark.parametrize("max_steps", [0, 2])
@pytest.mark.parametrize("writer", ["end_then_reset", "end_reset"])
def test_end_with_an_unaligned_cut_mask(monkeypatch, writer, max_steps):
    """(8, 12) would take the 4-wide kernel; a cut mask at an odd address sends it to the scalar one."""
    n, cap = R.ODD_CUT
    run_ring(monkeypatch, n, cap, writer, max_steps=max_steps, auto_reset=max_steps > 0, cut_mode="odd")


def test_end_without_a_cut_mask(monkeypatch):
    """cut = None: the record is written, nothing is cut and no env restarts."""
    n, cap = R.ODD_CUT
    run_ring(monkeypatch, n, cap, "end_then_reset", max_steps=0, auto_reset=False, cut_mode="none")


@pytest.mark.parametrize("max_steps", [0, 2])
@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("geometry", R.WIDE, ids=_id)
def test_step_record_in_one_launch(monkeypatch, geometry, nt, max_steps):
    """se_step_record where every group's ring slots are consecutive: the step kernel's record
    instantiation, with temporal and with nontemporal state loads."""
    n, cap = geometry
    run_ring(monkeypatch, n, cap, "step_end", max_steps=max_steps, auto_reset=True, nt=nt)


@pytest.mark.parametrize("max_steps", [0, 2])
@pytest.mark.parametrize("geometry,segments", [(R.ITERS_8, 32), (R.ITERS_9, 36)], ids=["iters8", "iters9"])
def test_step_record_at_the_groups_per_thread_limit(monkeypatch, geometry, segments, max_steps):
    """One workgroup (SHIPENV_STEP_BLOCKS=1): 8 groups per thread is the last one-launch case (32
    cut bits per thread), 9 the first that falls back to se_step + se_replay_end_reset."""
    n, cap = geometry
    run_ring(monkeypatch, n, cap, "step_end", max_steps=max_steps, auto_reset=True, blocks="1", segments=segments)


@pytest.mark.parametrize("max_steps", [0, 2])
@pytest.mark.parametrize("geometry,cut_mode", [(g, "aligned") for g in R.RECORD_FALLBACK] + [(R.ODD_CUT, "odd")],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_step_record_fallback(monkeypatch, geometry, cut_mode, max_steps):
    """se_step_record's two launches: n, the capacity or the cut mask's address not a multiple of 4."""
    n, cap = geometry
    run_ring(monkeypatch, n, cap, "step_end", max_steps=max_steps, auto_reset=True, cut_mode=cut_mode)


@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("P", [5, 64])
@pytest.mark.parametrize("geometry", R.POLICY, ids=_id)
def test_policy_record_writes_the_state_side(monkeypatch, geometry, P, precision, order):
    """se_policy_record / se_policy_record_f32 as the writer of s and a, the ring wrapping inside
    a policy tile, in position order and in the sea-first visiting order. The shadow runs
    se_policy / se_policy_f32 with the same weights and t: its actions are the recorder's and
    are what the oracle's memory receives. The script gives the fuel only (the finishing fuel
    and the tags); max_steps = 2 cuts episodes whether or not a step raised."""
    from shippingenv_amd.policy import DQNNetwork, QPolicy

    n, cap = geometry
    max_steps, eps = 2, 0.5
    env = make_env(monkeypatch, n, P=P, auto_reset=True, order=order)
    shadow = make_env(monkeypatch, n, P=P, auto_reset=True, order=order)
    world = R.world(P).oracle(O)
    torch.manual_seed(11)
    model = DQNNetwork(env.obs_size, env.action_space_size)
    pols = []
    for e in (env, shadow):
        pol = QPolicy(e, model)
        _OPEN.append(pol)
        pols.append(pol)
    rb = make_ring(env, cap)
    mem = O.ReplayMemory(cap, env.obs_size)
    cut = cut_buffer(env, "aligned")
    one_launch = R.takes_wide_kernel(n, cap)
    cuts = 0
    for t in range(R.steps_for(n, cap)):
        what = f"policy {precision} P={P} n={n} cap={cap} order={order} step {t}"
        fuel = R.fuel_for(R.roles(n, t), t)
        for e in (env, shadow):
            put_fuel(e, fuel)
        s_rows = rows(world, shadow)
        a = pols[0].act_record(rb, eps, t, precision=precision)
        a_s = pols[1].act(eps, t, precision=precision)
        assert torch.equal(a, a_s), f"{what}: actions"
        if one_launch:
            rb.step_end(a, cut, max_steps)
        else:
            env.step(a)
            rb.end(cut, max_steps, reset=True)
        shadow.step(a_s)
        torch.cuda.synchronize()
        r, d, e = (getattr(shadow, f).cpu().numpy() for f in ("reward", "done", "err"))
        want_cut = (e != 0) | (shadow.ep_len.cpu().numpy() >= max_steps)
        mem.push(s_rows, a_s.cpu().numpy(), r, rows(world, shadow), d, e != 0)
        np.testing.assert_array_equal(cut.cpu().numpy(), want_cut.astype(np.uint8), err_msg=f"{what}: cut")
        cuts += int(want_cut.sum())
        shadow.reset(torch.from_numpy(want_cut.astype(np.uint8)))
        torch.cuda.synchronize()
        for f in STATE:
            assert torch.equal(getattr(env, f), getattr(shadow, f)), f"{what}: {f}"
        full_read(rb, mem, env, t, what)
    assert cuts > 0 and rb.size == cap


# ---------------------------------------------------------------------- 2. the sampler
def filled_ring(monkeypatch, size, cap, P, flags):
    """A ring of exactly `size` transitions from one scripted step of `size` envs (none: no
    step), the oracle's memory of the same, and the step. flags: the envs to flag (a bool
    array), or None for the script's own roles."""
    n = size if size else 4
    env = make_env(monkeypatch, n, P=P)
    rb = make_ring(env, cap if size else n + cap)
    mem = O.ReplayMemory(rb.capacity, env.obs_size)
    if not size:
        assert rb.size == 0
        return env, rb, mem, None
    fixed = None if flags is None else R.ring_roles(size, flags)
    (s,) = R.scenario(P, size, 1, auto_reset=False, fixed_roles=fixed)
    world = R.world(P).oracle(O)
    put_fuel(env, s.fuel)
    a = actions_of(env, s.actions)
    s_rows = rows(world, env)
    rb.begin(a)
    env.step(a)
    rb.end()
    torch.cuda.synchronize()
    r, d, e = (getattr(env, f).cpu().numpy() for f in ("reward", "done", "err"))
    np.testing.assert_array_equal(e != 0, s.role == R.RAISE)
    np.testing.assert_array_equal(d != 0, s.role == R.FINISH)
    mem.push(s_rows, s.actions, r, rows(world, env), d, e != 0)
    assert rb.size == mem.size == size
    return env, rb, mem, s


def check_tags(got, s, B, size, what):
    """Among the weight-1 rows the tags (obs[:, 2]) are distinct and none is a flagged
    transition's; with no flags and B >= size they are exactly the stored set."""
    live = got["weight"] == 1
    tag = got["obs"][live, 2]
    if s is None:
        assert not live.any(), what
        return
    flagged = s.role == R.RAISE
    tagged = tag[tag != np.float32(R.FINISH_FUEL)]
    assert len(np.unique(tagged)) == len(tagged), f"{what}: a transition drawn twice"
    assert not np.isin(tag, s.tags[flagged].astype(np.float32)).any(), f"{what}: a flagged transition drawn"
    assert int(live.sum()) <= min(B, size - int(flagged.sum())), what
    if not flagged.any() and B >= size:
        np.testing.assert_array_equal(np.sort(tag), np.sort(s.fuel.astype(np.float32)), err_msg=what)


def sweep(env, rb, mem, s, size, batch_list, what):
    for B in batch_list:
        for t in R.KEYS:
            for dev_t in (False, True):
                w = f"{what} B={B} t={t} dev_t={dev_t}"
                got = read(rb, env, B, t, dev_t)
                check_batch(got, mem, B, t, w)
                check_tags(got, s, B, size, w)


def _table():
    out = [(size, 0) for size in R.SIZES] + [(size, 5) for size in R.PARTIAL]
    return sorted(out)


@pytest.mark.parametrize("flags", ["none", "scripted"])
@pytest.mark.parametrize("size,spare", _table())
def test_sampler_at_every_domain_edge(monkeypatch, size, spare, flags):
    """Ring sizes at the 4^k Feistel domain edges +-1 (spare = 5: the same in a ring of size + 5
    slots, so a sampler reading the capacity shows), B from 1 past 4 size + 1, both ends of the
    key range, from the host and from the device. flags: no transition flagged, or the script's
    own raise roles."""
    none = np.zeros(size, bool) if flags == "none" else None
    env, rb, mem, s = filled_ring(monkeypatch, size, size + spare, 5, none)
    sweep(env, rb, mem, s, size, R.batches(size), f"size={size} cap={rb.capacity}")


@pytest.mark.parametrize("size", R.SIZES_P64)
def test_sampler_with_64_ports(monkeypatch, size):
    env, rb, mem, s = filled_ring(monkeypatch, size, size, 64, None)
    assert env.obs_size == 262
    sweep(env, rb, mem, s, size, R.batches(size), f"P=64 size={size}")


def test_sampler_with_a_full_port_table(monkeypatch):
    """P = 254: the sampler's LDS port table is exactly full, rows of 1022 floats."""
    env, rb, mem, s = filled_ring(monkeypatch, R.P254_SIZE, R.P254_SIZE, 254, None)
    assert env.obs_size == 6 + 4 * 254
    sweep(env, rb, mem, s, R.P254_SIZE, R.P254_BATCHES, "P=254")


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("size", [s for s in R.SIZES if s >= 4])
def test_sampler_flag_patterns(monkeypatch, size, pattern):
    """B = size // 4, the flags peeled with the oracle for this (size, B, key): every row drawn at
    its first try, its second, its fourth, at none, at a mixed depth, or the whole ring flagged."""
    B = size // 4
    for t in R.KEYS:
        flags = R.pattern_flags(O, pattern, size, B, t)
        env, rb, mem, s = filled_ring(monkeypatch, size, size, 5, flags)
        depth = R.pattern_depth(pattern, B)
        live = 0 if pattern == "everything" else int((depth < 4).sum())
        for dev_t in (False, True):
            what = f"size={size} {pattern} t={t} dev_t={dev_t}"
            got = read(rb, env, B, t, dev_t)
            check_batch(got, mem, B, t, what)
            check_tags(got, s, B, size, what)
            assert int(got["weight"].sum()) == live, what
        while _OPEN:  # this key's ring and env
            _OPEN.pop().close()


# ---------------------------------------------------------------------- 3. the update that draws its own batch
@pytest.mark.parametrize("host_t", [True, False])
@pytest.mark.parametrize("with_policy", [True, False])
@pytest.mark.parametrize("name", list(R.UPDATE_CASES))
def test_update_drawing_its_own_batch_on_edge_rings(monkeypatch, name, with_policy, host_t):
    """se_qtrain_step_replay against se_replay_sample + se_qtrain_step_policy / se_qtrain_step on
    a twin, three updates, on the scripted rings: fewer transitions than the batch, every first
    candidate flagged (pick_resolve's later tries; a last tile of one row), mixed depths, every
    row at weight 0, an empty ring. Loss, parameters, both Adam moments, the counters and the
    policy's Q rows agree bit for bit. Where every weight is 0 the update is Adam on a zero
    gradient: the loss is exactly 0, parameters and moments stay as they were, and the counters
    still advance."""
    from shippingenv_amd.dqn import VecDQNAgent

    size, batch, _, all_zero = R.UPDATE_CASES[name]
    flags = R.update_flags(O, name)
    agents = []
    for _ in range(2):
        n = size if size else 4
        env = make_env(monkeypatch, n, auto_reset=True)
        torch.manual_seed(4)
        agent = VecDQNAgent(env, graph=False, batch_size=batch, epsilon=0.6, target_update_every=0, memory_size=n)
        _OPEN.append(agent)
        if size:
            (s,) = R.scenario(5, size, 1, auto_reset=True, fixed_roles=R.ring_roles(size, flags))
            put_fuel(env, s.fuel)
            acts = actions_of(env, s.actions)
            agent.memory.begin(acts)
            env.step(acts)
            agent.memory.end(agent.cut, 0)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(agent.cut.cpu().numpy() != 0, flags)
        assert agent.memory.size == size
        agents.append(agent)
    a, b = agents
    for p, q in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q)
    p0 = [p.detach().clone() for p in a.model.parameters()]
    for k in range(3):
        assert k == R.UPDATE_KEYS[k] == int(a._ctr[0].item())
        a.trainer.step_replay(a.memory, batch, a.gamma, a._ctr, a._loss, a.policy if with_policy else None,
                              t=k if host_t else None)
        b.memory.sample(b.batch, t_dev=b._ctr)
        if with_policy:
            b.trainer.step_policy(b.batch, b.gamma, b._ctr, b._loss, b.policy)
        else:
            b.trainer.step(b.batch, b.gamma, b._ctr, b._loss)
            b._ctr.add_(1)
        torch.cuda.synchronize()
        live = int(b.batch.weight.sum().item())
        want = mem_live(size, batch, flags, k)
        assert live == want, (name, k, live, want)
        assert a._ctr.tolist() == [k + 1, k + 1], k
        assert int(b._ctr[0].item()) == k + 1, k
        assert a._loss.item() == b._loss.item(), k
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p, q), k
        for p, q in zip(a.trainer.exp_avg + a.trainer.exp_avg_sq, b.trainer.exp_avg + b.trainer.exp_avg_sq):
            assert torch.equal(p, q), k
        if all_zero:
            assert live == 0
            for ag in agents:
                assert ag._loss.item() == 0.0, (name, k, ag._loss.item())
                for p, q in zip(ag.model.parameters(), p0):
                    assert torch.equal(p, q), (name, k, "a parameter moved on a zero gradient")
                for m in ag.trainer.exp_avg + ag.trainer.exp_avg_sq:
                    assert torch.equal(m, torch.zeros_like(m)), (name, k, "an Adam moment moved on a zero gradient")
        else:
            assert live > 0
    if not all_zero:
        assert not all(torch.equal(p, q) for p, q in zip(a.model.parameters(), p0))
    if with_policy:
        qs = []
        for ag in agents:
            q = torch.full((ag.env.n, ag.env.action_space_size), float("nan"), device=ag.env.device)
            ag.policy.act(0.0, 0, q_out=q)
            qs.append(q)
        assert torch.equal(qs[0], qs[1])


def mem_live(size, batch, flags, t):
    """The rows the oracle's sampler draws at weight 1."""
    inv = np.concatenate([flags, [False]]).astype(np.uint8)
    return int((O.replay_pick(size, batch, inv, seed=R.SEED, t=t) >= 0).sum())
