"""se_rollout_qnet, QPolicy.rollout, VecDQNAgent.rollout and .evaluate on the GPU, bit for bit (ret and
fuel as uint64).

The kernel is held to the plain-Python restatement of tests/qnet_rollout_support.py, which
tests/test_qnet_rollout_cpu.py pins to plan_support's scripted rollout and to the reference's
validity bits, and whose worlds and ships it shows to reach every status and branch. The restatement
needs no floating-point network: at epsilon = 1 no Q is read, and the integer and zero networks'
Q are exact in bf16 x bf16 -> f32. Then the two equalities of include/shipenv.h against the
library's own calls: se_rollout_plan fed the emitted rows (on every case), and se_policy on the
ships the plan gives, for a torch-default-init network. Then what the call must leave alone, its
footprint in a guarded arena, its refusals, the grid-stride loop, repacked weights, a captured call
and evaluate()."""
import ctypes as C

import numpy as np
import pytest

import dqn_numeric_support as NS
import footprint_support as F
import qnet_rollout_support as QS
from test_gpu_rollout import load_state
from test_gpu_rollout_plan import assert_untouched, snapshot
from test_gpu_sarsa import ships_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

POISON = -7
FIELDS, SHIP = QS.FIELDS, QS.SHIP
CHOOSERS = [(None, 1.0), ("integer", 0.0), ("integer", 0.3), ("zero", 0.0), ("zero", 0.3)]


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
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error is sticky: end the session instead of launching more
        _OPEN.clear()
        pytest.exit(f"the device reported an error, nothing more is run: {e}", returncode=3)
    while _OPEN:  # handles before their env, also when the test failed
        _OPEN.pop().close()


def keep(obj):
    _OPEN.append(obj)
    return obj


def lib():
    from shippingenv_amd import _native as N

    return N.lib()


def make_policy(world, ships, net=None, seed=QS.SEED):
    """(env holding the ships, QPolicy of the IntNet `net`; None: the zero network)."""
    from shippingenv_amd.policy import QPolicy

    env = keep(world.env(len(ships), seed=seed))
    load_state(env, ships_state(ships))
    net = QS.IntNet.zero(world.P) if net is None else net
    return env, keep(QPolicy(env, net.model()))


def world_policy(name, net):
    w = QS.WORLDS[name][0]
    return make_policy(w, QS.ships_for(w), None if net is None else QS.NETS[net](w.P))


def numpy_result(res, act=True):
    out = {f: getattr(res, f).cpu().numpy() for f in FIELDS + (("act",) if act else ())}
    assert out["ret"].dtype == np.float64 and out["fuel"].dtype == np.float64
    assert all(v.dtype == np.int32 for f, v in out.items() if f not in ("ret", "fuel"))
    return out


def assert_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        if f in ("ret", "fuel"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {f}")


def policy_bytes(pol):
    """The weights, and the two packed images as far as a caller can see them: every Q row of the
    full image (q_out; not on a 256 x 256 map, where se_policy's full image and the world together
    exceed the LDS) and the compact image's greedy actions."""
    env = pol.env
    out = [t.cpu().numpy().copy().view(np.uint8) for t in pol._w]
    if env.H * env.W < 1 << 15:
        q = torch.zeros((env.n, env.action_space_size), dtype=torch.float32, device=env.device)
        pol.act(0.0, 0, q_out=q)
        out.append(q.cpu().numpy().copy().view(np.uint8))
    return out + [pol.act(0.0, 0).cpu().numpy().copy()]


def assert_policy_untouched(pol, before, what=""):
    for a, b in zip(policy_bytes(pol), before):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: the weights or a packed image changed")


def assert_plan_equality(env, src, res, got, ids=None, base=0, what=""):
    """include/shipenv.h's plan equality: se_rollout_plan under the same ids, fed the agent indices
    the call wrote, as they lie, with len = counted + raised."""
    played = (got["counted"] + got["raised"]).astype(np.int32)
    plan = env.rollout_plan(src, actions=res.act, lengths=played, ids=ids, rollout_base=base, return_end=True)
    want = {f: getattr(plan, f).cpu().numpy() for f in ("ret", "steps", "status", "raised", "first_err", "first_err_at") + SHIP}
    want["counted"] = want["steps"]
    assert_equal(got, want, f"plan equality {what}", ("ret", "counted", "raised", "first_err", "first_err_at") + SHIP)
    raised = got["status"] == QS.RAISED
    np.testing.assert_array_equal(got["status"][~raised], want["status"][~raised], err_msg=what)
    assert (want["status"][raised] == QS.END).all()
    for r in range(len(played)):  # an action at every position played, the pad behind
        assert (got["act"][:played[r], r] >= 0).all() and (got["act"][played[r]:, r] == QS.PAD).all(), (what, r)


# ----------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("net,eps", CHOOSERS)
@pytest.mark.parametrize("name", list(QS.WORLDS))
def test_kernel_equals_the_restatement(name, net, eps):
    """Every world's hand-placed ships under the explore law alone and under the integer and zero
    networks: every output, the action rows and `explored` included, and the plan equality."""
    w, m, steps = QS.WORLDS[name]
    env, pol = world_policy(name, net)
    before, pb = snapshot(env), policy_bytes(pol)
    src = QS.world_src(name)
    rolls, _ = QS.suite(O, name, net, eps)
    res = pol.rollout(src, steps=steps, epsilon=eps, rollout_base=QS.BASE, return_end=True, return_actions=True)
    assert res.act.shape == (steps, m)
    got = numpy_result(res)
    what = f"{name} net={net} eps={eps}"
    assert_equal(got, QS.expected(rolls, steps), what, FIELDS + ("act",))
    assert_plan_equality(env, src, res, got, base=QS.BASE, what=what)
    assert_untouched(env, before, what)
    assert_policy_untouched(pol, pb, what)


@pytest.mark.parametrize("steps", [0, 1, 2])
def test_short_runs(steps):
    """0, 1 and 2 positions on 67 rollouts (two tiles + 3): steps = 0 writes ret 0, counted 0, END."""
    env, pol = world_policy("hand", "integer")
    m, eps = 67, 0.3
    src = QS.world_src("hand", m)
    rolls, _ = QS.suite(O, "hand", "integer", eps, steps=steps, m=m)
    res = pol.rollout(src, steps=steps, epsilon=eps, rollout_base=QS.BASE, return_end=True, return_actions=True)
    got = numpy_result(res)
    assert_equal(got, QS.expected(rolls, steps), f"steps={steps}", FIELDS + ("act",))
    assert_plan_equality(env, src, res, got, base=QS.BASE, what=f"steps={steps}")
    if steps == 0:
        good = got["status"] != QS.BAD_SRC
        assert (got["ret"] == 0).all() and (got["counted"] == 0).all() and (got["status"][good] == QS.END).all()


def test_ids_are_the_streams():
    """64-bit ids against the restatement; duplicate ids give identical rollouts whatever the lane;
    ids = base + r is rollout_base; src=None; an empty batch; precision='f32' is not built."""
    w = QS.WORLDS["hand"][0]
    ships = QS.ships_for(w)
    net = QS.IntNet.integer(w.P)
    env, pol = make_policy(w, ships, net)
    m, steps, eps = 131, 12, 0.3
    rng = np.random.default_rng(11)
    src = rng.integers(0, env.n, m).astype(np.int32)
    src[[0, 64, m - 1]] = [-1, (1 << 31) - 1, env.n]
    ids = rng.choice([5, 6, (1 << 40) + 3, (1 << 63) - 1, 0], m).astype(np.int64)
    rolls = QS.rollouts(QS.Player(O, w.oracle(O), net), ships, src, steps, eps, ids)
    res = pol.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=999, return_end=True, return_actions=True)
    got = numpy_result(res)
    assert_equal(got, QS.expected(rolls, steps), "ids", FIELDS + ("act",))
    assert_plan_equality(env, src, res, got, ids=ids, base=3, what="ids")
    assert (got["status"] == QS.BAD_SRC).sum() == 3
    same = numpy_result(pol.rollout(np.full(m, 9, np.int32), steps=steps, epsilon=eps, ids=np.full(m, (1 << 40) + 3),
                                    return_end=True, return_actions=True))
    for f in FIELDS:
        assert (same[f] == same[f][0]).all(), f
    assert (same["act"] == same["act"][:, :1]).all() and same["counted"][0] > 0
    good = np.clip(src, 0, env.n - 1).astype(np.int32)
    base = (1 << 32) - 100
    whole = numpy_result(pol.rollout(good, steps=steps, epsilon=eps, rollout_base=base, return_end=True), act=False)
    for lo, hi in ((0, 64), (96, 131), (m - 1, m)):
        part = numpy_result(pol.rollout(good[lo:hi], steps=steps, epsilon=eps, rollout_base=base + lo, return_end=True), act=False)
        assert_equal(part, {f: v[lo:hi] for f, v in whole.items()}, f"sub-batch [{lo}, {hi})")
    by_ids = numpy_result(pol.rollout(good, steps=steps, epsilon=eps, ids=base + np.arange(m), rollout_base=3, return_end=True), act=False)
    assert_equal(by_ids, whole, "ids = base + arange")
    every = pol.rollout(steps=2, return_end=True)
    assert every.ret.numel() == env.n and every.act is None
    none = pol.rollout(np.zeros(0, np.int32), steps=5, return_end=True, return_actions=True)
    assert all(getattr(none, f).numel() == 0 for f in FIELDS + ("act",)) and pol.rollout(np.zeros(0, np.int32)).x is None
    with pytest.raises(NotImplementedError):
        pol.rollout(steps=2, precision="f32")
    with pytest.raises(ValueError):
        pol.rollout(steps=2, precision="f16")


# ----------------------------------------------------------------- 2. the policy equality
@pytest.mark.parametrize("family", NS.FAMILIES)
def test_every_action_is_se_policy_on_the_ship_before_it(water, family):
    """A seeded network of every family of tests/dqn_numeric_support.py (default: torch's default
    init) on the default world, 67 rollouts of 8 positions from envs after a reset and 30 random
    steps, the first 39 of them with the fuels of dqn_numeric_support.FUELS in turn (three rounds:
    where the bf16 hi + lo split of the fuel changes behaviour). For each k, se_rollout_plan of the
    first k emitted actions gives the ships before position k; loaded into a scratch env,
    se_policy's greedy action there must equal row k for every rollout still playing. Nothing is
    left out, no tolerance."""
    from shippingenv_amd.policy import QPolicy
    from shippingenv_amd.vec import VecEnv

    n = m = 67
    steps = 8
    env = keep(VecEnv(n, seed=0))
    np.testing.assert_array_equal(env.water, water)
    env.reset()
    for t in range(30):
        env.step(env.gen_actions(t))
    edge = 3 * len(NS.FUELS)
    env.fuel[:edge] = torch.as_tensor(np.tile(NS.FUELS, 3), device=env.device)
    model = NS.make_family(family, env.obs_size, env.action_space_size, seed=1234)
    pol = keep(QPolicy(env, model))
    scratch = keep(VecEnv(n, seed=0))
    spol = keep(QPolicy(scratch, model))
    src = torch.arange(m, dtype=torch.int32, device=env.device)
    ids = (1 << 33) + 7 * np.arange(m)
    res = pol.rollout(src, steps=steps, epsilon=0.0, ids=ids, return_end=True, return_actions=True)
    got = numpy_result(res)
    assert_plan_equality(env, src, res, got, ids=ids, what=family)
    played = got["counted"] + got["raised"]
    compared = 0
    for k in range(steps):
        playing = played > k
        assert ((got["act"][k] != QS.PAD) == playing).all()
        if not playing.any():
            break
        ships = env.rollout_plan(src, actions=res.act, lengths=np.full(m, k, np.int32), ids=ids, return_end=True)
        st = ships_state(list(zip(*[getattr(ships, f).cpu().numpy().tolist() for f in SHIP])))
        load_state(scratch, st)
        chosen = spol.act(0.0, k).cpu().numpy()
        np.testing.assert_array_equal(got["act"][k][playing], chosen[playing], err_msg=f"position {k}")
        compared += int(playing.sum())
    assert compared > m * steps // 2 and len(np.unique(got["act"][got["act"] >= 0])) >= 3
    assert (got["explored"] == 0).all()


# ----------------------------------------------------------------- 3. what the call leaves alone
i32, f64, i64 = np.int32, np.float64, np.int64
OPTIONAL = ("act", "explored", "raised", "first_err", "first_err_at") + SHIP


@pytest.mark.parametrize("half", [0, 1], ids=["even-outputs", "odd-outputs"])
@pytest.mark.parametrize("m", [1, 33, 131])
def test_footprint_in_a_guarded_arena(m, half):
    """Every buffer of the call a view into one arena at its documented size between patterned
    guards: src and ids m entries, ret, counted and status m, each optional output m, the action
    rows [steps][ld] with ld = m rounded up to 4. The optional outputs alternate between wanted and
    NULL (`half` swaps them): the guards, the inputs and the env hold, the outputs that were not
    asked for and the ld - m columns behind each row keep their prefill, the others are the twin's."""
    from shippingenv_amd import _native as N
    from shippingenv_amd.policy import QPolicy

    w = QS.WORLDS["hand"][0]
    ships = QS.ships_for(w)
    n, steps, eps, ld = len(ships), 6, 0.3, (m + 3) // 4 * 4
    net = QS.IntNet.integer(w.P)
    extra = ([("src", i32, m), ("ids", i64, m), ("ret", f64, m), ("counted", i32, m), ("status", i32, m),
              ("act", i32, (steps, ld)), ("explored", i32, m)]
             + [(k, i32, m) for k in ("raised", "first_err", "first_err_at", "e_x", "e_y")] + [("e_fuel", f64, m)]
             + [(k, i32, m) for k in ("e_cargo", "e_origin", "e_dest")])
    name_of = {f: "e_" + f for f in SHIP}  # the end ship's buffers: x .. dest are the env's own
    g = keep(w.env(n, seed=QS.SEED))
    a = F.guard_env(g, extra)
    a.fill_out(*F.BIND_ORDER)
    load_state(g, ships_state(ships))
    gpol = keep(QPolicy(g, net.model()))
    tenv, tpol = make_policy(w, ships, net)
    src = (np.arange(m) * 3 % n).astype(i32)
    src[3::9] = n
    ids = np.random.default_rng(m).integers(0, 50, m)
    a.set("src", src)
    a.set("ids", ids)
    wanted = {k: (j % 2 == half) for j, k in enumerate(OPTIONAL)}
    ptr = lambda k: a.ptr(name_of.get(k, k)) if wanted[k] else None  # noqa: E731
    out = N.SeQnetOut(ptr("act"), ld, ptr("explored"), N.SePlanOut(*[ptr(k) for k in ("raised", "first_err", "first_err_at") + SHIP]))
    a.snapshot()
    N.check(lib().se_rollout_qnet(gpol._h, 0, eps, a.cptr("src"), m, a.cptr("ids"), 7, steps, a.cptr("ret"), a.cptr("counted"),
                                  a.cptr("status"), C.byref(out), g._stream()))
    image = a.host()
    what = f"m={m} half={half}"
    a.assert_clean(image=image, what=f"{what}: guards")
    a.assert_clean(unchanged=("src", "ids") + tuple(F.BIND_ORDER), image=image, what=f"{what}: inputs and state")
    tw = tpol.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=7, return_end=True, return_actions=True)
    u8 = np.uint8
    for k in ("ret", "counted", "status"):
        np.testing.assert_array_equal(a.get(k, image).view(u8), getattr(tw, k).cpu().numpy().view(u8), err_msg=f"{what}: {k}")
    for k in OPTIONAL:
        buf = name_of.get(k, k)
        if not wanted[k]:
            assert a.unwritten(buf, image).all(), f"{what}: {k} was not asked for and was written"
        elif k == "act":
            np.testing.assert_array_equal(a.get(buf, image)[:, :m], tw.act.cpu().numpy(), err_msg=f"{what}: act")
            assert a.unwritten(buf, image)[:, m:].all(), f"{what}: act: the columns behind a row were written"
        else:
            np.testing.assert_array_equal(a.get(buf, image).view(u8), getattr(tw, k).cpu().numpy().view(u8), err_msg=f"{what}: {k}")
    if m >= 33:
        assert (a.get("status", image) == QS.BAD_SRC).any() and len(set(a.get("status", image).tolist())) >= 3


def test_refusals_write_nothing_and_m_0_is_a_no_op():
    """Every SE_EINVAL of the header, a handle without weights and a handle whose ports changed
    (SE_ESTATE): a status, and no output entry written."""
    from shippingenv_amd import _native as N
    from shippingenv_amd._native import _ptr

    env, pol = world_policy("hand", "integer")
    w = QS.WORLDS["hand"][0]
    m, steps, ld = 8, 3, 8
    ret = torch.full((m,), float(POISON), dtype=torch.float64, device=env.device)
    cnt, status, expl, first = (torch.full((m,), POISON, dtype=torch.int32, device=env.device) for _ in range(4))
    src = torch.zeros(m, dtype=torch.int32, device=env.device)
    rows = torch.full((steps, ld), POISON, dtype=torch.int32, device=env.device)
    outs = [ret, cnt, status, expl, first, rows]
    nan = float("nan")

    def call(h=pol._h, mode=0, eps=0.3, src=src, m=m, base=0, steps=steps, ret=ret, cnt=cnt, status=status, act=rows, ld=ld,
             off=0, out=True):
        p = None if act is None else act.data_ptr() + off
        o = N.SeQnetOut(p, ld, expl.data_ptr(), N.SePlanOut(None, first.data_ptr(), *[None] * 7))
        rc = lib().se_rollout_qnet(h, mode, eps, _ptr(src), m, None, base, steps, _ptr(ret), _ptr(cnt), _ptr(status),
                                   C.byref(o) if out else None, env._stream())
        return rc, lib().se_last_error().decode()

    for kw, word in (
        (dict(m=-1), ">= 0"), (dict(steps=-1), ">= 0"), (dict(base=-1), ">= 0"),
        (dict(eps=nan), "epsilon"), (dict(eps=-0.25), "epsilon"), (dict(eps=-float("inf")), "epsilon"),
        (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(mode=1), "not built"),
        (dict(ld=m - 1), "ld"), (dict(ld=9), "aligned"), (dict(off=4), "aligned"),
        (dict(src=None), "null"), (dict(ret=None), "null"), (dict(cnt=None), "null"), (dict(status=None), "null"),
        (dict(h=None), "null qnet"),
    ):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # SE_ESTATE: a handle whose weights were never set
    fresh = C.c_void_p()
    N.check(lib().se_qnet_create(C.byref(fresh), env._h))
    rc, msg = call(h=fresh)
    assert rc == -3 and "se_qnet_set_weights" in msg
    N.check(lib().se_qnet_destroy(fresh))
    torch.cuda.synchronize()
    assert all((t == POISON).all() for t in outs), "a refused call wrote something"
    assert call(m=0, src=None, ret=None, cnt=None, status=None)[0] == 0  # m = 0: a no-op, whatever the pointers
    torch.cuda.synchronize()
    assert all((t == POISON).all() for t in outs), "m = 0 wrote something"
    assert call(act=None, ld=0)[0] == 0 and call(out=False)[0] == 0 and call(ld=9, steps=1)[0] == 0
    torch.cuda.synchronize()
    assert (expl != POISON).all() and (ret != POISON).all() and (rows[0] != POISON).all()  # these did run
    for t in outs:
        t.fill_(POISON)
    env.set_ports(w.ports, w.fuel_stock, w.cargo_stock)
    rc, msg = call()
    assert rc == -3 and "ports changed" in msg
    torch.cuda.synchronize()
    assert all((t == POISON).all() for t in outs), "a refused call wrote something"
    pol.set_weights()  # packed again for the new world version: the call runs
    assert call()[0] == 0


# ----------------------------------------------------------------- 4. the grid, new weights, a captured call
def test_one_tile_more_than_a_pass_of_the_launch():
    """One workgroup of 12 waves per compute unit, a tile of 32 rollouts per wave: with
    32 * 12 * CUs + 32 rollouts the first wave runs a second tile. Sources and ids repeat with period
    256, so the result is the 256 restated rollouts tiled; a bad source on each side of the wrap."""
    w = QS.WORLDS["hand"][0]
    ships = QS.ships_for(w)
    net = QS.IntNet.integer(w.P)
    env, pol = make_policy(w, ships, net)
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    one_pass = 32 * 12 * cus
    m, steps, eps, base = one_pass + 32, 2, 0.3, (1 << 32) - 128
    src256 = (np.arange(256) * 61 % env.n).astype(np.int32)
    want256 = QS.expected(QS.rollouts(QS.Player(O, w.oracle(O), net), ships, src256, steps, eps, base + np.arange(256)), steps)
    reps = -(-m // 256)
    src = np.tile(src256, reps)[:m].copy()
    bad = [one_pass - 1, one_pass + 5]
    src[bad] = [env.n, -1]
    ids = torch.as_tensor(base + np.arange(m) % 256, dtype=torch.int64)
    got = numpy_result(pol.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=12345, return_end=True, return_actions=True))
    want = {f: np.tile(v, reps)[..., :m].copy() for f, v in want256.items()}
    blank = QS.expected([QS.BAD], steps)
    for f in FIELDS + ("act",):
        want[f][..., bad] = blank[f][..., :1]
    assert_equal(got, want, "grid stride", FIELDS + ("act",))


def test_the_rollout_reads_the_weights_of_the_last_repack():
    """The zero network: change b3 in place, and the rollout plays the old priorities until
    repack(), then the new ones, as the restatement says for each."""
    w, m, steps = QS.WORLDS["hand"]
    ships = QS.ships_for(w)
    old, new = QS.IntNet.zero(w.P, seed=3), QS.IntNet.zero(w.P, seed=4)
    env, pol = make_policy(w, ships, old)
    src = QS.world_src("hand")
    ids = QS.BASE + np.arange(m)
    want = {k: QS.expected(QS.rollouts(QS.Player(O, w.oracle(O), net), ships, src, steps, 0.0, ids), steps)
            for k, net in (("old", old), ("new", new))}
    assert (want["old"]["act"] != want["new"]["act"]).any()
    run = lambda: numpy_result(pol.rollout(src, steps=steps, rollout_base=QS.BASE, return_end=True, return_actions=True))  # noqa: E731
    assert_equal(run(), want["old"], "before", FIELDS + ("act",))
    with torch.no_grad():
        pol.model.fc3.bias.copy_(torch.from_numpy(new.b3.astype(np.float32)))
    assert_equal(run(), want["old"], "changed, not repacked", FIELDS + ("act",))
    pol.repack()
    assert_equal(run(), want["new"], "repacked", FIELDS + ("act",))


def test_captured_call_replays_to_the_eager_result():
    """One launch on the current stream and nothing else, so torch.cuda.graph captures it; the
    replay equals the eager call and leaves the env and the policy alone."""
    env, pol = world_policy("hand", "integer")
    before, pb = snapshot(env), policy_bytes(pol)
    m = 131
    src = torch.as_tensor(np.random.default_rng(9).integers(0, env.n, m).astype(np.int32), device=env.device)
    ids = torch.arange(m, dtype=torch.int64, device=env.device) + (1 << 36)
    kw = dict(steps=12, epsilon=0.3, ids=ids, return_end=True, return_actions=True)
    eager = numpy_result(pol.rollout(src, **kw))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = pol.rollout(src, **kw)
    for f in FIELDS + ("act",):  # capture launched nothing: the replay has to write
        getattr(res, f).fill_(POISON)
    with torch.cuda.stream(side):
        g.replay()
    torch.cuda.synchronize()
    assert_equal(numpy_result(res), eager, "replay", FIELDS + ("act",))
    assert_untouched(env, before, "capture")
    assert_policy_untouched(pol, pb, "capture")


# ----------------------------------------------------------------- 5. the agent
def test_evaluate_is_the_per_origin_mean_and_touches_nothing():
    """VecDQNAgent.evaluate() equals the means of rollout()'s ret grouped by the envs' origin,
    computed on the host, envs without an origin left out; the auto-reset envs, t, epsilon, the
    ring and the weights are as they were, mid-training."""
    from shippingenv_amd.dqn import VecDQNAgent
    from shippingenv_amd.vec import VecEnv

    env = keep(VecEnv(200, seed=3, auto_reset=True))
    env.reset()
    agent = keep(VecDQNAgent(env, graph=False, batch_size=64, epsilon=0.5, memory_size=2000, max_steps=10))
    agent.train(6)
    env.origin[::7] = 255  # no origin: left out
    before, pb = snapshot(env), policy_bytes(agent.policy)
    t, eps, size, updates = agent.t, agent.epsilon, int(agent.memory.size), agent.updates
    got = agent.evaluate(steps=12, rollout_base=1 << 33)
    res = agent.rollout(steps=12, epsilon=0.0, rollout_base=1 << 33)
    ret = res.ret.cpu().numpy()
    origin = env.origin.cpu().numpy()
    want = {p: ret[origin == p].sum() / (origin == p).sum() for p in range(env.P) if (origin == p).any()}
    assert set(got) == set(want) and len(got) == env.P
    for p in want:  # the device sums in another order: n additions of relative error 2^-53 each
        assert abs(got[p] - want[p]) <= env.n * 2.0**-52 * np.abs(ret[origin == p]).sum() / (origin == p).sum(), p
    assert agent.evaluate(steps=12, ids=np.arange(env.n) % 5) != got
    assert (agent.t, agent.epsilon, int(agent.memory.size), agent.updates) == (t, eps, size, updates)
    assert_untouched(env, before, "evaluate")
    assert_policy_untouched(agent.policy, pb, "evaluate")
    assert (res.status.cpu().numpy() != QS.BAD_SRC).all() and res.act is None and res.x is None
    agent.train(2)  # and training goes on
    assert agent.t == t + 2
