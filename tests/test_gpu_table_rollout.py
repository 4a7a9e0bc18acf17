"""se_rollout_sarsa, VecSARSAAgent.rollout and .evaluate on the GPU, bit for bit (ret and fuel as
uint64).

The kernel is held to the plain-Python restatement of tests/table_rollout_support.py, which
tests/test_table_rollout_cpu.py pins to oracle.rollout (epsilon = 1) and to plan_support's scripted
rollout, and whose hand cases it shows to cover every branch of the position; then to the
equalities of include/shipenv.h against the library's own calls: se_rollout (E1), se_rollout_plan
fed the emitted rows (E2), se_sarsa_choose (E3), the sparse kind against the dense (E4), and a table
distilled from the navigator against se_rollout_nav. Then what the call must leave alone, its
footprint in a guarded arena, its refusals, the grid-stride loop, a captured call, evaluate()."""
import ctypes as C

import numpy as np
import pytest

import footprint_support as F
import nav_support as NS
import plan_support as PS
import rollout_support as RS
import sarsa_support as SS
import table_rollout_support as TS
from test_gpu_rollout import load_state, oracle_state
from test_gpu_rollout_plan import GRID_THREADS, assert_untouched, snapshot
from test_gpu_sarsa import ships_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

SEED, NONE, POISON = TS.SEED, TS.NONE, -7
FIELDS, ACTS, SHIP = TS.FIELDS, TS.ACTS, TS.SHIP
LEARNER = ("type", "a", "b", "fresh", "ep_len", "ep_return")
E1_STATUS = {RS.DONE: TS.DONE, RS.MAX_STEPS: TS.END, RS.ATTEMPTS: TS.END, RS.RAISED: TS.STUCK}  # se_rollout's -> ours
CONFIGS = [("zero", False), ("zero", True), ("normal", False), ("hand", False), ("hand", True)]


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


def make_env(world, ships, seed=SEED):
    env = keep(world.env(len(ships), seed=seed))
    load_state(env, ships_state(ships))
    return env


def make_agent(env, dense=None, image=None, **kw):
    """A dense agent holding the flat array `dense`, or a sparse one of the image's capacity."""
    from shippingenv_amd.sarsa import VecSARSAAgent

    if image is None:
        ag = keep(VecSARSAAgent(env, **kw))
        if dense is not None:
            ag.q.copy_(torch.from_numpy(np.asarray(dense).reshape(ag.rows, ag.A)))
        return ag
    keys, pages = image
    ag = keep(VecSARSAAgent(env, table="sparse", capacity=len(keys), **kw))
    ag.keys.copy_(torch.from_numpy(np.asarray(keys)))
    ag.pages.copy_(torch.from_numpy(np.asarray(pages).reshape(len(keys), ag.A)))
    ag._bind()
    return ag


def hand_agent(table, sparse):
    dense, image = TS.hand_table(O, table)
    env = make_env(TS.HAND, TS.HAND_SHIPS)
    return env, make_agent(env, dense, image if sparse else None)


def numpy_result(res, acts=False):
    out = {f: getattr(res, f).cpu().numpy() for f in FIELDS + (ACTS if acts else ())}
    assert out["ret"].dtype == np.float64 and out["fuel"].dtype == np.float64
    assert all(v.dtype == np.int32 for f, v in out.items() if f not in ("ret", "fuel"))
    return out


def assert_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        if f in ("ret", "fuel"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {f}")


def table_bytes(ag):
    ts = (ag.keys, ag.pages) if ag.table == "sparse" else (ag.q,)
    return [t.cpu().numpy().copy().view(np.uint8) for t in ts + tuple(getattr(ag, f) for f in LEARNER)], ag.stats(), ag.t


def assert_table_untouched(ag, before, what=""):
    after = table_bytes(ag)
    assert after[1:] == before[1:], f"{what}: stats or t"
    for a, b in zip(after[0], before[0]):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: the table or the learner state changed")


# ----------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("eps", TS.EPSILONS)
@pytest.mark.parametrize("table,sparse", CONFIGS)
def test_kernel_equals_the_restatement(table, sparse, eps):
    """The seven hand-placed ships from every lane residue of two waves + 3 at 21 positions; 0, 1
    and 2 positions on 67 rollouts: every output, the action rows included."""
    env, ag = hand_agent(table, sparse)
    before, tb = snapshot(env), table_bytes(ag)
    statuses = set()
    for steps, m in ((21, TS.M), (0, 67), (1, 67), (2, 67)):
        rolls, _ = TS.suite(O, table, eps, steps=steps, sparse=sparse, m=m)
        res = ag.rollout(TS.hand_src(m), steps=steps, epsilon=eps, rollout_base=TS.BASE, return_end=True, return_actions=True)
        assert res.act_type.shape == (steps, m)
        got = numpy_result(res, acts=True)
        assert_equal(got, TS.expected(rolls, steps), f"{table} sparse={sparse} eps={eps} steps={steps}", FIELDS + ACTS)
        if steps == 0:
            assert (got["ret"] == 0).all() and (got["counted"] == 0).all() and (got["status"] == TS.END).all()
        statuses |= set(got["status"].tolist())
        if eps == 1.0:  # E1: se_rollout of the same base with max_steps = max_attempts = steps
            ret, cnt, status = (t.cpu().numpy() for t in env.rollout(TS.hand_src(m), max_steps=steps, max_attempts=steps,
                                                                     rollout_base=TS.BASE))
            np.testing.assert_array_equal(got["ret"].view(np.uint64), ret.view(np.uint64), err_msg="E1 ret")
            np.testing.assert_array_equal(got["counted"], cnt, err_msg="E1 counted")
            np.testing.assert_array_equal(got["status"], [E1_STATUS[s] if steps else TS.END for s in status.tolist()], err_msg="E1 status")
    assert {TS.DONE, TS.END} <= statuses and (TS.STUCK in statuses or (table, eps) == ("normal", 0.0))
    assert_untouched(env, before, "rollout")
    assert_table_untouched(ag, tb, "rollout")


SCENARIOS = {"one": RS.ONE, "shared": RS.SHARED, "open": RS.OPEN}


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_worlds_under_a_random_table(name, eps):
    """P = 1, two ports on one cell, a port without cargo: rollout_support's actors under seeded
    normals over every row, dense, and E1 against se_rollout itself at epsilon 1."""
    world = SCENARIOS[name]
    ow = world.oracle(O)
    ships = [PS.ship_of(RS.table(O, name), i) for i in range(len(RS.actors(name)))]
    lay = SS.Layout(ow)
    dense = np.random.default_rng(len(name)).standard_normal(lay.rows * lay.A)
    env = make_env(world, ships)
    ag = make_agent(env, dense)
    m, steps = TS.M, 21
    src = (np.arange(m) % len(ships)).astype(np.int32)
    rolls = TS.rollouts(O, ow, ships, src, steps, eps, TS.Policy(ow, dense=dense), TS.BASE + np.arange(m))
    got = numpy_result(ag.rollout(src, steps=steps, epsilon=eps, rollout_base=TS.BASE, return_end=True, return_actions=True), True)
    assert_equal(got, TS.expected(rolls, steps), f"{name} eps={eps}", FIELDS + ACTS)
    # E1: epsilon 1 is se_rollout of the same base with max_steps = max_attempts = steps
    one = numpy_result(ag.rollout(src, steps=steps, epsilon=1.0, rollout_base=TS.BASE, return_end=True))
    ret, cnt, status = (t.cpu().numpy() for t in env.rollout(src, max_steps=steps, max_attempts=steps, rollout_base=TS.BASE))
    np.testing.assert_array_equal(one["ret"].view(np.uint64), ret.view(np.uint64))
    np.testing.assert_array_equal(one["counted"], cnt)
    np.testing.assert_array_equal(one["status"], [E1_STATUS[s] for s in status.tolist()])
    assert len(set(status.tolist())) >= 2


def test_largest_world_takes_the_large_lds_path_with_a_sparse_table():
    """256 x 256 cells and 254 ports: the world image is past 64 KiB and the dense table would have
    3 * 10^10 rows. 65 rollouts of 12 positions from envs after a reset and 40 random steps, under a
    sparse table of capacity 64 that holds normals on the rows the envs stand in."""
    w = RS.max_world()
    ow = w.oracle(O)
    n, m, steps = 33, 65, 12
    env = keep(w.env(n, seed=31))
    env.reset()
    for t in range(40):
        env.step(env.gen_actions(t))
    st = oracle_state(env)
    ships = [PS.ship_of(st, i) for i in range(n)]
    from shippingenv_amd.sarsa import sparse_image

    lay = SS.Layout(ow)
    blank = TS.Policy(ow)
    rows = sorted({blank.row_of(SS.discretize(sh)) for sh in ships[::2]})
    image = sparse_image(rows, np.random.default_rng(3).standard_normal((len(rows), lay.A)), 64)
    ag = make_agent(env, image=image)
    assert (ag.rows, ag.A) == (lay.rows, lay.A) and ag.rows > 1 << 34
    before = snapshot(env)
    src = np.random.default_rng(65).integers(0, n, m).astype(np.int32)
    src[17] = n
    for eps in (0.0, 0.3):
        pol = TS.Policy(ow, keys=image[0], pages=image[1])
        rolls = TS.rollouts(O, ow, ships, src, steps, eps, pol, 9 + np.arange(m), seed=31)
        got = numpy_result(ag.rollout(src, steps=steps, epsilon=eps, rollout_base=9, return_end=True, return_actions=True), True)
        assert_equal(got, TS.expected(rolls, steps), f"max world eps={eps}", FIELDS + ACTS)
        assert pol.seen["absent"] > 0 and got["counted"].sum() > m and got["status"][17] == TS.BAD_SRC
    assert_untouched(env, before, "max world")


# ----------------------------------------------------------------- 2. the equalities
@pytest.mark.parametrize("eps", TS.EPSILONS)
@pytest.mark.parametrize("table,sparse", [("zero", False), ("normal", False), ("hand", True)])
def test_equals_the_plan_of_the_emitted_rows(table, sparse, eps):
    """E2: se_rollout_plan (typed) fed the rows the call wrote, as they lie, under the same ids;
    type 0 pads behind the end. A stuck rollout is compared up to stuck_at."""
    env, ag = hand_agent(table, sparse)
    m, steps = TS.M, 21
    src = TS.hand_src(m)
    ids = np.random.default_rng(2).choice([5, 6, (1 << 40) + 3, (1 << 63) - 1, 0], m).astype(np.int64)
    res = ag.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=999, return_end=True, return_actions=True)
    got = numpy_result(res, acts=True)
    stuck = got["status"] == TS.STUCK
    lens = np.where(stuck, got["stuck_at"], steps).astype(np.int32)
    plan = env.rollout_plan(src, res.act_type, res.act_a, res.act_b, lengths=lens, ids=ids, return_end=True)
    want = {f: getattr(plan, f).cpu().numpy() for f in ("ret", "steps", "status", "raised", "first_err", "first_err_at") + SHIP}
    want["counted"] = want["steps"]
    assert_equal(got, want, f"E2 {table} eps={eps}", ("ret", "counted", "raised", "first_err", "first_err_at") + SHIP)
    np.testing.assert_array_equal(got["status"][~stuck], want["status"][~stuck])
    assert (want["status"][stuck] == TS.END).all() and (~stuck).any()
    # the ship in the port without cargo has no row in "zero" and "hand": its SELECT 0 raises and the sample after it too
    assert stuck.any() or table == "normal"
    played = got["counted"] + got["raised"]
    for r in range(m):  # type 0 behind the end, an action at every position played
        assert (got["act_type"][:played[r], r] > 0).all() and not got["act_type"][played[r]:, r].any()
        assert not got["act_a"][played[r]:, r].any() and not got["act_b"][played[r]:, r].any()


@pytest.mark.parametrize("table,sparse", CONFIGS)
def test_first_action_is_se_sarsa_choose(table, sparse):
    """E3: position 0 at epsilon 0 on every env is se_sarsa_choose(epsilon = 0)'s action there; where
    that falls to a sample_action, the two read different words, so only the type is compared."""
    env, ag = hand_agent(table, sparse)
    res = ag.rollout(steps=1, epsilon=0.0, return_actions=True)
    first = np.stack([getattr(res, f).cpu().numpy()[0] for f in ACTS], 1)
    chosen = np.stack([t.cpu().numpy() for t in ag.choose_action(epsilon=0.0)], 1)
    sampled = np.zeros(env.n, bool)
    if table == "hand":
        sampled[TS.DRY] = True  # the NaN / -inf row
    np.testing.assert_array_equal(first[~sampled], chosen[~sampled])
    assert (first[sampled, 0] == chosen[sampled, 0]).all() and (res.stuck_at.cpu().numpy() == -1).all()


@pytest.mark.parametrize("eps", TS.EPSILONS)
@pytest.mark.parametrize("table", ["zero", "hand"])
def test_sparse_equals_dense_byte_for_byte(table, eps):
    """E4: the two kinds holding the same map, every output as bytes."""
    outs = []
    for sparse in (False, True):
        env, ag = hand_agent(table, sparse)
        res = ag.rollout(TS.hand_src(), steps=21, epsilon=eps, rollout_base=TS.BASE, return_end=True, return_actions=True)
        outs.append({f: getattr(res, f).cpu().numpy().copy().view(np.uint8) for f in FIELDS + ACTS})
    for f in FIELDS + ACTS:
        np.testing.assert_array_equal(outs[0][f], outs[1][f], err_msg=f)


# ----------------------------------------------------------------- 3. ids
def test_ids_are_the_streams():
    """Duplicate ids give identical rollouts for identical sources, whatever the lane; 64-bit ids
    against the restatement; ids = base + r is rollout_base; sub-batches; src=None; an empty batch."""
    env, ag = hand_agent("normal", False)
    dense, _ = TS.hand_table(O, "normal")
    ow = TS.HAND.oracle(O)
    m, steps, eps = 197, 21, 0.3
    rng = np.random.default_rng(11)
    src = rng.integers(0, env.n, m).astype(np.int32)
    bad = {0: -1, m - 1: env.n, 70: env.n + 7, 131: -(1 << 31), 64: (1 << 31) - 1}
    for k, v in bad.items():
        src[k] = v
    ids = rng.choice([5, 6, (1 << 40) + 3, (1 << 63) - 1, 0], m).astype(np.int64)
    rolls = TS.rollouts(O, ow, TS.HAND_SHIPS, src, steps, eps, TS.Policy(ow, dense=dense), ids)
    got = numpy_result(ag.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=999, return_end=True, return_actions=True), True)
    assert_equal(got, TS.expected(rolls, steps), "ids", FIELDS + ACTS)
    where = np.array(sorted(bad))
    assert (got["status"][where] == TS.BAD_SRC).all() and (got["status"] == TS.BAD_SRC).sum() == len(where)
    same = numpy_result(ag.rollout(np.full(m, TS.LOADED, np.int32), steps=steps, epsilon=eps, ids=np.full(m, (1 << 40) + 3),
                                   return_end=True, return_actions=True), True)
    for f in FIELDS:
        assert (same[f] == same[f][0]).all(), f
    assert (same["act_type"] == same["act_type"][:, :1]).all() and same["counted"][0] > 0
    good = np.where(src < 0, 0, np.minimum(src, env.n - 1)).astype(np.int32)
    base = (1 << 32) - 100
    whole = numpy_result(ag.rollout(good, steps=steps, epsilon=eps, rollout_base=base, return_end=True))
    for lo, hi in ((0, 64), (130, 197), (m - 1, m)):
        part = numpy_result(ag.rollout(good[lo:hi], steps=steps, epsilon=eps, rollout_base=base + lo, return_end=True))
        assert_equal(part, {f: v[lo:hi] for f, v in whole.items()}, f"sub-batch [{lo}, {hi})")
    by_ids = numpy_result(ag.rollout(good, steps=steps, epsilon=eps, ids=base + np.arange(m), rollout_base=3, return_end=True))
    assert_equal(by_ids, whole, "ids = base + arange")
    every = ag.rollout(steps=2, return_end=True)
    assert every.ret.numel() == env.n and every.act_type is None
    none = ag.rollout(np.zeros(0, np.int32), steps=5, return_end=True, return_actions=True)
    assert all(getattr(none, f).numel() == 0 for f in FIELDS + ACTS) and ag.rollout(np.zeros(0, np.int32)).x is None


# ----------------------------------------------------------------- 4. the navigator, distilled
# worlds with a detour (a wall with its gap in the last row; a ground cell in open water), every port
# reachable from every cell a ship can stand on: at sea, in port with and without a destination
# (with and without an origin), cargo aboard, on the destination's cell, a ship that runs dry
DETOUR_SHIPS = {
    "wall": [(2, 3, 100.0, 20, 0, 1), (2, 5, 100.0, 0, 1, 0), (2, 1, 30.0, 0, NONE, NONE), (4, 4, 50.0, 0, 0, 1),
             (2, 1, 100.0, 0, 0, 1), (2, 7, 12.0, 3, 1, NONE), (4, 4, 3.5, 0, 1, 0)],
    "open": [(3, 3, 100.0, 0, 0, 1), (1, 1, 200.0, 0, NONE, NONE), (1, 1, 200.0, 0, 3, NONE), (3, 4, 100.0, 30, 0, 1),
             (3, 4, 1.5, 0, 0, 1), (5, 6, 200.0, 3, 0, 1), (2, 4, 100.0, 60, 0, 2)],
}


@pytest.mark.parametrize("name", list(DETOUR_SHIPS))
def test_a_distilled_table_equals_the_navigator(name):
    """The navigator written into a table (1.0 in the move slot dir[dest][cell] names for every
    fuel class and origin, 1.0 in the SELECT slot rule 1 picks in port rows without a destination)
    plays what se_rollout_nav(refuel_below = 0, load = 0) plays under the same ids: common random
    numbers make ret (bits), counted and the end ship equal for every one of the rollouts, all
    from reachable ships, none stuck in either."""
    from shippingenv_amd.nav import VecNavigator

    world, ships = NS.SMALL[name], DETOUR_SHIPS[name]
    env = make_env(world, ships)
    nav = keep(VecNavigator(env, refuel_below=0.0, load=0))
    lay = SS.Layout(world.oracle(O))
    ag = make_agent(env, TS.distilled(lay, world, nav.directions(), nav.fields()))
    m, steps = TS.M, 21
    src = (np.arange(m) % len(ships)).astype(np.int32)
    ids = (1 << 35) + 3 * np.arange(m)
    got = numpy_result(ag.rollout(src, steps=steps, epsilon=0.0, ids=ids, rollout_base=5, return_end=True))
    want = nav.rollout(src, steps=steps, ids=ids, rollout_base=77, return_end=True)
    wn = {f: getattr(want, f).cpu().numpy() for f in ("ret", "steps", "status", "raised") + SHIP}
    both = (got["status"] != TS.STUCK) & (wn["status"] != TS.STUCK)
    assert both.sum() == m, "a hand-placed ship is stuck under one of the two policies"
    wn["counted"] = wn["steps"]
    assert_equal(got, wn, name, ("ret", "counted", "status", "raised") + SHIP)
    assert (got["raised"] == 0).all() and {TS.DONE, TS.END} <= set(got["status"].tolist())
    assert (got["counted"] == steps).any() and len(np.unique(got["ret"])) > len(ships)


# ----------------------------------------------------------------- 5. what the call leaves alone
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_nothing_is_modified(kind):
    """After some learning steps (pending actions, running episodes, a table with content): the env
    state, the counters, q or keys and pages, the learner state, stats() and t, byte for byte."""
    from shippingenv_amd.sarsa import VecSARSAAgent

    env = keep(TS.HAND.env(130, seed=SEED))
    env.reset()
    ag = keep(VecSARSAAgent(env, table=kind, epsilon=0.5, max_steps=30))
    ag.train(12, sync_every=4)
    before, tb = snapshot(env), table_bytes(ag)
    assert tb[0][0].any() and tb[2] == 12
    for eps in TS.EPSILONS:
        res = ag.rollout(steps=21, epsilon=eps, return_end=True, return_actions=True)
        assert (res.counted.cpu().numpy() > 0).any()
        ag.evaluate(steps=5)
    assert_untouched(env, before, kind)
    assert_table_untouched(ag, tb, kind)


i32, f64, i64, u8 = np.int32, np.float64, np.int64, np.uint8
OPTIONAL = ("stuck_at", "sample_type", "acts", "raised", "first_err", "first_err_at") + SHIP


@pytest.mark.parametrize("half", [0, 1], ids=["even-outputs", "odd-outputs"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 131])
def test_footprint_in_a_guarded_arena(m, half):
    """Every buffer of the call a view into one arena at its documented size between patterned
    guards: src and ids m entries, ret, counted and status m, each optional output m, the action rows
    [steps][ld] with ld = m rounded up to 4, the table and the learner state. The optional outputs
    alternate between wanted and NULL (`half` swaps them; the three rows go together): the guards,
    the inputs, the env, the table and the learner state hold, the outputs that were not asked for
    and the ld - m columns behind each row keep their prefill, the others are the twin's."""
    from shippingenv_amd import _native as N

    steps, eps, ld = 6, 0.3, (m + 3) // 4 * 4
    dense, _ = TS.hand_table(O, "normal")
    lay = SS.Layout(TS.HAND.oracle(O))
    n = len(TS.HAND_SHIPS)
    extra = ([("src", i32, m), ("ids", i64, m), ("ret", f64, m), ("counted", i32, m), ("status", i32, m),
              ("stuck_at", i32, m), ("sample_type", i32, m)] + [(k, i32, (steps, ld)) for k in ACTS]
             + [(k, i32, m) for k in ("raised", "first_err", "first_err_at", "e_x", "e_y")] + [("e_fuel", f64, m)]
             + [(k, i32, m) for k in ("e_cargo", "e_origin", "e_dest")]
             + [("q", f64, (lay.rows, lay.A)), ("type", i32, n), ("a", i32, n), ("b", i32, n), ("fresh", u8, n),
                ("ep_len", i32, n), ("sarsa_return", f64, n)])
    name_of = {f: "e_" + f for f in SHIP}  # the end ship's buffers: x .. dest are the env's own
    g = keep(TS.HAND.env(n, seed=SEED))
    a = F.guard_env(g, extra)
    a.fill_out(*F.BIND_ORDER)
    load_state(g, ships_state(TS.HAND_SHIPS))
    tenv, tag = hand_agent("normal", False)
    ag = make_agent(g)
    learner = ("type", "a", "b", "fresh", "ep_len", "sarsa_return")
    a.set("q", dense.reshape(lay.rows, lay.A))
    for k, v in zip(learner, (2, 1, 0, 0, 3, 1.5)):
        a.set(k, np.full(n, v))
    N.check(lib().se_sarsa_bind(ag._h, a.cptr("q"), C.byref(N.SeSarsaState(*[a.ptr(k) for k in learner]))))
    src = (np.arange(m) * 3 % n).astype(i32)
    src[3::9] = n
    ids = np.random.default_rng(m).integers(0, 50, m)
    a.set("src", src)
    a.set("ids", ids)
    wanted = {k: (j % 2 == half) for j, k in enumerate(OPTIONAL)}
    ptr = lambda k: a.ptr(name_of.get(k, k)) if wanted[k] else None  # noqa: E731
    acts = [a.ptr(k) if wanted["acts"] else None for k in ACTS]
    out = N.SeTableOut(ptr("stuck_at"), ptr("sample_type"), *acts, ld,
                       N.SePlanOut(*[ptr(k) for k in ("raised", "first_err", "first_err_at") + SHIP]))
    a.snapshot()
    N.check(lib().se_rollout_sarsa(ag._h, eps, a.cptr("src"), m, a.cptr("ids"), 7, steps, a.cptr("ret"), a.cptr("counted"),
                                   a.cptr("status"), C.byref(out), g._stream()))
    image = a.host()
    what = f"m={m} half={half}"
    a.assert_clean(image=image, what=f"{what}: guards")
    a.assert_clean(unchanged=("src", "ids", "q") + learner + tuple(F.BIND_ORDER), image=image, what=f"{what}: inputs and state")
    tw = tag.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=7, return_end=True, return_actions=True)
    for k in ("ret", "counted", "status"):
        np.testing.assert_array_equal(a.get(k, image).view(u8), getattr(tw, k).cpu().numpy().view(u8), err_msg=f"{what}: {k}")
    for k in OPTIONAL:
        for f in (ACTS if k == "acts" else (k,)):
            buf = name_of.get(f, f)
            if not wanted[k]:
                assert a.unwritten(buf, image).all(), f"{what}: {f} was not asked for and was written"
            elif k == "acts":
                np.testing.assert_array_equal(a.get(buf, image)[:, :m], getattr(tw, f).cpu().numpy(), err_msg=f"{what}: {f}")
                assert a.unwritten(buf, image)[:, m:].all(), f"{what}: {f}: the columns behind a row were written"
            else:
                np.testing.assert_array_equal(a.get(buf, image).view(u8), getattr(tw, f).cpu().numpy().view(u8), err_msg=f"{what}: {f}")
    if m >= 63:
        assert (a.get("status", image) == TS.BAD_SRC).any() and len(set(a.get("status", image).tolist())) >= 3


def test_refusals_write_nothing_and_m_0_is_a_no_op():
    """Every SE_EINVAL of the header, an unbound handle and a handle whose ports changed
    (SE_ESTATE): a status, and no output entry written."""
    from shippingenv_amd import _native as N
    from shippingenv_amd._native import _ptr

    env, ag = hand_agent("normal", False)
    m, steps, ld = 8, 3, 8
    ret = torch.full((m,), float(POISON), dtype=torch.float64, device=env.device)
    cnt, status, stuck, first = (torch.full((m,), POISON, dtype=torch.int32, device=env.device) for _ in range(4))
    src = torch.zeros(m, dtype=torch.int32, device=env.device)
    rows = [torch.full((steps, ld), POISON, dtype=torch.int32, device=env.device) for _ in range(3)]
    nan = float("nan")

    def call(h=ag._h, eps=0.3, src=src, m=m, base=0, steps=steps, ret=ret, cnt=cnt, status=status, acts=rows, ld=ld, off=0,
             out=True):
        ptrs = [None if t is None else C.c_void_p(t.data_ptr() + off) for t in acts]
        o = N.SeTableOut(stuck.data_ptr(), None, *ptrs, ld, N.SePlanOut(None, first.data_ptr(), *[None] * 7))
        rc = lib().se_rollout_sarsa(h, eps, _ptr(src), m, None, base, steps, _ptr(ret), _ptr(cnt), _ptr(status),
                                    C.byref(o) if out else None, env._stream())
        return rc, lib().se_last_error().decode()

    for kw, word in (
        (dict(m=-1), ">= 0"), (dict(steps=-1), ">= 0"), (dict(base=-1), ">= 0"),
        (dict(eps=nan), "epsilon"), (dict(eps=-0.25), "epsilon"), (dict(eps=-float("inf")), "epsilon"),
        (dict(ld=m - 1), "ld"), (dict(ld=9), "aligned"), (dict(off=4), "aligned"),
        (dict(acts=[rows[0], None, rows[2]]), "all or none"), (dict(acts=[None, None, rows[2]]), "all or none"),
        (dict(acts=[rows[0], rows[1], None]), "all or none"),
        (dict(src=None), "null"), (dict(ret=None), "null"), (dict(cnt=None), "null"), (dict(status=None), "null"),
        (dict(h=None), "null sarsa handle"),
    ):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # SE_ESTATE: a handle that was never bound; the ports changed since create
    fresh = C.c_void_p()
    N.check(lib().se_sarsa_create(C.byref(fresh), env._h, 1 << 40))
    rc, msg = call(h=fresh)
    assert rc == -3 and "se_sarsa_bind" in msg
    torch.cuda.synchronize()
    assert all((t == POISON).all() for t in [ret, cnt, status, stuck, first] + rows), "a refused call wrote something"
    assert call(m=0, src=None, ret=None, cnt=None, status=None)[0] == 0  # m = 0: a no-op, whatever the pointers
    assert call(acts=[None] * 3, ld=0)[0] == 0 and call(out=False)[0] == 0 and call(ld=9, steps=1)[0] == 0
    torch.cuda.synchronize()
    assert (stuck != POISON).all() and (ret != POISON).all() and (rows[0][0] != POISON).all()  # these did run
    for t in [ret, cnt, status, stuck, first] + rows:
        t.fill_(POISON)
    env.set_ports(TS.HAND.ports, TS.HAND.fuel_stock, TS.HAND.cargo_stock)
    rc, msg = call()
    assert rc == -3 and "stale" in msg
    torch.cuda.synchronize()
    N.check(lib().se_sarsa_destroy(fresh))
    assert all((t == POISON).all() for t in [ret, cnt, status, stuck, first] + rows), "a refused call wrote something"


# ----------------------------------------------------------------- 6. the grid, a captured call
def test_more_rollouts_than_threads():
    """2048 * 256 + 257 rollouts: the first 257 lanes run a second rollout. Sources and ids repeat
    with period 256, so the result is the 256 restated rollouts tiled; a bad source on each side
    of the wrap."""
    env, ag = hand_agent("normal", False)
    dense, _ = TS.hand_table(O, "normal")
    ow = TS.HAND.oracle(O)
    m, steps, eps, base = GRID_THREADS + 257, 4, 0.3, (1 << 32) - 128
    src256 = (np.arange(256) * 61 % env.n).astype(np.int32)
    want256 = TS.expected(TS.rollouts(O, ow, TS.HAND_SHIPS, src256, steps, eps, TS.Policy(ow, dense=dense), base + np.arange(256)), steps)
    assert {TS.DONE, TS.END, TS.STUCK} <= set(want256["status"].tolist())
    reps = -(-m // 256)
    src = np.tile(src256, reps)[:m].copy()
    bad = [GRID_THREADS - 1, GRID_THREADS + 5]
    src[bad] = [env.n, -1]
    ids = torch.as_tensor(base + np.arange(m) % 256, dtype=torch.int64)
    got = numpy_result(ag.rollout(src, steps=steps, epsilon=eps, ids=ids, rollout_base=12345, return_end=True, return_actions=True), True)
    want = {f: np.tile(v, reps)[..., :m].copy() for f, v in want256.items()}
    blank = TS.expected([TS.BAD], steps)
    for f in FIELDS + ACTS:
        want[f][..., bad] = blank[f][..., :1]
    assert_equal(got, want, "grid stride", FIELDS + ACTS)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_captured_call_replays_to_the_eager_result(sparse):
    """One launch on the current stream and nothing else, so torch.cuda.graph captures it; the
    replay equals the eager call and leaves the env and the table alone."""
    env, ag = hand_agent("hand", sparse)
    before, tb = snapshot(env), table_bytes(ag)
    m = 257
    src = torch.as_tensor(np.random.default_rng(9).integers(0, env.n, m).astype(np.int32), device=env.device)
    ids = torch.arange(m, dtype=torch.int64, device=env.device) + (1 << 36)
    kw = dict(steps=21, epsilon=0.3, ids=ids, return_end=True, return_actions=True)
    eager = numpy_result(ag.rollout(src, **kw), True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = ag.rollout(src, **kw)
    for f in FIELDS + ACTS:  # capture launched nothing: the replay has to write
        getattr(res, f).fill_(POISON)
    with torch.cuda.stream(side):
        g.replay()
    torch.cuda.synchronize()
    assert_equal(numpy_result(res, True), eager, "replay", FIELDS + ACTS)
    assert_untouched(env, before, "capture")
    assert_table_untouched(ag, tb, "capture")


# ----------------------------------------------------------------- 7. evaluate, and the workload's shape
def test_evaluate_is_the_per_origin_mean_and_test_policy_is_unchanged():
    """evaluate() equals the means of rollout()'s ret grouped by the envs' origin, computed on the
    host, envs without an origin left out, and leaves the envs, the table and t alone. test_policy
    still returns what it returned: an agent that has evaluated in between answers what its twin,
    trained the same way and never evaluated, answers."""
    from shippingenv_amd.sarsa import VecSARSAAgent

    def trained():
        env = keep(TS.HAND.env(200, seed=SEED))
        env.reset()
        ag = keep(VecSARSAAgent(env, epsilon=0.5, max_steps=10))
        ag.train(16, sync_every=8)
        return env, ag

    env, ag = trained()
    env.origin[::7] = 255  # no origin: left out
    before, tb = snapshot(env), table_bytes(ag)
    got = ag.evaluate(steps=21, rollout_base=1 << 33)
    ret = ag.rollout(steps=21, epsilon=0.0, rollout_base=1 << 33).ret.cpu().numpy()
    origin = env.origin.cpu().numpy()
    want = {p: ret[origin == p].sum() / (origin == p).sum() for p in range(env.P) if (origin == p).any()}
    assert set(got) == set(want) and len(got) == env.P
    for p in want:  # the device sums in another order: n additions of relative error 2^-53 each
        assert abs(got[p] - want[p]) <= env.n * 2.0**-52 * np.abs(ret[origin == p]).sum() / (origin == p).sum(), p
    ids = np.arange(env.n) % 5
    assert ag.evaluate(steps=21, ids=ids) != got
    assert_untouched(env, before, "evaluate")
    assert_table_untouched(ag, tb, "evaluate")
    twin_env, twin = trained()
    first = ag.test_policy(25)
    ag.evaluate(steps=3)
    assert twin.test_policy(25) == first and first


def test_default_world_at_4096_envs_after_a_random_pre_roll(water):
    """n = 2^12 on the builtin map after a reset, 50 random steps and a few learning steps of a
    sparse learner: 30 positions at epsilon 0.1, two slices of 64 rollouts against the restatement
    reading the learner's own keys and pages."""
    from shippingenv_amd.sarsa import VecSARSAAgent
    from shippingenv_amd.vec import VecEnv

    n, steps, eps = 1 << 12, 30, 0.1
    env = keep(VecEnv(n, seed=0))
    np.testing.assert_array_equal(env.water, water)
    world = NS.default_world(water, seed=0)
    env.reset()
    for t in range(50):
        env.step(env.gen_actions(t))
    ag = keep(VecSARSAAgent(env, table="sparse", epsilon=0.5))
    ag.fresh.fill_(1)
    ag.train(6, sync_every=3)
    before, tb = snapshot(env), table_bytes(ag)
    got = numpy_result(ag.rollout(steps=steps, epsilon=eps, rollout_base=1 << 20, return_end=True, return_actions=True), True)
    assert_untouched(env, before, "2^12")
    assert_table_untouched(ag, tb, "2^12")
    st, ow = oracle_state(env), world.oracle(O)
    picked = np.concatenate([np.arange(lo, lo + 64) for lo in (0, n - 64)])
    pol = TS.Policy(ow, keys=ag.keys.cpu().numpy(), pages=ag.pages.cpu().numpy())
    ships = [PS.ship_of(st, i) for i in range(n)]
    rolls = TS.rollouts(O, ow, ships, picked, steps, eps, pol, (1 << 20) + picked, seed=0)
    want = TS.expected(rolls, steps)
    assert_equal({f: v[..., picked] for f, v in got.items()}, want, "2^12 slices", FIELDS + ACTS)
    kinds = {k for ro in rolls for k in ro.kinds}
    assert {"greedy", "explore", "fallback"} <= kinds and pol.seen["absent"] > 0 and ag.stats()["used"] > 0
