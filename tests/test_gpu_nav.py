"""se_nav_actions, se_rollout_nav and VecNavigator on the GPU, bit for bit (ret and fuel as uint64).

Everything is held to the plain-Python restatement of tests/nav_support.py, which
tests/test_nav_cpu.py pins to the library's host builder, the field laws and the C oracle's typed
step; and a navigated rollout is held to se_rollout_plan on the same env fed the restated action
list, the contract of include/shipenv.h. The unreachable and stuck cases are ordinary statuses:
where a dir byte is SE_NAV_NONE, a destination names no port or a ship stands outside the map, no
table index is formed from it (worlds `lake`, `dot`, `one` and the hand-placed ships below)."""
import ctypes as C

import numpy as np
import pytest

import nav_support as NS
import plan_support as PS
import rollout_support as RS
from test_gpu_rollout import load_state, oracle_state
from test_gpu_rollout_plan import GRID_THREADS, assert_untouched, rows, snapshot

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

NONE = NS.NONE
SHIP = ("x", "y", "fuel", "cargo", "origin", "dest")
FIELDS = ("ret", "steps", "status", "arrivals", "nav_status", "stuck_at", "raised", "first_err", "first_err_at") + SHIP
SEED = RS.SEED
POISON = -7


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


# a MANY-like world whose stocks straddle the amounts the agent index can name (cargo 49, fuel 199)
MANY100 = RS.World(9, 13, ports=RS.MANY.ports, fuel=[(199, 200, 250, 3)[i % 4] for i in range(64)],
                   cargo=[(49, 50, 100, 7)[i % 4] for i in range(64)])
EMPTY = RS.World(4, 5, ports=[], fuel=[], cargo=[])  # P = 0: a valid handle
WORLDS = dict(NS.SMALL, many100=MANY100, empty=EMPTY)

# name -> (refuel_below, load, hand-placed ships): every rule and every status the world can show
CASES = {
    "open": (50.0, 2, [
        (1, 1, 200.0, 0, NONE, NONE), (1, 1, 200.0, 0, 3, NONE),  # select the nearest; ... that is not the origin
        (3, 3, 200.0, 0, 0, NONE),                                  # no destination at sea
        (1, 1, 10.0, 0, 2, 1), (1, 1, 50.0, 0, 2, 1),              # refuel; fuel == refuel_below: load
        (5, 2, 200.0, 0, 0, 1), (1, 1, 200.0, 3, 2, 1),            # no cargo in stock, cargo aboard: move
        (3, 4, 100.0, 30, 0, 1), (3, 4, 1.5, 0, 0, 1),             # loaded at sea; runs dry
        (5, 6, 200.0, 3, 0, 1), (2, 5, 100.0, 0, 0, 1),            # on the destination's cell; on a ground cell
        (1, 1, 200.0, 3, 0, 4), (1, 1, 200.0, 3, 0, 254),          # a destination that names no port
        (7, 1, 100.0, 0, 0, 1), (1, 9, 100.0, 0, 0, 1), (255, 255, 100.0, 0, 0, 1),  # outside the map
    ]),
    "lake": (0.0, 3, [
        (0, 0, 100.0, 0, 0, 1), (3, 3, 100.0, 0, NONE, NONE), (3, 3, 100.0, 0, 0, 2), (2, 2, 100.0, 0, 0, 0),
        (3, 7, 100.0, 0, 0, 2), (0, 0, 100.0, 0, 0, 2), (0, 7, 100.0, 0, NONE, NONE), (2, 3, 100.0, 5, 0, 1),
    ]),
    "wall": (99.5, 4, [(2, 3, 100.0, 20, 0, 1), (2, 5, 100.0, 0, 1, 0), (2, 1, 30.0, 0, NONE, NONE), (0, 4, 50.0, 0, 0, 1)]),
    "row": (0.0, 0, [(0, 1, 100.0, 0, NONE, NONE), (0, 11, 100.0, 5, 0, 1), (0, 0, 3.0, 0, 1, 0)]),
    "col": (0.0, 0, [(1, 0, 100.0, 60, 1, 2), (11, 0, 100.0, 0, NONE, NONE), (5, 0, 100.0, 0, 0, NONE)]),
    "dot": (0.0, 0, [(0, 0, 50.0, 0, NONE, 0), (0, 0, 50.0, 0, NONE, NONE), (0, 0, 50.0, 0, 0, 0)]),
    "one": (0.0, 1, [(2, 4, 50.0, 5, NONE, 0), (2, 3, 50.0, 0, 0, NONE), (2, 3, 50.0, 0, NONE, 0)]),
    "shared": (0.0, 2, [(3, 4, 100.0, 7, 2, 1), (3, 3, 100.0, 0, NONE, NONE), (3, 3, 100.0, 0, 2, NONE), (3, 3, 100.0, 0, 2, 1),
                        (1, 5, 100.0, 0, 0, 0)]),
    "many": (20.0, 6, [(1, 1, 100.0, 0, NONE, NONE), (5, 6, 200.0, 0, 49, 3), (1, 2, 5.0, 20, 5, 0), (8, 12, 9.0, 0, 1, 63),
                       (6, 9, 100.0, 0, 2, NONE)]),
    "many100": (1e9, 100, [(1 + i // 11, 1 + i % 11, f, c, 63 - i, 63 - i) for i in range(8) for f, c in ((1.0, 0), (2e9, 0))]),
    "empty": (0.0, 0, [(1, 1, 50.0, 0, NONE, NONE), (1, 1, 50.0, 0, NONE, 0), (3, 4, 50.0, 0, 0, 254)]),
}


def make(name, reps=64, extra=3, seed=SEED):
    """The world's env holding every hand-placed ship `reps` times in a row (each one in every
    lane of a wave) and `extra` more: n = 64 k + 3."""
    world = WORLDS[name]
    rb, load, ships = CASES[name]
    idx = np.concatenate([np.repeat(np.arange(len(ships)), reps), np.arange(extra) % len(ships)])
    st = O.OracleState(len(idx))
    for i, j in enumerate(idx):
        st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = ships[j]
    env = world.env(st.n, seed=seed)
    load_state(env, st)
    return env, world, st, rb, load


def navigator(env, rb, load):
    from shippingenv_amd.nav import VecNavigator

    return VecNavigator(env, refuel_below=rb, load=load)


def numpy_result(res):
    out = {f: getattr(res, f).cpu().numpy() for f in FIELDS}
    assert out["ret"].dtype == np.float64 and out["fuel"].dtype == np.float64
    assert all(out[f].dtype == np.int32 for f in FIELDS if f not in ("ret", "fuel"))
    return out


BAD = None  # a bad source's rollout


def expected(navs):
    """[nav_support.NavRollout or BAD] -> the arrays se_rollout_nav writes."""
    cols = {f: [] for f in FIELDS}
    for nv in navs:
        if nv is BAD:
            row = dict(ret=0.0, steps=0, status=PS.BAD_SRC, arrivals=0, nav_status=0, stuck_at=-1, raised=0, first_err=0,
                       first_err_at=-1, **dict(zip(SHIP, PS.BAD_SHIP)))
        else:
            r = nv.res
            row = dict(ret=r.ret, steps=r.steps, status=r.status, arrivals=nv.arrivals, nav_status=nv.nav_status,
                       stuck_at=nv.stuck_at, raised=r.raised, first_err=r.first_err, first_err_at=r.first_err_at,
                       **dict(zip(SHIP, r.ship)))
        for f in FIELDS:
            cols[f].append(row[f])
    return {f: np.array(v, np.float64 if f in ("ret", "fuel") else np.int32) for f, v in cols.items()}


def assert_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        if f in ("ret", "fuel"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {f}")


def restate(world, st, src, steps, rb, load, ids, seed=SEED, tab=None):
    sp = PS.Stepper(O, world.oracle(O), seed)
    out = []
    for r, i in enumerate(src):
        if not 0 <= i < st.n:
            out.append(BAD)
            continue
        out.append(NS.nav_rollout(O, world, PS.ship_of(st, i), steps, rb, load, seed, int(ids[r]), stepper=sp, tab=tab))
    return out


def assert_equals_the_plan(env, src, navs, got, ids, what):
    """The contract: se_rollout_plan on the same env and ids, fed the actions the navigator
    emitted, gives the navigated rollout's ret (bits), counted, raised, done-ness and end ship."""
    plans = [[] if nv is BAD else nv.actions for nv in navs]
    ty, a, b, lens = PS.pack(plans, K=max(max(len(p) for p in plans), 1))
    res = env.rollout_plan(np.asarray(src, np.int32), rows(env, ty), rows(env, a), rows(env, b), lengths=lens,
                           ids=np.asarray(ids, np.int64), return_end=True)
    plan = {f: getattr(res, f).cpu().numpy() for f in ("ret", "steps", "raised", "status") + SHIP}
    assert_equal(got, plan, what + " vs se_rollout_plan", fields=("ret", "steps", "raised") + SHIP)
    np.testing.assert_array_equal(got["status"] == PS.DONE, plan["status"] == PS.DONE, err_msg=what + ": done-ness")
    np.testing.assert_array_equal(got["status"] == PS.BAD_SRC, plan["status"] == PS.BAD_SRC)


# ----------------------------------------------------------------- 1. se_nav_actions
@pytest.mark.parametrize("name", list(CASES))
def test_actions_equal_the_restatement_and_step_without_error(name):
    env, world, st, rb, load = make(name)
    assert env.n % 64 == 3
    nav = navigator(env, rb, load)
    tab = NS.tables(world)
    np.testing.assert_array_equal(nav.fields(), tab.fields())
    np.testing.assert_array_equal(nav.directions(), tab.dirs())
    assert nav.max_leg == tab.max_leg()
    before = snapshot(env)
    ty, a, b, status, agent, dist = (t.cpu().numpy() for t in nav.actions(agent=True, dist=True))
    assert_untouched(env, before, "se_nav_actions")
    want = [NS.nav_action(world, tab, PS.ship_of(st, i), rb, load) for i in range(st.n)]
    np.testing.assert_array_equal(np.stack([ty, a, b], 1), np.array([w[0] for w in want], np.int32), err_msg="action")
    np.testing.assert_array_equal(status, [w[1] for w in want], err_msg="status")
    np.testing.assert_array_equal(dist, [w[2] for w in want], err_msg="dist")
    np.testing.assert_array_equal(agent, [NS.agent_index(world.P, w[0], w[1]) for w in want], err_msg="agent")
    np.testing.assert_array_equal(nav.distance().cpu().numpy(), dist)
    every = {"open": {0, 1, 2}, "lake": {0, 1, 2}, "dot": {1, 2}, "one": {0, 1}, "empty": {1, 2}, "many100": {0}}
    assert set(status.tolist()) == every.get(name, set(status.tolist()))
    if name == "open":
        assert set(ty.tolist()) == {0, 1, 2, 3, 4}
    if name == "many100":  # amounts 49 / 199 have an index, 50, 100, 200 and 250 have none
        amounts = {(int(t), int(v)): int(g) for t, v, g in zip(ty, a, agent)}
        assert amounts == {(4, 49): 4 + 64 + 49, (4, 50): -1, (4, 100): -1, (4, 7): 4 + 64 + 7,
                           (3, 199): 54 + 64 + 199, (3, 200): -1, (3, 250): -1, (3, 3): 54 + 64 + 3}
    ok = status == NS.OK
    if world.P:  # every index decodes back to its action
        dty, da, db, derr = O.decode_agent(agent[agent >= 0], world.P)
        has = agent >= 0
        assert (derr == 0).all() and (dty == ty[has]).all() and (da == a[has]).all() and (db == b[has]).all()
        assert (has <= ok).all()
    # stepped through se_step_typed: no error wherever the navigator had an action, the no-op elsewhere
    fuel0 = env.fuel.cpu().numpy().copy()
    reward, done, err, status2 = nav.step()
    err = err.cpu().numpy()
    np.testing.assert_array_equal(status2.cpu().numpy(), status)
    assert (err[ok] == 0).all() and (err[~ok] != 0).all()
    assert (err[~ok] == (7 if world.P else 8)).all()  # BAD_CATEGORY; NO_PORTS comes first in a world without ports
    np.testing.assert_array_equal(env.fuel.cpu().numpy()[~ok].view(np.uint64), fuel0[~ok].view(np.uint64))
    nav.close()
    env.close()


# ----------------------------------------------------------------- 2. se_rollout_nav
@pytest.mark.parametrize("name", list(CASES))
def test_rollouts_equal_the_restatement_and_the_plan(name):
    """Every hand-placed ship from every lane of a wave and a ragged last wave at 21 positions;
    0, 1 and 2 positions on the first 67 rollouts."""
    env, world, st, rb, load = make(name)
    nav = navigator(env, rb, load)
    before = snapshot(env)
    base = (1 << 32) - 40  # the ids carry into the high word inside the batch
    seen = set()
    for steps, m in ((21, st.n), (0, 67), (1, 67), (2, 67)):
        src = np.arange(m, dtype=np.int32)
        ids = base + np.arange(m)
        navs = restate(world, st, src, steps, rb, load, ids)
        got = numpy_result(nav.rollout(src, steps=steps, rollout_base=base, return_end=True))
        assert_equal(got, expected(navs), f"{name} steps {steps}")
        assert (got["raised"] == 0).all() and (got["first_err_at"] == -1).all()
        if steps == 0:
            assert (got["ret"] == 0).all() and (got["steps"] == 0).all() and (got["status"] == PS.END).all()
        if world.P:
            assert_equals_the_plan(env, src, navs, got, ids, f"{name} steps {steps}")
        seen |= set(zip(got["status"].tolist(), got["nav_status"].tolist()))
        if steps == 21 and name == "row":
            assert got["arrivals"][:64].min() >= 2
    want = {"open": {(0, 0), (1, 0), (5, 1), (5, 2)}, "lake": {(1, 0), (5, 1), (5, 2)}, "dot": {(1, 0), (5, 1), (5, 2)},
            "one": {(5, 2), (5, 1), (1, 0)}, "empty": {(1, 0), (5, 1), (5, 2)}}
    assert want.get(name, set()) <= seen
    assert_untouched(env, before, name)
    nav.close()
    env.close()


def test_ids_bases_bad_sources_and_tiny_batches():
    env, world, st, rb, load = make("open")
    nav = navigator(env, rb, load)
    before = snapshot(env)
    rng = np.random.default_rng(11)
    m, steps = 197, 21
    src = rng.integers(0, st.n, m).astype(np.int32)
    bad = {0: -1, m - 1: st.n, 70: st.n + 7, 131: -(1 << 31), 64: (1 << 31) - 1}
    for k, v in bad.items():
        src[k] = v
    ids = rng.choice([5, 6, (1 << 40) + 3, (1 << 63) - 1, 0], m).astype(np.int64)  # duplicates and 64-bit ids
    navs = restate(world, st, src, steps, rb, load, ids)
    got = numpy_result(nav.rollout(src, steps=steps, ids=ids, rollout_base=999, return_end=True))
    assert_equal(got, expected(navs), "ids")
    where = np.array(sorted(bad))
    assert (got["status"][where] == PS.BAD_SRC).all() and (got["status"] == PS.BAD_SRC).sum() == len(where)
    assert_equals_the_plan(env, src, navs, got, ids, "ids")
    # equal ids and sources: equal results, whatever the lane (common random numbers)
    same = numpy_result(nav.rollout(np.full(m, 7 * 64, np.int32), steps=steps, ids=np.full(m, (1 << 40) + 3), return_end=True))
    for f in FIELDS:
        assert (same[f] == same[f][0]).all(), f
    # rollout_base names the ids of a sub-batch
    good = np.where(src < 0, 0, np.minimum(src, st.n - 1)).astype(np.int32)
    whole = numpy_result(nav.rollout(good, steps=steps, rollout_base=(1 << 32) - 100, return_end=True))
    for lo, hi in ((0, 64), (130, 197), (m - 1, m)):
        part = numpy_result(nav.rollout(good[lo:hi], steps=steps, rollout_base=(1 << 32) - 100 + lo, return_end=True))
        assert_equal(part, {f: v[lo:hi] for f, v in whole.items()}, f"sub-batch [{lo}, {hi})")
    by_ids = numpy_result(nav.rollout(good, steps=steps, ids=(1 << 32) - 100 + np.arange(m), rollout_base=3, return_end=True))
    assert_equal(by_ids, whole, "ids = base + arange")
    # src=None: every env once; an empty batch
    every = numpy_result(nav.rollout(steps=2, return_end=True))
    assert_equal(every, expected(restate(world, st, np.arange(st.n), 2, rb, load, np.arange(st.n))), "src=None")
    none = nav.rollout(np.zeros(0, np.int32), steps=5, return_end=True)
    assert all(getattr(none, f).numel() == 0 for f in FIELDS)
    assert nav.rollout(np.zeros(0, np.int32)).x is None
    assert_untouched(env, before, "ids")
    nav.close()
    env.close()


def test_one_env_and_no_envs():
    for n in (1, 0):
        env = RS.OPEN.env(n)
        nav = navigator(env, 50.0, 2)
        if n:
            st = O.OracleState(1)
            st.x[0], st.y[0], st.fuel[0], st.cargo[0], st.origin[0], st.dest[0] = (1, 1, 10.0, 0, 2, 1)
            load_state(env, st)
        ty, a, b, status, agent, dist = nav.actions(agent=True, dist=True)
        assert ty.numel() == n
        if n:
            assert (ty.item(), a.item(), b.item(), status.item(), agent.item(), dist.item()) == (3, 9, 0, 0, 54 + 4 + 9, 9)
            got = numpy_result(nav.rollout(steps=3, rollout_base=4, return_end=True))
            assert_equal(got, expected(restate(RS.OPEN, st, [0], 3, 50.0, 2, [4])), "n = 1")
        else:
            assert nav.rollout(steps=3).ret.numel() == 0 and nav.step()[3].numel() == 0
        nav.close()
        env.close()


def test_more_rollouts_than_threads():
    """2048 * 256 + 257 rollouts: the first 257 lanes run a second rollout. Sources and ids repeat
    with period 256, so the result is the 256 restated rollouts tiled; a bad source on each side
    of the wrap."""
    env, world, st, rb, load = make("open")
    nav = navigator(env, rb, load)
    before = snapshot(env)
    m, steps, base = GRID_THREADS + 257, 6, (1 << 32) - 128
    src256 = (np.arange(256) * 61 % st.n).astype(np.int32)
    want256 = expected(restate(world, st, src256, steps, rb, load, base + np.arange(256)))
    assert {PS.DONE, PS.END, NS.STUCK} <= set(want256["status"].tolist())
    reps = -(-m // 256)
    src = np.tile(src256, reps)[:m].copy()
    bad = [GRID_THREADS - 1, GRID_THREADS + 5]
    src[bad] = [st.n, -1]
    ids = torch.as_tensor(base + np.arange(m) % 256, dtype=torch.int64)
    got = numpy_result(nav.rollout(src, steps=steps, ids=ids, rollout_base=12345, return_end=True))
    want = {f: np.tile(v, reps)[:m].copy() for f, v in want256.items()}
    blank = expected([BAD])
    for f in FIELDS:
        want[f][bad] = blank[f][0]
    assert_equal(got, want, "grid stride")
    assert_untouched(env, before, "grid stride")
    nav.close()
    env.close()


class BuiltTables:
    """The library's host tables behind nav_support.Tables' lookups (tests/test_nav_cpu.py pins the
    builder to the restatement; a 254-port restatement in Python would take minutes)."""

    def __init__(self, field, dirs):
        self._f, self._d = field.astype(np.int32), dirs

    def field(self, p):
        return self._f[p]

    def dir(self, p):
        return self._d[p]


def test_largest_world_takes_the_large_lds_path():
    """256 x 256 cells and 254 ports: the world image is past 64 KiB, the tables hold 254 * 65536
    entries. 65 rollouts of 12 positions from envs after a reset and 40 random steps, and the
    policy's action for every env."""
    w = RS.max_world()
    n, m, steps = 33, 65, 12
    env = w.env(n, seed=31)
    env.reset()
    for t in range(40):
        env.step(env.gen_actions(t))
    st = oracle_state(env)
    nav = navigator(env, 150.0, 3)
    tab = BuiltTables(nav.fields(), nav.directions())
    for p in (0, 253):  # two of the 254 fields against the restatement
        f = NS.bfs(NS.open_mask(w), tuple(w.ports[p]))
        np.testing.assert_array_equal(tab.field(p), f)
        np.testing.assert_array_equal(tab.dir(p), NS.directions(f))
    before = snapshot(env)
    ty, a, b, status, dist = (t.cpu().numpy() for t in nav.actions(dist=True))
    want = [NS.nav_action(w, tab, PS.ship_of(st, i), 150.0, 3) for i in range(n)]
    np.testing.assert_array_equal(np.stack([ty, a, b], 1), np.array([x[0] for x in want], np.int32))
    np.testing.assert_array_equal(status, [x[1] for x in want])
    np.testing.assert_array_equal(dist, [x[2] for x in want])
    rng = np.random.default_rng(65)
    src = rng.integers(0, n, m).astype(np.int32)
    src[17] = n
    ids = 9 + np.arange(m)
    navs = restate(w, st, src, steps, 150.0, 3, ids, seed=31, tab=tab)
    got = numpy_result(nav.rollout(src, steps=steps, rollout_base=9, return_end=True))
    assert_equal(got, expected(navs), "max world")
    assert got["steps"].sum() > m
    assert_equals_the_plan(env, src, navs, got, ids, "max world")
    assert_untouched(env, before, "max world")
    nav.close()
    env.close()


def test_captured_call_replays_to_the_eager_result():
    """Each call is one launch on the current stream and nothing else, so torch.cuda.graph captures
    both; the replay equals the eager calls and leaves the env alone."""
    env, world, st, rb, load = make("open")
    nav = navigator(env, rb, load)
    before = snapshot(env)
    m = 257
    src = torch.as_tensor(np.random.default_rng(9).integers(0, st.n, m).astype(np.int32), device=env.device)
    ids = torch.arange(m, dtype=torch.int64, device=env.device) + (1 << 36)
    eager = numpy_result(nav.rollout(src, steps=21, ids=ids, return_end=True))
    eager_act = [t.cpu().numpy().copy() for t in nav.actions(agent=True, dist=True)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = nav.rollout(src, steps=21, ids=ids, return_end=True)
            acts = nav.actions(agent=True, dist=True)
    for t in tuple(getattr(res, f) for f in FIELDS) + tuple(acts):  # capture launched nothing: the replay has to write
        t.fill_(POISON)
    with torch.cuda.stream(side):
        g.replay()
    torch.cuda.synchronize()
    assert_equal(numpy_result(res), eager, "replay")
    for got, want in zip(acts, eager_act):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_untouched(env, before, "capture")
    nav.close()
    env.close()


def test_set_ports_between_calls():
    """Through the C-ABI a handle made for other ports answers SE_ESTATE and launches nothing until
    se_nav_rebuild; VecNavigator rebuilds by itself; the results follow the new ports."""
    from shippingenv_amd import _native as N
    from shippingenv_amd._native import _ptr

    env, world, st, rb, load = make("open")
    nav = navigator(env, rb, load)
    lib = N.lib()
    first = [t.cpu().numpy().copy() for t in nav.actions(dist=True)]
    moved = RS.World(7, 9, ports=[(5, 6), (1, 1), (5, 2)], fuel=[2, 3, 4], cargo=[1, 0, 9], ground=[(2, 5)])
    env.set_ports(moved.ports, moved.fuel_stock, moved.cargo_stock)
    outs = [torch.full((env.n,), POISON, dtype=torch.int32, device=env.device) for _ in range(4)]
    rc = lib.se_nav_actions(nav._h, rb, load, *[_ptr(t) for t in outs], None, None, env._stream())
    assert rc == -3 and "se_nav_rebuild" in lib.se_last_error().decode()
    ret = torch.full((4,), float(POISON), dtype=torch.float64, device=env.device)
    cnt, status, src = (torch.full((4,), POISON, dtype=torch.int32, device=env.device) for _ in range(3))
    src.zero_()
    rc = lib.se_rollout_nav(nav._h, _ptr(src), 4, 3, rb, load, None, 0, _ptr(ret), _ptr(cnt), _ptr(status), None, env._stream())
    assert rc == -3 and "se_nav_rebuild" in lib.se_last_error().decode()
    leg = C.c_int32(POISON)
    assert lib.se_nav_tables(nav._h, None, None, C.byref(leg)) == -3 and leg.value == POISON
    torch.cuda.synchronize()
    assert all((t == POISON).all() for t in outs + [ret, cnt, status]), "a stale handle launched something"
    # the class rebuilds by itself
    tab = NS.tables(moved)
    assert nav.max_leg == tab.max_leg()
    np.testing.assert_array_equal(nav.fields(), tab.fields())
    ty, a, b, status, dist = (t.cpu().numpy() for t in nav.actions(dist=True))
    want = [NS.nav_action(moved, tab, PS.ship_of(st, i), rb, load) for i in range(st.n)]
    np.testing.assert_array_equal(np.stack([ty, a, b], 1), np.array([w[0] for w in want], np.int32))
    np.testing.assert_array_equal(status, [w[1] for w in want])
    np.testing.assert_array_equal(dist, [w[2] for w in want])
    assert not np.array_equal(first[4], dist)
    src = np.arange(st.n, dtype=np.int32)
    got = numpy_result(nav.rollout(src, steps=9, rollout_base=77, return_end=True))
    assert_equal(got, expected(restate(moved, st, src, 9, rb, load, 77 + src)), "after set_ports")
    # a second change, met by rollout first; then by hand through the C-ABI
    env.set_ports(world.ports, world.fuel_stock, world.cargo_stock)
    got = numpy_result(nav.rollout(src, steps=9, rollout_base=77, return_end=True))
    assert_equal(got, expected(restate(world, st, src, 9, rb, load, 77 + src)), "back to the first ports")
    env.set_ports(moved.ports, moved.fuel_stock, moved.cargo_stock)
    assert lib.se_nav_rebuild(nav._h) == 0 and lib.se_nav_tables(nav._h, None, None, C.byref(leg)) == 0
    assert leg.value == tab.max_leg()
    nav.close()
    env.close()


# ----------------------------------------------------------------- 3. the workload's own shape
def test_default_world_at_65536_envs_after_a_random_pre_roll(water):
    """n = 2^16 on the builtin map after a reset and 50 random steps, 100 positions: 16 slices of
    64 rollouts against the restatement; the navigator's own parameters (refuel_below from
    max_leg)."""
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.vec import VecEnv

    n, steps, load = 1 << 16, 100, 5
    env = VecEnv(n, seed=0)
    np.testing.assert_array_equal(env.water, water)
    world = NS.default_world(water, seed=0)
    assert world.fuel_stock == env.port_fuel.tolist() and world.cargo_stock == env.port_cargo.tolist()
    env.reset()
    for t in range(50):
        env.step(env.gen_actions(t))
    nav = VecNavigator(env, load=load)
    tab = NS.tables(world)
    assert nav.max_leg == tab.max_leg() == 72 and nav.refuel_below == 1.1 * 73
    rb = nav.refuel_below
    before = snapshot(env)
    res = nav.rollout(steps=steps, rollout_base=1 << 20, return_end=True)
    dist = nav.distance().cpu().numpy()
    got = numpy_result(res)
    assert_untouched(env, before, "2^16")
    st = oracle_state(env)
    picked = np.concatenate([np.arange(lo, lo + 64) for lo in range(0, n, n // 16)])
    navs = restate(world, st, picked, steps, rb, load, (1 << 20) + picked, seed=0)
    assert_equal({f: v[picked] for f, v in got.items()}, expected(navs), "2^16 slices")
    want_dist = [NS.nav_action(world, tab, PS.ship_of(st, i), rb, load)[2] for i in picked]
    np.testing.assert_array_equal(dist[picked], want_dist)
    assert (got["raised"] == 0).all() and (got["arrivals"] > 0).mean() > 0.5
    nav.close()
    env.close()
