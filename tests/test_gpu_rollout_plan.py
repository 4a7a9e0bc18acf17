"""se_rollout_plan / VecEnv.rollout_plan on the GPU, bit for bit (ret and fuel as uint64).

The pin: a scripted rollout whose plan is the attempt list of se_rollout's rollout with the same
id equals that rollout, against both the C oracle's rollout and the GPU's own. Everything the
random policy cannot reach (every error a typed action can raise, moves of +-(2^31 - 1), pads,
lengths, ids, agent-index plans, the batch's shape, the grid-stride loop, the largest world) is
held to the restatement of tests/plan_support.py, which tests/test_rollout_plan_cpu.py pins to
the oracle's rollout on the CPU."""
import numpy as np
import pytest

import plan_support as PS
import rollout_support as RS
from test_gpu_rollout import load_state, oracle_state

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

SHIP = ("x", "y", "fuel", "cargo", "origin", "dest")
FIELDS = ("ret", "steps", "status", "raised", "first_err", "first_err_at") + SHIP
GRID_THREADS = 2048 * 256  # the most threads the kernel launches
I31 = (1 << 31) - 1
GARBAGE = 0x7F7F7F7F  # fills what the kernel must not read: as a type, an amount or a move it raises or shows


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def table_env(name, seed=RS.SEED):
    w = RS.WORLDS[name]
    st = RS.table(O, name)
    env = w.env(st.n, seed=seed)
    load_state(env, st)
    return env, w.oracle(O), st


def snapshot(env):
    """Everything a rollout must leave alone, as bytes."""
    t = {f: getattr(env, f).cpu().numpy().copy() for f in SHIP + ("reward", "done", "err")}
    return {k: v.view(np.uint8) for k, v in t.items()}, env.counters


def assert_untouched(env, before, what=""):
    after = snapshot(env)
    assert after[1] == before[1], f"{what}: counters"
    for f, v in before[0].items():
        np.testing.assert_array_equal(after[0][f], v, err_msg=f"{what}: the rollout changed {f}")


def rows(env, arr, ld=None):
    """A host [K, m] array as an int32 device view with rows ld apart (a multiple of 4, so the
    rows are 16-byte aligned); the pad between rows is GARBAGE."""
    arr = np.asarray(arr, np.int32)
    K, m = arr.shape
    ld = (m + 3) // 4 * 4 if ld is None else ld
    assert ld >= m and ld % 4 == 0
    buf = torch.full((max(K, 1), max(ld, 4)), GARBAGE, dtype=torch.int32, device=env.device)
    view = buf[:K, :m]
    view.copy_(torch.as_tensor(arr, device=env.device))
    return view


def numpy_result(res):
    out = {f: getattr(res, f).cpu().numpy() for f in FIELDS}
    assert out["ret"].dtype == np.float64 and out["fuel"].dtype == np.float64
    assert all(out[f].dtype == np.int32 for f in FIELDS if f not in ("ret", "fuel"))
    return out


def run_typed(env, src, ty, a, b, ld=None, **kw):
    res = env.rollout_plan(np.asarray(src, np.int32), rows(env, ty, ld), rows(env, a, ld), rows(env, b, ld),
                           return_end=True, **kw)
    return numpy_result(res)


def run_agent(env, src, idx, ld=None, **kw):
    return numpy_result(env.rollout_plan(np.asarray(src, np.int32), actions=rows(env, idx, ld), return_end=True, **kw))


def expected(results):
    """[plan_support.Result] -> the arrays se_rollout_plan writes."""
    out = {f: np.array([getattr(r, f) for r in results], np.float64 if f == "ret" else np.int32) for f in FIELDS[:6]}
    for j, f in enumerate(SHIP):
        out[f] = np.array([r.ship[j] for r in results], np.float64 if f == "fuel" else np.int32)
    return out


def assert_equal(got, want, what="", fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        if f in ("ret", "fuel"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {f}")


def restate(world, st, src, plans, ids, lengths=None, agent=False, seed=RS.SEED):
    """The restatement's result for every rollout (a bad source: zeros and -1)."""
    sp = PS.Stepper(O, world, seed)
    out = []
    for r, i in enumerate(src):
        if not 0 <= i < st.n:
            out.append(PS.Result(PS.BAD_SHIP, PS.BAD_SRC))
            continue
        out.append(PS.plan_rollout(O, world, PS.ship_of(st, i), plans[r], seed, int(ids[r]),
                                   length=None if lengths is None else lengths[r], agent=agent, stepper=sp))
    return out


# ----------------------------------------------------------------- 1. equals the random rollout
@pytest.mark.parametrize("base", [0, (1 << 32) - 100, (1 << 40) + 3])
@pytest.mark.parametrize("name", list(RS.WORLDS))
def test_random_plans_equal_the_random_rollouts(name, base):
    """Each world's table (every actor in every lane of a wave) at BUDGET: the scripted rollout of
    the random policy's attempts equals oracle.rollout and env.rollout of the same base in ret,
    steps, DONE or not and the end ship. Base 2^32 - 100: the ids carry into the high word inside
    the batch."""
    env, world, st = table_env(name)
    before = snapshot(env)
    src = RS.table_src(name)
    ms, ma = RS.BUDGET
    plans, results = PS.random_table(O, RS, name, base)
    ty, a, b, lens = PS.pack(plans, K=ma)
    got = run_typed(env, src, ty, a, b, lengths=lens, rollout_base=base)
    assert_equal(got, expected(results), f"{name} base {base} vs the restatement")
    ret, steps, status, log = O.rollout(world, st, src, max_steps=ms, max_attempts=ma, seed=RS.SEED,
                                        rollout_base=base, trace=True)
    dev = [v.cpu().numpy() for v in env.rollout(src, max_steps=ms, max_attempts=ma, rollout_base=base)]
    for who, (r_ret, r_steps, r_status) in (("oracle.rollout", (ret, steps, status)), ("env.rollout", dev)):
        np.testing.assert_array_equal(got["ret"].view(np.uint64), r_ret.view(np.uint64), err_msg=f"{who}: ret")
        np.testing.assert_array_equal(got["steps"], r_steps, err_msg=f"{who}: steps")
        np.testing.assert_array_equal(got["status"] == PS.DONE, r_status == RS.DONE, err_msg=f"{who}: done")
    np.testing.assert_array_equal(got["raised"], log["raised"])
    assert_equal(got, log, f"{name} base {base} vs the oracle's end ship", fields=SHIP)
    # without lengths the pads are played and raise: more raises, nothing else
    padded = run_typed(env, src, ty, a, b, rollout_base=base)
    assert_equal(padded, got, "padded", fields=("ret", "steps", "status") + SHIP)
    open_end = got["status"] == PS.END
    np.testing.assert_array_equal(padded["raised"][open_end], (got["raised"] + (ma - lens))[open_end])
    assert_untouched(env, before, name)
    env.close()


# ----------------------------------------------------------------- 2. hand-written plans
N, E, S, W = (1, 0, -1), (1, -1, 0), (1, 0, 1), (1, 1, 0)
PAD = (0, 0, 0)
HAND = [  # (actor of world `open`, plan, what it is for)
    ("corner_first", [E, S, N, S, (1, -1, -1), W], "OOB in the middle and a diagonal one"),
    ("select_other_origin", [(2, 2, 0), (2, 4, 0), (2, -1, 0), (2, I31, 0), (2, 1, 0), S, S], "same port, port range, then a select that holds"),
    ("loaded_30", [(3, 1, 0), (4, 1, 0), S, (3, 0, 0)], "not at port"),
    ("take_at_port", [(4, 7, 0), (4, 0, 0), (4, -1, 0), (3, 5, 0), (3, 4, 0), (4, 6, 0), N], "amounts past the stock, zero, negative; the whole stock"),
    ("no_dest_at_sea", [N, S, (1, I31, 0), (2, 1, 0)], "no destination, also before out of range; a select at sea holds"),
    ("loaded_30", [(0, 0, 1), N, (5, 0, 1), (-1, 0, 1), E, (I31, 0, 0), (-I31 - 1, 0, 0)], "bad categories 0, 5, -1 and the int32 edges"),
    ("loaded_30", [(1, I31, 0), (1, 0, -I31), (1, -I31, I31), (1, -I31 - 1, 0), (1, 257, 0), (1, 0, -257), S], "moves of +-(2^31 - 1)"),
    ("low_fuel", [S, N, S, N, (0, 0, 0), S], "runs dry mid-plan with actions after it"),
    ("loaded_60", [PAD, N, S, E, W, N], "a raising action first"),
    ("loaded_60", [N, S, E, W, N, PAD], "... last"),
    ("loaded_60", [N, PAD, PAD, S, E, W], "... twice in a row"),
    ("loaded_60", [PAD, (5, 1, 1), (1, I31, I31), (3, 1, 0)], "raises only"),
    ("next_to_dest", [S, N, W, S, E, S], "an arrival at the first step, then on with the new destination"),
    ("corner_last", [(1, 0, -2), (1, -2, 0), (1, -1, -2), (1, 3, 3)], "longer moves: the sqrt in the fuel cost"),
    ("select_other_origin", [(2, 4, 0), (2, 1, 0)], "port range as the first error"),
]


def test_hand_written_plans_on_world_open():
    """Every SE_ERR_* a typed action can raise, the int32 edges, a rollout that ends mid-plan,
    raising actions first, last, twice in a row and alone, an arrival and a partial loss: each
    case in all 64 lanes of a wave (64 ids), against the restatement."""
    env, world, st = table_env("open")
    before = snapshot(env)
    labels = [a[0] for a in RS.actors("open")]
    src = np.repeat([labels.index(h[0]) for h in HAND], 64).astype(np.int32)
    plans = [h[1] for h in HAND for _ in range(64)]
    base = (1 << 33) + 5
    results = restate(world, st, src, plans, base + np.arange(len(src)))
    want = expected(results)
    # the cases hold what they are for
    by_case = {k: results[64 * k:64 * (k + 1)] for k in range(len(HAND))}
    assert {r.first_err for r in results} == {0, 1, 2, 3, 4, 5, 6, 7}
    assert by_case[1][0].raised == 4 and by_case[3][0].raised == 4 and by_case[3][0].steps == 3
    assert all(r.raised == 3 and r.steps == 1 for r in by_case[4])
    assert all(r.raised == 5 and r.steps == 2 for r in by_case[5])
    assert all(r.raised == 6 and r.steps == 1 for r in by_case[6])
    assert all(r.status == PS.DONE and r.steps <= 2 for r in by_case[7])
    assert all(r.first_err_at == 0 and r.raised == 1 for r in by_case[8])
    assert all(r.first_err_at == 5 for r in by_case[9]) and all(r.first_err_at == 1 and r.raised == 2 for r in by_case[10])
    assert all(r.steps == 0 and r.raised == 4 and r.ret == 0.0 and r.status == PS.END for r in by_case[11])
    assert all(r.used & PS.USED_ARRIVE for r in by_case[12])
    assert any(r.used & PS.USED_BETA for k in (8, 9, 10) for r in by_case[k])
    assert all(r.steps == 4 and r.raised == 0 for r in by_case[13])
    assert all(r.first_err == 3 and r.steps == 1 for r in by_case[14])
    ty, a, b, lens = PS.pack(plans)
    got = run_typed(env, src, ty, a, b, lengths=lens, rollout_base=base)
    assert_equal(got, want, "hand-written plans")
    assert_untouched(env, before, "hand-written plans")
    env.close()


# ----------------------------------------------------------------- 3. shapes
# unit moves beside a longer one, a diagonal and a move of no length: the lanes of one wave differ
# in whether their move's fuel cost needs a square root
MENU = [N, E, S, W, N, S, E, W, (2, 1, 0), (2, 3, 0), (4, 1, 0), (3, 1, 0), PAD, (1, 2, 0), (1, 1, -1), (1, 0, 0)]


def menu_plans(rng, m, K):
    return [[MENU[j] for j in rng.integers(0, len(MENU), K)] for _ in range(m)]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_batch_sizes_sources_lengths_and_strides(m):
    """Batches around a wave and past a workgroup with shuffled repeated sources; bad sources
    first, last and mid-wave; K = 0, 1, 2 and 5; lengths 0, K, past K and negative, differing
    inside a wave; rows further apart than m with garbage between them."""
    env, world, st = table_env("open")
    before = snapshot(env)
    rng = np.random.default_rng(m)
    n = st.n
    for K in (0, 1, 2, 5):
        src = rng.integers(0, n, m).astype(np.int32)
        plans = menu_plans(rng, m, K)
        ids = 1000 + np.arange(m)
        ty, a, b, _ = PS.pack(plans, K=K)
        got = run_typed(env, src, ty, a, b, rollout_base=1000)
        assert_equal(got, expected(restate(world, st, src, plans, ids)), f"m={m} K={K}")
        if K == 0:
            assert (got["ret"] == 0).all() and (got["steps"] == 0).all() and (got["status"] == PS.END).all()
        bad = {0: -1, m - 1: n, m // 2: n + 7}
        if m > 128:
            bad.update({64 + 31: -(1 << 31), 63: I31})
        for k, v in bad.items():
            src[k] = v
        lens = rng.choice([0, K, K + 3, -2, 1, K - 1, I31, -I31 - 1], m).astype(np.int32)
        wide = run_typed(env, src, ty, a, b, ld=(m + 3) // 4 * 4 + 8, lengths=lens, rollout_base=1000)
        want = expected(restate(world, st, src, plans, ids, lengths=lens))
        assert_equal(wide, want, f"m={m} K={K} with bad sources, lengths and a wide stride")
        where = np.array(sorted(bad))
        assert (wide["status"][where] == PS.BAD_SRC).all() and (wide["status"] == PS.BAD_SRC).sum() == len(where)
        assert (wide["ret"][where] == 0).all() and (wide["steps"][where] == 0).all() and (wide["x"][where] == -1).all()
    assert_untouched(env, before, f"m={m}")
    env.close()


def test_empty_batch_and_argument_checks():
    env, _, _ = table_env("open")
    before = snapshot(env)
    z = torch.zeros((3, 0), dtype=torch.int32, device=env.device)
    res = env.rollout_plan(np.zeros(0, np.int32), z, z, z, return_end=True)
    assert all(getattr(res, f).numel() == 0 for f in FIELDS)
    res = env.rollout_plan(np.zeros(0, np.int32), actions=z)
    assert res.ret.numel() == 0 and res.x is None and res.dest is None
    p = rows(env, np.zeros((3, 8), np.int32))
    src = np.zeros(8, np.int32)
    with pytest.raises(ValueError):
        env.rollout_plan(src, p, p, p, actions=p)  # both encodings
    with pytest.raises(ValueError):
        env.rollout_plan(src, p, p)  # half a typed plan
    with pytest.raises(ValueError):
        env.rollout_plan(src)
    with pytest.raises(ValueError):
        env.rollout_plan(src, p, p, p[:2])  # shapes differ
    with pytest.raises(ValueError):
        env.rollout_plan(src, actions=p.to(torch.int64))
    with pytest.raises(ValueError):
        env.rollout_plan(src, actions=p.cpu())
    with pytest.raises(ValueError):
        env.rollout_plan(src[:7], actions=p)  # m differs
    odd = torch.zeros((3, 9), dtype=torch.int32, device=env.device)[:, :7]  # rows 36 bytes apart
    with pytest.raises(ValueError):
        env.rollout_plan(src[:7], actions=odd)
    with pytest.raises(ValueError):
        env.rollout_plan(src, actions=p, lengths=np.zeros(7, np.int32))
    assert_untouched(env, before, "argument checks")
    env.close()


# ----------------------------------------------------------------- 4. grid stride
def test_more_rollouts_than_threads():
    """2048 * 256 + 257 rollouts: the first 257 lanes run a second rollout. ids, sources and plan
    columns repeat with period 256, so the result is the 256 restated rollouts tiled; one bad
    source on each side of the wrap."""
    env, world, st = table_env("open")
    before = snapshot(env)
    labels = [a[0] for a in RS.actors("open")]
    four = np.array([labels.index(k) for k in ("next_to_dest", "loaded_60", "corner_last", "low_fuel")], np.int32)
    m, K, base = GRID_THREADS + 257, 6, (1 << 32) - 128
    rng = np.random.default_rng(4)
    plans = menu_plans(rng, 256, K)
    src256 = four[np.arange(256) % 4]
    want256 = expected(restate(world, st, src256, plans, base + np.arange(256)))
    assert {PS.DONE, PS.END} <= set(want256["status"].tolist()) and (want256["raised"] > 0).any()
    reps = -(-m // 256)
    ty, a, b, _ = PS.pack(plans, K=K)
    tile = lambda v: np.tile(v, (1, reps))[:, :m] if v.ndim == 2 else np.tile(v, reps)[:m]  # noqa: E731
    src = tile(src256).copy()
    bad = [GRID_THREADS - 1, GRID_THREADS + 5]
    src[bad] = [st.n, -1]
    ids = torch.as_tensor(base + np.arange(m) % 256, dtype=torch.int64)
    got = run_typed(env, src, tile(ty), tile(a), tile(b), ids=ids, rollout_base=12345)
    want = {f: tile(v).copy() for f, v in want256.items()}
    blank = expected([PS.Result(PS.BAD_SHIP, PS.BAD_SRC)])
    for f in FIELDS:
        want[f][bad] = blank[f][0]
    assert_equal(got, want, "grid stride")
    assert_untouched(env, before, "grid stride")
    env.close()


# ----------------------------------------------------------------- 5. ids
def test_ids_name_the_random_numbers():
    env, world, st = table_env("open")
    rng = np.random.default_rng(5)
    m, K, base = 333, 8, (1 << 32) - 100
    src = rng.integers(0, st.n, m).astype(np.int32)
    ty, a, b, _ = PS.pack(menu_plans(rng, m, K), K=K)
    whole = run_typed(env, src, ty, a, b, rollout_base=base)
    assert_equal(run_typed(env, src, ty, a, b, ids=base + np.arange(m), rollout_base=7), whole, "ids = base + arange")
    for lo, hi in ((0, 64), (130, 333), (m - 1, m)):  # the second starts past the carry
        part = run_typed(env, src[lo:hi], ty[:, lo:hi], a[:, lo:hi], b[:, lo:hi], rollout_base=base + lo)
        assert_equal(part, {f: v[lo:hi] for f, v in whole.items()}, f"sub-batch [{lo}, {hi})")
    other = run_typed(env, src, ty, a, b, rollout_base=base + 1)
    assert not np.array_equal(other["fuel"], whole["fuel"])
    # equal ids, plans and sources: equal results, whatever the lane
    one = lambda v: np.repeat(v[:, 5:6], m, axis=1)  # noqa: E731
    same = run_typed(env, np.full(m, src[5], np.int32), one(ty), one(a), one(b), ids=np.full(m, (1 << 40) + 3), rollout_base=0)
    for f in FIELDS:
        assert (same[f] == same[f][0]).all(), f
    env.close()


# ----------------------------------------------------------------- 6. agent-index plans
def agent_menu(P):
    return [0, 1, 2, 3, 0, 2, -1, -2, -3, -4, -5, -(1 << 31), 4, 4 + P - 1, 4 + P, 4 + P + 1, 4 + P + 49, 4 + P + 50,
            4 + P + 51, 4 + P + 249, 4 + P + 250, I31]


@pytest.mark.parametrize("name", ["open", "many"])
def test_agent_index_plans(name):
    """Agent-index plans equal the restatement (oracle.decode_agent, then the typed step; an
    index below -4 raises BAD_INDEX) and the GPU's typed run of the decoded plan. Indices -1,
    4 + P + 250 and 2^31 - 1 among them; P = 64 on `many`."""
    if name == "open":
        env, world, st = table_env("open")
    else:
        w = RS.MANY
        ships = [(1, 1, 100.0, 0, 0, -1), (5, 6, 200.0, 0, 49, 3), (1, 2, 50.0, 20, 5, 0), (8, 12, 9.0, 0, 1, 63)]
        st = O.OracleState(len(ships))
        for i, sh in enumerate(ships):
            st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = sh
        env, world = w.env(st.n), w.oracle(O)
        load_state(env, st)
    before = snapshot(env)
    P = world.P
    assert P == (4 if name == "open" else 64)
    rng = np.random.default_rng(P)
    m, K = 193, 7
    menu = agent_menu(P)
    src = rng.integers(0, st.n, m).astype(np.int32)
    plans = [[menu[j] for j in rng.integers(0, len(menu), K)] for _ in range(m)]
    idx = np.array(plans, np.int32).T.copy()
    assert {-1, 4 + P + 250, I31, -5} <= set(idx.ravel().tolist())
    lens = rng.integers(-1, K + 2, m).astype(np.int32)
    got = run_agent(env, src, idx, lengths=lens, rollout_base=(1 << 32) - 9)
    want = restate(world, st, src, plans, (1 << 32) - 9 + np.arange(m), lengths=lens, agent=True)
    assert_equal(got, expected(want), f"{name}: agent-index plans")
    assert {9, 5} <= {r.first_err for r in want} and any(r.steps > 2 for r in want)
    # the same plans typed, through oracle.decode_agent (a decode error becomes the pad)
    ty, a, b, err = (v.reshape(K, m) for v in O.decode_agent(idx.ravel(), P))
    ty = np.where(err != 0, 0, ty)
    typed = run_typed(env, src, ty, np.where(err != 0, 0, a), np.where(err != 0, 0, b), lengths=lens,
                      rollout_base=(1 << 32) - 9)
    assert_equal(typed, got, f"{name}: typed vs agent", fields=[f for f in FIELDS if f != "first_err"])
    differ = typed["first_err"] != got["first_err"]
    assert differ.any() and (typed["first_err"][differ] == 7).all() and (got["first_err"][differ] == 9).all()
    assert_untouched(env, before, name)
    env.close()


# ----------------------------------------------------------------- 7. world edges
def custom_env(w, ships):
    st = O.OracleState(len(ships))
    for i, sh in enumerate(ships):
        st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = sh
    env = w.env(st.n)
    load_state(env, st)
    return env, w.oracle(O), st


def test_world_edges_one_shared_heavy():
    """P = 1: an arrival picks its new destination over zero other ports (the plan ends there: the
    pick names a port that does not exist). A shared cell: the arrival at the second port on it.
    Cargo >= 2^21 in a partial loss."""
    # ONE: port 0 at (2, 3); a ship east of it bound for it
    env, world, st = custom_env(RS.ONE, [(2, 4, 50.0, 5, -1, 0), (2, 3, 50.0, 0, 0, -1)])
    src = np.repeat([0, 1], 64).astype(np.int32)
    plans = [[N]] * 64 + [[(2, 0, 0), (2, 1, 0), (4, 3, 0), (4, 1, 0), (3, 6, 0), (3, 7, 0)]] * 64
    ids = 50 + np.arange(128)
    want = restate(world, st, src, plans, ids)
    assert all(r.used & PS.USED_ARRIVE and r.ship[5] == 1 and r.ship[4] == 0 for r in want[:64])
    assert all(r.raised == 3 and r.steps == 3 for r in want[64:])
    ty, a, b, lens = PS.pack(plans)
    assert_equal(run_typed(env, src, ty, a, b, lengths=lens, rollout_base=50), expected(want), "one")
    env.close()
    # SHARED: the table's own actors, a plan that walks onto the shared cell and on
    env, world, st = table_env("shared")
    src = np.repeat([0, 1], 64).astype(np.int32)
    plans = [[N, S, N, E, W]] * 64 + [[(2, 1, 0), (2, 3, 0), (2, 0, 0), S, N]] * 64
    want = restate(world, st, src, plans, 50 + np.arange(128))
    assert all(r.used & PS.USED_ARRIVE for r in want[:64]) and all(r.raised == 2 for r in want[64:])
    ty, a, b, _ = PS.pack(plans)
    assert_equal(run_typed(env, src, ty, a, b, rollout_base=50), expected(want), "shared")
    env.close()
    # HEAVY: every actor with cargo >= 2^21 moves back and forth; the gate fires on every move
    env, world, st = table_env("heavy")
    src = RS.table_src("heavy")
    plans = [[N, S, E, W, (4, 1 << 22, 0), N]] * len(src)
    want = restate(world, st, src, plans, (1 << 35) + np.arange(len(src)))
    big = [r for r, i in zip(want, src) if st.cargo[i] >= RS.BIG]
    assert sum(1 for r in big if r.used & PS.USED_BETA) > len(big) // 2
    ty, a, b, _ = PS.pack(plans)
    assert_equal(run_typed(env, src, ty, a, b, rollout_base=1 << 35), expected(want), "heavy")
    env.close()


def test_largest_world_takes_the_large_lds_path():
    """256 x 256 cells and 254 ports: the world image is past 64 KiB. 65 rollouts from envs after a
    reset and 40 steps, typed and agent-index plans."""
    w = RS.max_world()
    n, m, K = 33, 65, 6
    env = w.env(n, seed=31)
    world = w.oracle(O)
    env.reset()
    for t in range(40):
        env.step(env.gen_actions(t))
    st = oracle_state(env)
    before = snapshot(env)
    rng = np.random.default_rng(65)
    src = rng.integers(0, n, m).astype(np.int32)
    src[17] = n
    menu = [N, E, S, W, (2, 253, 0), (2, 254, 0), (4, 1, 0), (1, 255, 0), (1, 0, -255), (3, 1, 0)]
    plans = [[menu[j] for j in rng.integers(0, len(menu), K)] for _ in range(m)]
    ty, a, b, _ = PS.pack(plans)
    want = restate(world, st, src, plans, 9 + np.arange(m), seed=31)
    assert sum(r.steps for r in want) > m
    assert_equal(run_typed(env, src, ty, a, b, rollout_base=9), expected(want), "max world, typed")
    amenu = agent_menu(254)
    aplans = [[amenu[j] for j in rng.integers(0, len(amenu), K)] for _ in range(m)]
    want = restate(world, st, src, aplans, 9 + np.arange(m), agent=True, seed=31)
    assert_equal(run_agent(env, src, np.array(aplans, np.int32).T.copy(), rollout_base=9), expected(want), "max world, agent")
    assert_untouched(env, before, "max world")
    env.close()


# ----------------------------------------------------------------- 9. capture
def test_captured_call_replays_to_the_eager_result():
    """The call makes one launch on the current stream and nothing else (no allocation, no
    synchronisation in the library), so torch.cuda.graph captures it; the replay equals the eager
    call and leaves the env alone."""
    env, world, st = table_env("open")
    before = snapshot(env)
    rng = np.random.default_rng(9)
    m, K = 257, 6
    src = torch.as_tensor(rng.integers(0, st.n, m).astype(np.int32), device=env.device)
    ty, a, b, _ = PS.pack(menu_plans(rng, m, K), K=K)
    dty, da, db = rows(env, ty), rows(env, a), rows(env, b)
    ids = torch.arange(m, dtype=torch.int64, device=env.device) + (1 << 36)
    eager = numpy_result(env.rollout_plan(src, dty, da, db, ids=ids, return_end=True))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            res = env.rollout_plan(src, dty, da, db, ids=ids, return_end=True)
    for f in FIELDS:  # capture launched nothing: poison the outputs so the replay has to write them
        getattr(res, f).fill_(-7)
    with torch.cuda.stream(side):
        g.replay()
    torch.cuda.synchronize()
    assert_equal(numpy_result(res), eager, "replay")
    assert_untouched(env, before, "capture")
    env.close()
