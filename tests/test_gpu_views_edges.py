"""The view kernels of csrc/views.h (observe, valid_mask, gen_actions) at their edges.

(a) every record of tests/golden/views_edges.npz (the reference's own preprocess_state rows and
    is_valid_action bits, tests/golden/make_views_golden.py) through every kernel;
(b)-(f) tile, stride, template-count and handle edges against the C oracle, which
    test_views_edges_cpu.py pins to the same records.

Every output is carved from a larger buffer prefilled with a sentinel byte, at least 64 bytes
either side, and the margins (and the gap columns of a strided output) must still hold the
sentinel after the call. Which kernel a call takes follows from its arguments (se_observe,
se_valid_mask): a dense 16-byte aligned output the tiled / template kernels, any other stride
or alignment the generic ones, SHIPENV_MASK_TILED=1 (read when the env is made) or more than
kMaskTmplMax templates the tiled mask kernel.
"""
import numpy as np
import pytest

import views_edge_support as V
from test_gpu_parity import _oracle_pair
from test_gpu_rollout import load_state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT, MARGIN = 0xA5, 64
K_MASK_TMPL_MAX = 320  # csrc/views.h kMaskTmplMax
STOCK_EDGES = np.array([0, 1, 49, 50, 199, 200, 250])
FUEL_EDGES = np.array(V.FUELS)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from shippingenv_amd import build

    build.build(verbose=False)


def VecEnv(*a, **k):
    from shippingenv_amd.vec import VecEnv as E

    return E(*a, **k)


def env_of(world, n, **kw):
    water, px, py, pf, pc = world
    return VecEnv(n, water=water, ports=[[int(a), int(b)] for a, b in zip(px, py)], port_fuel=pf, port_cargo=pc, **kw)


# ---------------------------------------------------------------- sentinel-guarded outputs
class Carved:
    """nbytes of output at `offset` bytes past a 16-byte boundary, inside a sentinel-filled block."""

    def __init__(self, dev, nbytes, offset=0):
        self.raw = torch.full((MARGIN + offset + nbytes + MARGIN,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi = MARGIN + offset, MARGIN + offset + nbytes
        self.out = self.raw[self.lo:self.hi]
        assert (self.out.data_ptr() % 16 == 0) == (offset % 16 == 0)

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[:self.lo] == SENT).all()), f"{what}: bytes before the output were written"
        assert bool((self.raw[self.hi:] == SENT).all()), f"{what}: bytes after the output were written"


def observe_into(env, ld, offset, what):
    """env.observe into a guarded [n, ld] f32 output -> the device tensor of its first obs_size columns."""
    n, W = env.n, env.obs_size
    c = Carved(env.device, n * ld * 4, offset)
    out = c.out.view(torch.float32).view(n, ld)
    env.observe(out)
    c.check(what)
    if ld > W:
        assert bool((out[:, W:].contiguous().view(torch.uint8) == SENT).all()), f"{what}: gap columns were written"
    return out[:, :W]


def mask_into(env, offset, what):
    n, S = env.n, (env.action_space_size + 7) // 8
    c = Carved(env.device, n * S, offset)
    out = c.out.view(n, S)
    env.valid_mask(out)
    c.check(what)
    return out


def rows_equal(got, want, what):
    """V.assert_rows_equal of a device tensor; equal bits are settled on the device (the large cases)."""
    w = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    if got.is_contiguous() and torch.equal(got.view(torch.int32), w.view(torch.int32)):
        return
    V.assert_rows_equal(got.cpu().numpy(), want, what)


def bits_equal(got, want, what):
    w = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    if not torch.equal(got, w):
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)


def check_env(env, want_obs, want_bits, what, generic=True):
    """The calls one env serves: observe tiled, strided and offset; valid_mask aligned and offset."""
    W = env.obs_size
    assert want_obs.shape == (env.n, W) and want_bits.shape == (env.n, (4 + env.P + 250 + 7) // 8)
    rows_equal(observe_into(env, W, 0, f"{what}: observe tiled"), want_obs, f"{what}: observe tiled")
    bits_equal(mask_into(env, 0, f"{what}: mask aligned"), want_bits, f"{what}: mask aligned")
    if generic:
        rows_equal(observe_into(env, W + 2, 0, f"{what}: observe ld=W+2"), want_obs, f"{what}: observe ld=W+2")
        rows_equal(observe_into(env, W, 4, f"{what}: observe +4 bytes"), want_obs, f"{what}: observe +4 bytes")
        bits_equal(mask_into(env, 1, f"{what}: mask +1 byte"), want_bits, f"{what}: mask +1 byte")


def check_world(monkeypatch, world, st, want_obs, want_bits, what, generic=True, **kw):
    """All six calls of the issue on one world and batch: check_env, then valid_mask aligned on an
    env made under SHIPENV_MASK_TILED=1."""
    env = env_of(world, st.n, **kw)
    load_state(env, st)
    check_env(env, want_obs, want_bits, what, generic)
    env.close()
    with monkeypatch.context() as m:
        m.setenv("SHIPENV_MASK_TILED", "1")
        env = env_of(world, st.n, **kw)
    load_state(env, st)
    bits_equal(mask_into(env, 0, f"{what}: mask tiled"), want_bits, f"{what}: mask tiled")
    env.close()


# ---------------------------------------------------------------- random worlds and placements
def draw_stocks(rng, P):
    """Half from the amount rows' edges (the first port always), half from add_port's 5..20."""
    edge = rng.random(P) < 0.5
    edge[0] = True
    return np.where(edge, rng.choice(STOCK_EDGES, P), rng.integers(5, 21, P)).astype(np.int32)


def world_of_cells(water, counts, rng):
    """A world with counts[j] ports on the j-th of len(counts) distinct water cells, port order
    shuffled, stocks from draw_stocks."""
    cells = np.argwhere(water != 0)
    pick = cells[rng.choice(len(cells), len(counts), replace=False)]
    ports = np.repeat(pick, counts, axis=0)
    ports = ports[rng.permutation(len(ports))]
    P = len(ports)
    return (water, ports[:, 0].astype(np.int32), ports[:, 1].astype(np.int32), draw_stocks(rng, P), draw_stocks(rng, P))


def edge_world(P, water, rng):
    """P ports with some repeated cells; P = 254 on a 256 x 256 random map (14 cells of two)."""
    if P == 254:
        water = (rng.random((256, 256)) < 0.6).astype(np.uint8)
    rep = {1: 0, 2: 0, 3: 1, 64: 6, 65: 5, 254: 14}[P]
    return world_of_cells(water, [2] * rep + [1] * (P - 2 * rep), rng)


def place(O, world, n, rng, first=None):
    """An OracleState of n ships placed as test_valid_mask_row_templates does: mostly on port cells;
    the origin is the port itself, a cell-mate, any port, or none. `first` = (port, origin) arrays
    to put at the head of the batch."""
    water, px, py, _, _ = world
    P = len(px)
    k = rng.integers(0, P, n)
    cells = np.argwhere(water != 0)
    sea = cells[rng.integers(0, len(cells), n)]
    at_port = rng.random(n) < 0.85
    pos = px.astype(np.int64) * 65536 + py
    same = pos[:, None] == pos[None, :]
    mates = np.argsort(~same, axis=1, kind="stable")  # row p: the ports of p's cell first
    alt = mates[k, rng.integers(0, 1 << 30, n) % same.sum(axis=1)[k]]
    u = rng.random(n)
    origin = np.where(u < 0.4, k, np.where(u < 0.7, alt, np.where(u < 0.9, rng.integers(0, P, n), -1)))
    if first is not None:
        m = min(n, len(first[0]))
        k[:m], origin[:m], at_port[:m] = first[0][:m], first[1][:m], True
    st = O.OracleState(n)
    st.x[:] = np.where(at_port, px[k], sea[:, 0])
    st.y[:] = np.where(at_port, py[k], sea[:, 1])
    st.origin[:] = origin
    st.dest[:] = np.where(rng.random(n) < 0.2, -1, rng.integers(0, P, n))
    st.fuel[:] = np.where(rng.random(n) < 0.3, rng.choice(FUEL_EDGES, n), rng.random(n) * 120.0)
    st.cargo[:] = rng.integers(0, 51, n)
    return st


def oracle_views(O, world, st):
    ow = O.OracleWorld(*world)
    return O.observe(ow, st), O.valid_mask(ow, st)


# ---------------------------------------------------------------- (a) the fixture through every kernel
@pytest.mark.parametrize("name", V.worlds())
def test_fixture_through_every_kernel(oracle_mod, monkeypatch, name):
    """The reference's rows and bits, exactly (a NaN need only be a NaN), from the tiled, strided
    and offset observe kernels and the template, tiled and generic mask kernels."""
    sel = V.ragged(len(V.states(name)["x"]))
    assert len(sel) % 256
    st = V.oracle_state(oracle_mod, V.states(name, sel))
    check_world(monkeypatch, V.world(name), st, V.want_obs(name, sel), V.want_bits(name, sel), name)


# ---------------------------------------------------------------- (b) tile and stride edges
@pytest.mark.parametrize("P", [1, 2, 3, 64, 65, 254])
def test_tile_and_stride_edges_vs_oracle(oracle_mod, water, monkeypatch, P):
    """n below, on and past one tile and two; row strides S = 32, 32, 33 (P = 1, 2, 3) and 64
    (P = 254, W = 1022: the widest row the tiled observe kernel takes); P = 65 past the 64-bit
    same-cell masks. Stocks sit on the amount rows' edges."""
    O = oracle_mod
    rng = np.random.default_rng(1000 + P)
    world = edge_world(P, water, rng)
    assert len(world[1]) == P and set(world[3].tolist() + world[4].tolist()) & set(STOCK_EDGES.tolist())
    if P <= 64:
        assert V.ntmpl(world[1], world[2]) <= K_MASK_TMPL_MAX  # the template kernel serves the aligned call
    W = 6 + 4 * P
    assert W <= 1022
    tails = set()
    for n in (1, 2, 255, 256, 257, 513):
        tails.add((((n - 1) % 256 + 1) * W) % 4 == 2)  # the last tile's float count leaves a 2-float run
        st = place(O, world, n, rng)
        want_obs, want_bits = oracle_views(O, world, st)
        check_world(monkeypatch, world, st, want_obs, want_bits, f"P={P} n={n}")
    assert tails == {True, False}


# ---------------------------------------------------------------- (c) the template-count switch
@pytest.mark.parametrize("counts,ntmpl", [
    ([13] + [2] * 17 + [1] * 17, 319),            # the most templates the LDS kernel takes
    ([13, 3] + [2] * 15 + [1] * 18, 321),         # the fewest that go to the tiled kernel
    ([64], 4161),                                 # every port on one cell
], ids=["319", "321", "4161"])
def test_template_count_switch(oracle_mod, water, monkeypatch, counts, ntmpl):
    O = oracle_mod
    assert sum(counts) == 64 and 1 + 64 + sum(k * k for k in counts) == ntmpl
    assert (ntmpl <= K_MASK_TMPL_MAX) == (ntmpl == 319)
    rng = np.random.default_rng(ntmpl)
    world = world_of_cells(water, counts, rng)
    _, px, py, _, _ = world
    assert V.ntmpl(px, py) == ntmpl
    crowd = np.nonzero((px == px[0]) & (py == py[0]))[0] if counts == [64] else None
    if crowd is None:
        pos = px.astype(np.int64) * 65536 + py
        vals, cnt = np.unique(pos, return_counts=True)
        crowd = np.nonzero(pos == vals[cnt.argmax()])[0]
    assert len(crowd) == counts[0]
    assert len(crowd) == 64 or (np.diff(crowd) > 1).any()  # the cell's ports are scattered over the indices
    # every origin on the crowded cell, and None, from its first port's cell; then from each of its ports
    origins = np.concatenate([crowd, [-1], crowd])
    ports = np.concatenate([np.full(len(crowd) + 1, crowd[-1]), crowd])
    n = 3 * 256 + 77
    st = place(O, world, n, rng, first=(ports, origins))
    on = (st.x == px[crowd[0]]) & (st.y == py[crowd[0]])
    assert set(st.origin[on].tolist()) >= set(crowd.tolist()) | {-1}
    want_obs, want_bits = oracle_views(O, world, st)
    check_world(monkeypatch, world, st, want_obs, want_bits, f"ntmpl={ntmpl}")


# ---------------------------------------------------------------- (d) a workgroup's second tile
@pytest.mark.parametrize("P", [5, 64])
def test_second_tile_of_a_workgroup(oracle_mod, water, monkeypatch, P):
    """The grid-stride loop of the tiled kernels and of the template kernel runs a second tile once n
    passes (blocks x 256) rows: 2048 blocks, or 1024 for the template kernel when its templates
    exceed 4 KB of LDS (P = 64 on distinct cells: 129 blocks of mask_tb(40) = 80 bytes). n is one
    tile and a ragged one past that, and every row is compared."""
    from shippingenv_amd.vec import random_water_ports

    O = oracle_mod
    rng = np.random.default_rng(2000 + P)
    if P == 5:
        env0 = VecEnv(1)  # the default world
        world = (env0.water, env0.port_x, env0.port_y, env0.port_fuel, env0.port_cargo)
        env0.close()
        blocks = 2048
    else:
        cells = np.array(random_water_ports(water, 64, seed=4), np.int32)
        world = (water, cells[:, 0].copy(), cells[:, 1].copy(), draw_stocks(rng, P), draw_stocks(rng, P))
        blocks = 1024
    S = (4 + P + 250 + 7) // 8
    nt = V.ntmpl(world[1], world[2])
    assert nt == 1 + 2 * P
    assert (nt * V.mask_tb(S) > 4096) == (P == 64) and (P != 64 or 129 * V.mask_tb(S) > 4096)
    n = blocks * 256 + 256 + 77
    st = place(O, world, n, rng)
    want_obs, want_bits = oracle_views(O, world, st)
    check_world(monkeypatch, world, st, want_obs, want_bits, f"P={P} n={n}", generic=False)


# ---------------------------------------------------------------- (e) a world that changes under the handle
def test_views_follow_set_ports(oracle_mod, water):
    """set_ports from 5 ports to 64, to 1 and to 5 again on one env: the template buffer grows,
    is rebuilt in place for fewer templates, and obs_size, the mask stride and both outputs
    follow the oracle each time."""
    O = oracle_mod
    rng = np.random.default_rng(31)
    n = 256 + 77
    env = VecEnv(n, seed=8)
    first = (env.water, env.port_x, env.port_y, env.port_fuel, env.port_cargo)
    seq = [first, edge_world(64, water, rng), edge_world(1, water, rng), first]
    for step, world in enumerate(seq):
        _, px, py, pf, pc = world
        P = len(px)
        if step:
            env.set_ports([[int(a), int(b)] for a, b in zip(px, py)], pf, pc)
        assert env.P == P and env.obs_size == 6 + 4 * P
        assert env.valid_mask().shape == (n, (4 + P + 250 + 7) // 8)
        st = place(O, world, n, rng)
        load_state(env, st)
        ow, st2 = _oracle_pair(O, env)  # the world as the env itself reports it
        for f in V.STATE:
            getattr(st2, f)[:] = getattr(st, f)
        check_env(env, O.observe(ow, st2), O.valid_mask(ow, st2), f"set_ports step {step} P={P}")
    env.close()


# ---------------------------------------------------------------- (f) the synthetic agent
def test_env_id_base_off_a_multiple_of_4_is_refused(water):
    """Why test_gen_actions_edges reaches the ids from 2^32 - 130 through an env based at 2^32 - 132:
    se_create takes a base only on a multiple of 4 (envs 4k..4k+3 share draw blocks)."""
    from shippingenv_amd._native import ShipEnvError

    world = edge_world(1, water, np.random.default_rng(3001))
    for base in (2 ** 32 - 130, 2 ** 32 - 131, 1):
        with pytest.raises(ShipEnvError, match="multiple of 4"):
            env_of(world, 1, seed=77, env_id_base=base)
    env_of(world, 1, seed=77, env_id_base=2 ** 32 - 132).close()


@pytest.mark.parametrize("P", [1, 254])
@pytest.mark.parametrize("n", [1, 257])
def test_gen_actions_edges(oracle_mod, water, P, n):
    """t = 0 and 2^32 - 1, env ids that carry past 2^32 inside the batch, P = 1 (every SELECT draw
    is action 4) and P = 254. se_create takes an env_id_base only on a multiple of 4 (envs 4k..4k+3
    share draw blocks), so the ids 2^32 - 130 .. of the oracle's batch are rows 2.. of an env of
    n + 2 based at 2^32 - 132; an env of exactly n envs on that base is compared as well."""
    O = oracle_mod
    seed, base = 77, 2 ** 32 - 130
    world = edge_world(P, water, np.random.default_rng(3000 + P))
    kinds = set()
    for lead in (2, 0):
        env = env_of(world, n + lead, seed=seed, env_id_base=base - 2)
        for t in (0, 2 ** 32 - 1):
            want = O.gen_actions(n, P, seed, base - 2 + lead, t)
            c = Carved(env.device, 4 * (n + lead))
            out = c.out.view(torch.int32)
            env.gen_actions(t, out)
            c.check(f"gen_actions P={P} n={n} t={t}")
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got[lead:], want, err_msg=f"P={P} n={n} t={t} lead={lead}")
            if lead:
                np.testing.assert_array_equal(got, O.gen_actions(n + lead, P, seed, base - 2, t))
            assert ((want >= 0) & (want < 4 + P + 250)).all()
            select = (want >= 4) & (want < 4 + P)
            if P == 1:
                assert (want[select] == 4).all()
            kinds |= {"move"} if (want < 4).any() else set()
            kinds |= {"select"} if select.any() else set()
            kinds |= {"take"} if (want >= 4 + P).any() else set()
        env.close()
    if n == 257:
        assert kinds == {"move", "select", "take"}
