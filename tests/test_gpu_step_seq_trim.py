"""The state-only steps of a fused se_step_seq draw their FUEL and GATE blocks together (philox.h
draw2: the rounds the two blocks share computed once, the step-invariant parts before the loop),
carry the cell code under the ship from step to step instead of looking it up, and check a take
against a table of stocks by cell code built once per launch. What these can break is a draw
(a high quad word, a key's high word, a counter that wraps inside the run, the peel at the run's
end), a carried code that is stale when a later inner step depends on it, and a take check off a
port, at the stock's edge or against the wrong column.

Every scenario is stepped by a twin env through K VecEnv.step calls (recorded step by step), then
by one step_seq call, and compared exactly (fuel by its bits; the last step's reward, done and
err); 2 plain steps on both follow. The hand-built scenarios claim that a state-dependent action
runs in an inner step (k < K - 1) after the cell code changed, or should not have changed, in an
earlier inner step. Each claim is a list of (step, field, value) asserted on the recorded steps,
and the tests without the gpu mark assert the same claims on the C oracle."""
import numpy as np
import pytest

from step_seq_support import (AMOUNT, NO_DEST, NO_PORTS, NONE, NOT_AT_PORT, OK, OOB, TAIL, assert_same, device_rows,  # noqa: F401
                              empty_state, environ, gpu_lib, oracle_trace, run_fused, twin_trace)

gpu = pytest.mark.gpu

N_, E_, S_, W_ = 0, 1, 2, 3  # moves by (dx, dy): (0, -1), (-1, 0), (0, 1), (1, 0); x is the map row
K_SCN = 4  # rows 0 .. 2 run as state-only steps, row 3 in full


class World:
    """A 9 x 13 map (W != H, so a cell index with the sides swapped shows), water but for
    `ground`, with hand-placed ports and stocks."""

    H, W = 9, 13

    def __init__(self, ports, fuel, cargo, ground=()):
        self.water = np.ones((self.H, self.W), np.uint8)
        for x, y in ground:
            self.water[x, y] = 0
        self.ports = [list(p) for p in ports]
        self.fuel_stock, self.cargo_stock = list(fuel), list(cargo)
        self.P = len(self.ports)
        self.A = 4 + self.P + 250

    def env(self, n, seed=22, env_id_base=0, **env):
        from shippingenv_amd.vec import VecEnv

        with environ(**env):
            return VecEnv(n, water=self.water, ports=self.ports, port_fuel=self.fuel_stock,
                          port_cargo=self.cargo_stock, seed=seed, env_id_base=env_id_base)

    def oracle(self, O):
        return O.OracleWorld(self.water, [p[0] for p in self.ports], [p[1] for p in self.ports],
                             self.fuel_stock, self.cargo_stock)

    def cargo(self, v):
        return 4 + self.P + v

    def fuel(self, v):
        return 54 + self.P + v


# ports 0 .. 3: fuel and cargo stocks differ everywhere, port 1 is empty; (2, 1) is ground next
# to port 0, (4, 6) ground in open water, port 3 on the map's edge
SMALL = World(ports=[(2, 2), (2, 5), (6, 8), (0, 9)], fuel=[7, 0, 4, 5], cargo=[3, 0, 9, 6], ground=[(2, 1), (4, 6)])
# ports 0 and 1 on one cell: its code is port 0's, and an arrival at port 1 happens there
SHARED = World(ports=[(3, 3), (3, 3), (7, 10)], fuel=[5, 9, 4], cargo=[2, 8, 6])
ONE = World(ports=[(4, 4)], fuel=[6], cargo=[3])
NO_PORT = World(ports=[], fuel=[], cargo=[])
# 64 ports, port i at cell (1 + i // 11, 1 + i % 11): port 63 has the last code, 64
MANY = World(ports=[(1 + i // 11, 1 + i % 11) for i in range(64)], fuel=[1 + i % 9 for i in range(64)],
             cargo=[1 + (5 * i) % 7 for i in range(64)])
# the random runs: stocks large enough for drawn takes to pass now and then
GENERIC = World(ports=[(1, 2), (2, 10), (4, 4), (7, 1), (7, 11)], fuel=[150, 60, 199, 90, 30], cargo=[40, 10, 49, 25, 33],
                ground=[(0, 0), (3, 7), (4, 7), (5, 7), (8, 12), (6, 3)])
WORLDS = {"small": SMALL, "shared": SHARED, "one": ONE, "none": NO_PORT, "many": MANY, "generic": GENERIC}


def ship(cell, origin, dest, cargo=0, fuel=100.0):
    return dict(cell=cell, origin=origin, dest=dest, cargo=cargo, fuel=fuel)


def scenarios(name):
    """name -> [(label, initial ship, rows 0 .. K_SCN - 1, claims)]: a claim (k, field, value)
    holds after step k <= K_SCN - 2. Cargo is 0 wherever a claim reads it after a move (no gate)."""
    w = WORLDS[name]
    tc, tf = w.cargo, w.fuel
    if name == "small":
        return [
            # onto port 0, then cargo == stock, then stock + 1 (the fuel stock, 7, would let it pass)
            ("onto_port_take_cargo", ship((2, 3), 1, 2), [N_, tc(3), tc(4), 4 + 0],
             [(0, "pos", (2, 2)), (1, "err", OK), (1, "cargo", 3), (2, "err", AMOUNT), (2, "cargo", 3)]),
            # fuel == the fuel stock (7 > cargo stock 3), then fuel stock + 1
            ("onto_port_take_fuel", ship((2, 3), 1, 2), [N_, tf(7), tf(8), S_],
             [(0, "pos", (2, 2)), (1, "err", OK), (2, "err", AMOUNT)]),
            # off port 0, then a take on water, then back and a take
            ("off_port_take", ship((2, 2), 1, 2), [S_, tc(1), N_, tc(1)],
             [(0, "pos", (2, 3)), (1, "err", NOT_AT_PORT), (1, "cargo", 0), (2, "pos", (2, 2))]),
            ("off_and_back_take", ship((2, 2), 1, 2), [S_, N_, tf(2), tc(1)],
             [(0, "pos", (2, 3)), (1, "pos", (2, 2)), (2, "err", OK)]),
            # a move blocked by ground at (2, 1) leaves the ship on port 0, whose code it keeps
            ("blocked_then_take", ship((2, 2), 1, 2), [N_, tc(2), tf(7), S_],
             [(0, "pos", (2, 2)), (0, "err", OK), (1, "err", OK), (1, "cargo", 2), (2, "err", OK)]),
            # off the map from port 3 on the edge, then a take there
            ("oob_then_take", ship((0, 9), 0, 2), [E_, tf(5), tc(7), W_],
             [(0, "err", OOB), (0, "pos", (0, 9)), (1, "err", OK), (2, "err", AMOUNT)]),
            # no destination: the move is refused where it stands (cp == p), then a take
            ("nodest_then_take", ship((2, 2), 1, NONE), [S_, tc(1), tc(2), tc(1)],
             [(0, "err", NO_DEST), (0, "pos", (2, 2)), (1, "err", OK), (1, "cargo", 1), (2, "cargo", 3)]),
            # an arrival at port 2, then cargo == its stock
            ("arrive_then_take", ship((6, 9), 0, 2, cargo=10), [N_, tc(9), tf(4), tf(1)],
             [(0, "pos", (6, 8)), (0, "origin", 2), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 9), (2, "err", OK)]),
            # water to water, then takes on water
            ("take_on_water", ship((7, 3), 0, 2), [S_, tf(1), tc(1), N_],
             [(0, "pos", (7, 4)), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)]),
            # onto the empty port 1: both stocks are 0
            ("zero_stock_port", ship((2, 6), 0, 2), [N_, tc(1), tf(1), tc(1)],
             [(0, "pos", (2, 5)), (1, "err", AMOUNT), (2, "err", AMOUNT)]),
            # onto port 2 without arriving: fuel stock + 1, then the stock
            ("stock_plus_one", ship((6, 9), 1, 0), [N_, tf(5), tf(4), tc(10)],
             [(0, "pos", (6, 8)), (0, "origin", 1), (1, "err", AMOUNT), (2, "err", OK)]),
            # an index past the action space is TAKE_FUEL above every stock: at a port, on water
            ("past_space_at_port", ship((2, 3), 1, 2), [N_, w.A + 1, tc(0), tc(1)],
             [(0, "pos", (2, 2)), (1, "err", AMOUNT), (2, "err", AMOUNT)]),
            ("past_space_on_water", ship((2, 2), 1, 2), [S_, w.A, w.A + 2, N_],
             [(0, "pos", (2, 3)), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)]),
            # a ship loaded onto a ground cell (code 255): no port there
            ("on_ground_code", ship((4, 6), 0, 2), [4 + 1, tc(1), tf(1), tc(1)],
             [(0, "dest", 1), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)]),
            # a select between the move and the take changes no code
            ("move_select_take", ship((2, 3), 1, 2), [N_, 4 + 3, tc(3), tc(1)],
             [(0, "pos", (2, 2)), (1, "dest", 3), (2, "err", OK), (2, "cargo", 3)]),
        ]
    if name == "shared":
        return [
            # the shared cell answers with port 0's stocks (2 cargo, 5 fuel), not port 1's (8, 9)
            ("shared_take_cargo", ship((3, 4), 2, 2), [N_, tc(2), tc(3), tc(1)],
             [(0, "pos", (3, 3)), (1, "err", OK), (1, "cargo", 2), (2, "err", AMOUNT)]),
            ("shared_take_fuel", ship((3, 4), 2, 2), [N_, tf(5), tf(6), tc(1)],
             [(0, "pos", (3, 3)), (1, "err", OK), (2, "err", AMOUNT)]),
            # an arrival at port 1 (on port 0's cell), then takes against port 0's stocks
            ("shared_arrive_take", ship((4, 3), 2, 1, cargo=7), [E_, tc(2), tf(6), tc(1)],
             [(0, "pos", (3, 3)), (0, "origin", 1), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 2), (2, "err", AMOUNT)]),
            ("shared_leave_take", ship((3, 3), 2, 2), [S_, tc(1), N_, tc(1)],
             [(0, "pos", (3, 4)), (1, "err", NOT_AT_PORT), (2, "pos", (3, 3))]),
        ]
    if name == "one":
        return [
            # P = 1: code 1 is the only port code
            ("one_at_port", ship((4, 4), 0, NONE), [S_, tc(3), tf(6), tc(1)],
             [(0, "err", NO_DEST), (1, "err", OK), (1, "cargo", 3), (2, "err", OK)]),
            ("one_over_stock", ship((4, 4), 0, NONE), [tc(4), tf(7), tc(3), tc(1)],
             [(0, "err", AMOUNT), (1, "err", AMOUNT), (2, "err", OK), (2, "cargo", 3)]),
            ("one_on_water", ship((4, 5), 0, NONE), [N_, tc(1), tf(1), tc(1)],
             [(0, "err", NO_DEST), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)]),
        ]
    if name == "none":
        return [
            ("none_take", ship((4, 4), NONE, NONE), [S_, 4 + 1, 60, 300], [(0, "err", NO_PORTS), (1, "err", NO_PORTS), (2, "err", NO_PORTS)]),
            ("none_move", ship((0, 0), NONE, NONE), [E_, N_, 254, -1], [(0, "err", NO_PORTS), (0, "pos", (0, 0)), (2, "err", NO_PORTS)]),
        ]
    if name == "many":
        f, c = w.fuel_stock, w.cargo_stock
        p63, p62, p0 = tuple(w.ports[63]), tuple(w.ports[62]), tuple(w.ports[0])
        return [
            # onto port 63 (code 64, the last) from port 62 beside it
            ("last_port_cargo", ship(p62, 5, 7), [S_, tc(c[63]), tc(c[63] + 1), tc(1)],
             [(0, "pos", p63), (1, "err", OK), (1, "cargo", c[63]), (2, "err", AMOUNT)]),
            ("last_port_fuel", ship(p62, 5, 7), [S_, tf(f[63]), tf(f[63] + 1), tc(1)],
             [(0, "pos", p63), (1, "err", OK), (2, "err", AMOUNT)]),
            # off port 63 to the water beside it: code 0
            ("last_port_leave", ship(p63, 5, 7), [S_, tc(1), tf(1), N_],
             [(0, "pos", (p63[0], p63[1] + 1)), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)]),
            # from port 0 onto the water above it and back
            ("first_port_back", ship(p0, 5, 7), [N_, tc(1), S_, tc(1)],
             [(0, "pos", (p0[0], p0[1] - 1)), (1, "err", NOT_AT_PORT), (2, "pos", p0)]),
            ("first_port_stock", ship((p0[0], p0[1] - 1), 5, 7), [S_, tc(c[0]), tf(f[0] + 1), tc(1)],
             [(0, "pos", p0), (1, "err", OK), (1, "cargo", c[0]), (2, "err", AMOUNT)]),
        ]
    raise KeyError(name)


def scenario_size(name):
    """S + 3 full groups and a partial one of 3 envs (the tail kernel runs beside the fused one)."""
    return 4 * (len(scenarios(name)) + 3) + 3


def scenario_run(name):
    """Lane j of group g runs scenario (g + j) % S: with more than S groups every scenario meets
    every lane of a group. Rows past K_SCN (the plain steps) are moves."""
    scn = scenarios(name)
    S, n = len(scn), scenario_size(name)
    st = empty_state(n)
    acts = np.zeros((K_SCN + TAIL, n), np.int32)
    which = np.array([(i // 4 + i % 4) % S for i in range(n)])
    for i in range(n):
        _, sh, rows, _ = scn[which[i]]
        assert len(rows) == K_SCN
        st["x"][i], st["y"][i] = sh["cell"]
        st["origin"][i], st["dest"][i], st["cargo"][i] = sh["origin"], sh["dest"], sh["cargo"]
        st["fuel"][i] = sh["fuel"] + 0.125 * i
        acts[:K_SCN, i] = rows
        acts[K_SCN:, i] = i % 4
    return st, acts, which


def assert_claims(name, which, trace):
    scn = scenarios(name)
    for s, (label, _, _, claims) in enumerate(scn):
        envs = np.flatnonzero(which == s)
        assert {int(i) % 4 for i in envs} == {0, 1, 2, 3}, label
        for k, field, want in claims:
            assert k <= K_SCN - 2, f"{label}: a claim about the last step proves nothing about an inner one"
            if field == "pos":
                got = np.stack([trace[k]["x"][envs], trace[k]["y"][envs]], 1)
                assert (got == np.array(want)).all(), f"{label}: step {k} position {got[0]} != {want}"
            else:
                assert (trace[k][field][envs] == want).all(), f"{label}: step {k} {field} {trace[k][field][envs][0]} != {want}"


# ----------------------------------------------------------------- the hand-built scenarios
SCN_WORLDS = ("small", "shared", "one", "none", "many")


@pytest.mark.parametrize("name", SCN_WORLDS)
def test_scenarios_hold_what_they_claim_on_the_oracle(name, oracle_mod):
    init, acts, which = scenario_run(name)
    assert_claims(name, which, oracle_trace(oracle_mod, WORLDS[name], init, acts))


def test_worlds_are_what_the_scenarios_need():
    assert SHARED.ports[0] == SHARED.ports[1] and (SHARED.fuel_stock[0], SHARED.cargo_stock[0]) != (SHARED.fuel_stock[1], SHARED.cargo_stock[1])
    assert all(f != c for f, c in zip(SMALL.fuel_stock, SMALL.cargo_stock) if f or c) and (SMALL.fuel_stock[1], SMALL.cargo_stock[1]) == (0, 0)
    assert MANY.P == 64 and len({tuple(p) for p in MANY.ports}) == 64 and NO_PORT.P == 0 and ONE.P == 1
    assert all(0 <= x < World.H and 0 <= y < World.W for w in WORLDS.values() for x, y in w.ports)


@gpu
@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("name", SCN_WORLDS)
def test_scenario_fused_equals_step_calls(name, nt, gpu_lib, oracle_mod):
    """The twin's recorded steps hold the claims, equal the oracle's step by step, and the fused
    run ends where the twin does: as one launch and cut into launches of at most three steps."""
    world = WORLDS[name]
    init, acts, which = scenario_run(name)
    trace = twin_trace(world, init, acts)
    assert_claims(name, which, trace)
    for k, want in enumerate(oracle_trace(oracle_mod, world, init, acts)):
        assert_same(trace[k], want, f"{name}: twin vs oracle, step {k}")
    for env in ({}, {"SHIPENV_SEQ_MAX_STEPS": "3"}):
        b = world.env(len(init["x"]), SHIPENV_NT_LOADS=nt, **env)
        run_fused(b, init, device_rows(b, acts), trace, K_SCN, None, f"{name} nt={nt} {env}")
        b.close()


# ----------------------------------------------------------------- the draws
# (env_id_base, seed, first counter): a quad id with a high word, a key with a high word, a
# counter that wraps inside the run (at step 3, and at step 20 of the 33)
DRAWS = {
    "plain": (0, 22, 0),
    "high_quad": ((1 << 34) + 8, 22, 0),
    "high_key_wrap3": (0, (5 << 32) | 9, (1 << 32) - 3),
    "all_high_wrap20": ((1 << 36) + (1 << 34) + 4, (0xfedcba98 << 32) | 0x76543210, (1 << 32) - 20),
}
KS = (1, 2, 3, 4, 33)
N_GENERIC = 1031  # 257 full groups (the second workgroup has one live lane) and a tail of 3


def generic_run(world, n, rows):
    """Ships at ports and at sea with a destination, cargo 0 .. 59; the actions are drawn over
    the action space and a little beyond on both sides, half of them moves."""
    rng = np.random.default_rng(n + world.P)
    sea = [(x, y) for x in range(world.H) for y in range(world.W) if world.water[x, y] and [x, y] not in world.ports]
    st = empty_state(n)
    for i in range(n):
        o = int(rng.integers(world.P))
        st["origin"][i], st["dest"][i] = o, (o + 1 + i % (world.P - 1)) % world.P
        st["x"][i], st["y"][i] = world.ports[o] if i % 3 else sea[int(rng.integers(len(sea)))]
        st["fuel"][i] = 0.5 + 0.75 * (i % 64)
        st["cargo"][i] = i % 60
    acts = rng.integers(-6, world.A + 3, (rows, n)).astype(np.int32)
    moves = rng.integers(-4, 4, (rows, n)).astype(np.int32)
    return st, np.where(rng.random((rows, n)) < 0.5, moves, acts)


def assert_generic_coverage(init, acts, trace):
    """The random runs go through out of fuel, refusals, passed takes of both kinds, lost cargo
    and arrivals."""
    P = GENERIC.P
    prev = [init] + trace[:-1]
    took_c = took_f = lost = arrived = False
    for s0, a, s1 in zip(prev, acts, trace):
        ok = s1["err"] == OK
        took_c |= bool((ok & (a >= 4 + P) & (a < 54 + P) & (s1["cargo"] > s0["cargo"])).any())
        took_f |= bool((ok & (a >= 54 + P) & (s1["fuel"] > s0["fuel"])).any())
        mv = ok & (a >= -4) & (a < 4)
        lost |= bool((mv & (s1["origin"] == s0["origin"]) & (s1["cargo"] < s0["cargo"])).any())
        arrived |= bool((mv & (s1["origin"] != s0["origin"])).any())
    assert took_c and took_f and lost and arrived
    assert any((s["done"] == 1).any() for s in trace) and any((s["err"] != OK).any() for s in trace)


@pytest.mark.parametrize("draws", list(DRAWS))
def test_generic_run_on_the_oracle(draws, oracle_mod):
    base, seed, t0 = DRAWS[draws]
    init, acts = generic_run(GENERIC, N_GENERIC, max(KS) + TAIL)
    assert_generic_coverage(init, acts, oracle_trace(oracle_mod, GENERIC, init, acts, seed, base, t0))


_REF = {}


def generic_reference(draws):
    """The twin's 33 + TAIL recorded steps (read-only, shared by the cases of one draw set)."""
    if draws not in _REF:
        base, seed, t0 = DRAWS[draws]
        init, acts = generic_run(GENERIC, N_GENERIC, max(KS) + TAIL)
        _REF[draws] = (init, acts, twin_trace(GENERIC, init, acts, seed, base, t0))
    return _REF[draws]


@gpu
@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("draws", list(DRAWS))
def test_draws_and_peel_edges(draws, nt, gpu_lib, oracle_mod):
    """Runs of 1, 2, 3, 4 and 33 steps, whole and split at a mark, with the quad id, key and first
    counter of `draws`; the twin equals the oracle at the run's ends."""
    base, seed, t0 = DRAWS[draws]
    init, acts, trace = generic_reference(draws)
    assert_generic_coverage(init, acts, trace)
    want = oracle_trace(oracle_mod, GENERIC, init, acts, seed, base, t0)
    for k in (0, 3, max(KS) - 1, max(KS) + TAIL - 1):
        assert_same(trace[k], want[k], f"{draws}: twin vs oracle, step {k}")
    b = GENERIC.env(N_GENERIC, seed=seed, env_id_base=base, SHIPENV_NT_LOADS=nt)
    dev = device_rows(b, acts)
    for K in KS:
        for mark_after in [None] + sorted({1, K - 1} & set(range(1, K))):
            run_fused(b, init, dev, trace, K, mark_after, f"{draws} nt={nt}", t0)
    b.close()


@gpu
def test_one_workgroup_walks_several_groups(gpu_lib):
    """SHIPENV_STEP_BLOCKS=1: every thread steps several groups in turn, each with its own
    carried codes and draw invariants."""
    base, seed, t0 = DRAWS["all_high_wrap20"]
    init, acts, trace = generic_reference("all_high_wrap20")
    b = GENERIC.env(N_GENERIC, seed=seed, env_id_base=base, SHIPENV_STEP_BLOCKS="1")
    dev = device_rows(b, acts)
    for K in (2, 33):
        run_fused(b, init, dev, trace, K, None, "one workgroup", t0)
    b.close()
