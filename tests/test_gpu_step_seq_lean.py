"""The fused se_step_seq runs every step but a launch's last in a state-only mode
(step_group_state: no reward, no done, no err, the action's checks as one bit, x | y, origin
and dest carried unpacked) and only the last step in full. What could go wrong is the
state an inner step leaves behind and whose outputs a run stores, so every scenario here is
stepped by a twin env through K VecEnv.step calls (recorded step by step), then by one
step_seq call, and compared exactly, fuel by its bits; 2 plain steps on both follow, so a wrong
carried state shows even where the stored one looked right.

The hand-built scenarios claim to put particular events into the inner steps (k < K - 1): every
refusal, a blocked move, takes, selects, a firing gate, an arrival. Each claim is asserted on
the twin's recorded steps before anything is compared, and the same claims are asserted on the
C oracle in the tests without the gpu mark, so the scenarios (and the seed) are proven to hold
what they say on a machine without a GPU.

An agent index past the action space is no SE_ERR_BAD_INDEX in this project (nor in the
reference, whose decode only raises below -4): it decodes as TAKE_FUEL of an amount above every
stock, so it raises SE_ERR_AMOUNT at a port and SE_ERR_NOT_AT_PORT at sea. Both are covered."""
import numpy as np
import pytest

from conftest import golden_water
from step_seq_support import (AMOUNT, BAD_INDEX, NO_DEST, NO_PORTS, NONE, NOT_AT_PORT, OK, OOB, SAME_PORT, STATE, TAIL,  # noqa: F401
                              assert_same, device_rows, empty_state, environ, gpu_lib, oracle_trace, run_fused,
                              steps_before_last, twin_trace)

gpu = pytest.mark.gpu

SEED = 22
MOVES = ((0, -1), (-1, 0), (0, 1), (1, 0))  # N, E, S, W as (dx, dy)


class World:
    """The map, the ports and their stocks, with the cell lists the scenarios place ships on."""

    def __init__(self, n_ports):
        from shippingenv_amd.vec import DEFAULT_PORTS, draw_port_stocks, random_water_ports

        self.water = golden_water()
        self.H, self.W = self.water.shape
        if n_ports == 5:
            self.ports = [list(p) for p in DEFAULT_PORTS]
        else:
            self.ports = random_water_ports(self.water, n_ports, seed=3) if n_ports else []
        self.P = len(self.ports)
        self.A = 4 + self.P + 250  # the action space
        self.fuel_stock, self.cargo_stock = draw_port_stocks(self.P, SEED)
        ng = self.water.copy()
        for x, y in self.ports:
            ng[x, y] = 1
        self.nonground = ng
        port_cells = {(x, y) for x, y in self.ports}
        inside = lambda x, y: 0 <= x < self.H and 0 <= y < self.W  # noqa: E731
        free = lambda x, y: inside(x, y) and ng[x, y] and (x, y) not in port_cells  # noqa: E731
        # water, no port, all four neighbours water: every move from here moves
        self.open_sea = [(x, y) for x in range(1, self.H - 1) for y in range(1, self.W - 1)
                         if free(x, y) and all(free(x + dx, y + dy) for dx, dy in MOVES)]
        # (x, y, d): a free cell whose neighbour in direction d is ground
        self.shore = [(x, y, d) for x in range(self.H) for y in range(self.W) if free(x, y)
                      for d, (dx, dy) in enumerate(MOVES) if inside(x + dx, y + dy) and not ng[x + dx, y + dy]]
        # approach[p]: (d, cell one move before port p, cell two moves before), both free
        self.approach = {}
        for p, (px, py) in enumerate(self.ports):
            ways = [(d, (px - dx, py - dy), (px - 2 * dx, py - 2 * dy)) for d, (dx, dy) in enumerate(MOVES)
                    if free(px - dx, py - dy) and free(px - 2 * dx, py - 2 * dy)]
            if ways:
                self.approach[p] = ways
        # (x, y, d): an edge cell and the move that leaves the map from it
        self.edge = ([(0, y, 1) for y in range(0, self.W, 7)] + [(self.H - 1, y, 3) for y in range(0, self.W, 7)]
                     + [(x, 0, 0) for x in range(0, self.H, 7)] + [(x, self.W - 1, 2) for x in range(0, self.H, 7)])

    def env(self, n, seed=SEED, env_id_base=0, **env):
        from shippingenv_amd.vec import VecEnv

        with environ(**env):
            return VecEnv(n, water=self.water, ports=self.ports, port_fuel=self.fuel_stock,
                          port_cargo=self.cargo_stock, seed=seed, env_id_base=env_id_base)

    def oracle(self, O):
        px = [p[0] for p in self.ports]
        py = [p[1] for p in self.ports]
        return O.OracleWorld(self.water, px, py, self.fuel_stock, self.cargo_stock)


_WORLDS = {}


def world_of(n_ports):
    if n_ports not in _WORLDS:
        _WORLDS[n_ports] = World(n_ports)
    return _WORLDS[n_ports]


# ----------------------------------------------------------------- the fused run
def fused_matches_twin(world, init, acts, trace, K, mark_after=None, nt="1", **env):
    """One step_seq of rows 0 .. K-1 from init equals the twin after K steps, and after TAIL
    plain steps more."""
    b = world.env(len(init["x"]), SHIPENV_NT_LOADS=nt, **env)
    dev = device_rows(b, acts)
    run_fused(b, init, dev, trace, K, mark_after, f"K={K} nt={nt} {env}")
    b.close()


# ----------------------------------------------------------------- scenarios
def other_port(world, p, i):
    return (p + 1 + i % (world.P - 1)) % world.P


def generic_scenario(world, n, rows):
    """Ships at ports and at sea with fuel, cargo 0 .. 59 and a destination; the actions are
    drawn over the whole action space and a little beyond on both sides, half of them moves."""
    rng = np.random.default_rng(n + world.P)
    st = empty_state(n)
    for i in range(n):
        o = int(rng.integers(world.P))
        st["origin"][i], st["dest"][i] = o, other_port(world, o, i)
        cell = world.ports[o] if i % 3 else world.open_sea[int(rng.integers(len(world.open_sea)))]
        st["x"][i], st["y"][i] = cell
        st["fuel"][i] = 0.5 + 0.75 * (i % 64)  # some run out of fuel within the run
        st["cargo"][i] = i % 60
    acts = rng.integers(-6, world.A + 3, (rows, n)).astype(np.int32)
    moves = rng.integers(-4, 4, (rows, n)).astype(np.int32)
    return st, np.where(rng.random((rows, n)) < 0.5, moves, acts)


REFUSAL_CLASSES = 16


def refusal_scenario(world, n, K):
    """Env i takes the action of class (i + i // 16) % 16 (so every class meets every lane of
    a group) in rows 0 and 1, from a state made for it; later rows are drawn over the action
    space and beyond."""
    rng = np.random.default_rng(7)
    P, A = world.P, world.A
    st = empty_state(n)
    acts = rng.integers(-6, A + 3, (K + TAIL, n)).astype(np.int32)
    arrivals = sorted(world.approach)
    for i in range(n):
        c = (i + i // REFUSAL_CLASSES) % REFUSAL_CLASSES
        p = i % P  # the port the ship is at, where the class wants one
        o = (i // 3) % P
        sea = world.open_sea[(37 * i) % len(world.open_sea)]
        cell, origin, dest, cargo = sea, o, other_port(world, o, i), i % 40
        if c == 0:    # a plain move
            a = i % 4
        elif c == 1:  # a move given as -4 .. -1
            a = -4 + i % 4
        elif c == 2:  # below -4: BAD_INDEX
            a = -5 - i % 7
        elif c == 3:  # past the action space at a port: TAKE_FUEL above the stock, AMOUNT
            cell, a = world.ports[p], A + i % 3
        elif c == 4:  # past the action space at sea: NOT_AT_PORT
            a = A + i % 3
        elif c == 5:  # no destination
            dest, a = NONE, (i % 4 if i % 2 else -1 - i % 4)
        elif c == 6:  # off the map
            x, y, a = world.edge[i % len(world.edge)]
            cell = (x, y)
        elif c == 7:  # select the origin
            a = 4 + origin
        elif c == 8:  # a take at sea
            a = (4 + P + 1) if i % 2 else (54 + P + 1)
        elif c == 9:  # amount 0 at a port
            cell, a = world.ports[p], (4 + P) if i % 2 else (54 + P)
        elif c == 10:  # amount stock + 1 at a port
            cell = world.ports[p]
            a = (4 + P + world.cargo_stock[p] + 1) if i % 2 else (54 + P + world.fuel_stock[p] + 1)
        elif c == 11:  # a move onto ground
            x, y, a = world.shore[(11 * i) % len(world.shore)]
            cell = (x, y)
        elif c == 12:  # take cargo: 1 .. stock
            cell, a = world.ports[p], 4 + P + 1 + i % world.cargo_stock[p]
        elif c == 13:  # take fuel: 1 .. stock
            cell, a = world.ports[p], 54 + P + 1 + i % world.fuel_stock[p]
        elif c == 14:  # select another port
            a = 4 + other_port(world, origin, i // 5)
        else:          # arrive: one move before the destination port
            dest = arrivals[i % len(arrivals)]
            origin = other_port(world, dest, i)
            ways = world.approach[dest]
            a, cell, _ = ways[i % len(ways)]
            cargo = 10
        st["x"][i], st["y"][i] = cell
        st["origin"][i], st["dest"][i], st["cargo"][i] = origin, dest, cargo
        st["fuel"][i] = 100.0 + 0.25 * i
        acts[0, i] = acts[1, i] = a
    return st, acts


def assert_refusal_coverage(world, init, acts, trace, K):
    """Every class shows in the recorded inner steps."""
    P, A = world.P, world.A
    seen = dict.fromkeys(
        ["ok", "bad_low", "past_amount", "past_not_at_port", "no_dest", "oob", "same_port", "not_at_port",
         "amount_0", "amount_over", "neg_move", "blocked", "take_cargo", "take_fuel", "select", "arrival"], False)
    for _, s0, a, s1 in steps_before_last(init, acts, trace, K):
        err = s1["err"]
        mv = (a >= -4) & (a < 4)
        stayed = (s0["x"] == s1["x"]) & (s0["y"] == s1["y"])
        tc = (a >= 4 + P) & (a < 54 + P)
        tf = (a >= 54 + P) & (a < A)
        seen["ok"] |= bool((err == OK).any())
        seen["bad_low"] |= bool(((err == BAD_INDEX) & (a < -4)).any())
        seen["past_amount"] |= bool(((a >= A) & (err == AMOUNT)).any())
        seen["past_not_at_port"] |= bool(((a >= A) & (err == NOT_AT_PORT)).any())
        seen["no_dest"] |= bool(((err == NO_DEST) & mv).any())
        seen["oob"] |= bool(((err == OOB) & mv).any())
        seen["same_port"] |= bool(((err == SAME_PORT) & (a == 4 + s0["origin"])).any())
        seen["not_at_port"] |= bool(((err == NOT_AT_PORT) & (tc | tf)).any())
        seen["amount_0"] |= bool(((err == AMOUNT) & ((a == 4 + P) | (a == 54 + P))).any())
        seen["amount_over"] |= bool(((err == AMOUNT) & ((tc & (a > 4 + P)) | (tf & (a > 54 + P)))).any())
        seen["neg_move"] |= bool(((err == OK) & (a >= -4) & (a < 0) & ~stayed).any())
        seen["blocked"] |= bool(((err == OK) & mv & stayed).any())
        seen["take_cargo"] |= bool(((err == OK) & tc & (s1["cargo"] == s0["cargo"] + (a - 4 - P))).any())
        seen["take_fuel"] |= bool(((err == OK) & tf & (s1["fuel"] == s0["fuel"] + (a - 54 - P)) & (a > 54 + P)).any())
        seen["select"] |= bool(((err == OK) & (a >= 4) & (a < 4 + P) & (s1["dest"] == a - 4)).any())
        seen["arrival"] |= bool(((err == OK) & mv & (s1["origin"] != s0["origin"]) & (s1["origin"] == s0["dest"])).any())
        # a raised step changes nothing
        raised = err != OK
        for f in STATE:
            assert np.array_equal(s0[f][raised], s1[f][raised]), f
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the scenario no longer exercises {missing} in an inner step"


def last_outputs_scenario(world, n, K):
    """Fuel 0.5, so every move runs out of fuel (done 1, the out-of-fuel reward). By class
    (i + i // 4) % 4, rows K-2 / K-1 are: move / select, select / move, bad index / select,
    select / select of the origin. Earlier rows select; the plain steps after move."""
    st = empty_state(n)
    acts = np.zeros((K + TAIL, n), np.int32)
    for i in range(n):
        o = i % world.P
        q1, q2 = other_port(world, o, i), other_port(world, o, i + 1)
        st["x"][i], st["y"][i] = world.open_sea[(53 * i) % len(world.open_sea)]
        st["origin"][i], st["dest"][i], st["cargo"][i], st["fuel"][i] = o, q1, i % 7, 0.5
        acts[:, i] = 4 + q2
        acts[K:, i] = i % 4
        c = (i + i // 4) % 4
        acts[K - 2, i], acts[K - 1, i] = ((i % 4, 4 + q1), (4 + q1, i % 4), (-5, 4 + q1), (4 + q1, 4 + o))[c]
    return st, acts


def assert_last_outputs_coverage(init, acts, trace, K):
    n = len(init["x"])
    c = (np.arange(n) + np.arange(n) // 4) % 4
    p, s = trace[K - 2], trace[K - 1]  # the step before the last, the last
    assert ((p["done"] == 1) & (p["reward"] != 0) & (p["err"] == OK))[c == 0].all()
    assert ((s["done"] == 0) & (s["reward"] == 0) & (s["err"] == OK))[c == 0].all()
    assert ((p["done"] == 0) & (p["err"] == OK))[c == 1].all() and (s["done"] == 1)[c == 1].all()
    assert (p["err"] == BAD_INDEX)[c == 2].all() and (s["err"] == OK)[c == 2].all()
    assert (p["err"] == OK)[c == 3].all() and (s["err"] == SAME_PORT)[c == 3].all()
    assert all((c == k).any() for k in range(4))


def gate_scenario(world, n, K):
    """Movers with cargo 49 one move (even quads) or two moves (odd quads) before their
    destination port, heading for it in rows 0 and 1; later rows are moves."""
    rng = np.random.default_rng(11)
    st = empty_state(n)
    acts = rng.integers(-4, 4, (K + TAIL, n)).astype(np.int32)
    ports = sorted(world.approach)
    for i in range(n):
        dest = ports[i % len(ports)]
        ways = world.approach[dest]
        d, c1, c2 = ways[(i // len(ports)) % len(ways)]
        st["x"][i], st["y"][i] = c2 if (i // 4) % 2 else c1
        st["origin"][i], st["dest"][i] = other_port(world, dest, i), dest
        st["cargo"][i], st["fuel"][i] = 49, 150.0 + i
        acts[0, i] = acts[1, i] = d
    return st, acts


def assert_gate_coverage(init, acts, trace, K):
    lost = arrived = False
    for _, s0, a, s1 in steps_before_last(init, acts, trace, K):
        moved = (s1["err"] == OK) & (a < 4) & (a >= -4)
        same_trip = s1["origin"] == s0["origin"]
        lost |= bool((moved & same_trip & (s1["cargo"] < s0["cargo"]) & (s0["cargo"] == 49)).any())
        arrived |= bool((moved & ~same_trip & (s1["cargo"] == 0)).any())
    assert lost, "no gate fired and cost cargo in an inner step"
    assert arrived, "no ship arrived in an inner step"


def no_ports_scenario(world, n, K):
    st = empty_state(n)
    for i in range(n):
        st["x"][i], st["y"][i] = world.open_sea[(5 * i) % len(world.open_sea)]
        st["fuel"][i], st["cargo"][i] = 20.0 + i, i
    acts = np.array([[(-6, -1, 0, 3, 4, 30, 60, 254, 300)[(i + k) % 9] for i in range(n)]
                     for k in range(K + TAIL)], np.int32)
    return st, acts


def assert_no_ports_coverage(init, acts, trace, K):
    for _, s0, a, s1 in steps_before_last(init, acts, trace, K):
        assert np.array_equal(s1["err"], np.where(a < -4, BAD_INDEX, NO_PORTS))
        for f in STATE:
            assert np.array_equal(s0[f], s1[f]), f
    assert K >= 2


SCENARIOS = {
    # name: (builder, coverage check, ports of the worlds it runs on, n, K)
    "refusals": (refusal_scenario, lambda w, *a: assert_refusal_coverage(w, *a), (5, 64), 1028, 4),
    "last_outputs_K2": (last_outputs_scenario, lambda w, *a: assert_last_outputs_coverage(*a), (5,), 1028, 2),
    "last_outputs_K3": (last_outputs_scenario, lambda w, *a: assert_last_outputs_coverage(*a), (5, 64), 1028, 3),
    "gate_arrival": (gate_scenario, lambda w, *a: assert_gate_coverage(*a), (5, 64), 1028, 4),
    "no_ports": (no_ports_scenario, lambda w, *a: assert_no_ports_coverage(*a), (0,), 7, 3),
}
SCENARIO_IDS = [(name, P) for name, v in SCENARIOS.items() for P in v[2]]


# ----------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name,P", SCENARIO_IDS)
def test_scenarios_hold_what_they_claim_on_the_oracle(name, P, oracle_mod):
    build, check, _, n, K = SCENARIOS[name]
    world = world_of(P)
    init, acts = build(world, n, K)
    check(world, init, acts, oracle_trace(oracle_mod, world, init, acts), K)


def assert_generic_coverage(trace):
    """The peel-edge runs go through out of fuel, refusals, cargo changes and arrivals."""
    assert any((s["done"] == 1).any() for s in trace) and any((s["err"] != OK).any() for s in trace)
    assert any((a["cargo"] != b["cargo"]).any() for a, b in zip(trace, trace[1:]))


@pytest.mark.parametrize("P", [5, 64])
@pytest.mark.parametrize("size", ["n7", "n1028", "n2052_one_block"])
def test_generic_scenario_on_the_oracle(size, P, oracle_mod):
    world = world_of(P)
    init, acts = generic_scenario(world, SIZES[size][0], max(KS) + TAIL)
    assert_generic_coverage(oracle_trace(oracle_mod, world, init, acts))


# ----------------------------------------------------------------- on the GPU
@gpu
@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("name,P", SCENARIO_IDS)
def test_scenario_fused_equals_step_calls(name, P, nt, gpu_lib, oracle_mod):
    """The twin's recorded steps hold the scenario's events in inner steps (asserted), equal the
    oracle's step by step, and the fused run ends where the twin does: as one launch, and cut
    into launches of one state-only step plus the full one (SHIPENV_SEQ_MAX_STEPS=2)."""
    build, check, _, n, K = SCENARIOS[name]
    world = world_of(P)
    init, acts = build(world, n, K)
    trace = twin_trace(world, init, acts)
    check(world, init, acts, trace, K)
    for k, want in enumerate(oracle_trace(oracle_mod, world, init, acts)):
        assert_same(trace[k], want, f"twin vs oracle, step {k}")
    fused_matches_twin(world, init, acts, trace, K, nt=nt)
    fused_matches_twin(world, init, acts, trace, K, nt=nt, SHIPENV_SEQ_MAX_STEPS="2")


# n: one group plus a tail of 3; 257 groups, so the second workgroup has one live lane; 513
# groups in one workgroup, 3 groups per thread
SIZES = {"n7": (7, {}), "n1028": (1028, {}), "n2052_one_block": (2052, {"SHIPENV_STEP_BLOCKS": "1"})}
KS = (1, 2, 3, 9)
_PEEL = {}


def peel_reference(size, P):
    """The twin's 9 + TAIL recorded steps of the generic scenario (read-only, shared)."""
    if (size, P) not in _PEEL:
        world = world_of(P)
        init, acts = generic_scenario(world, SIZES[size][0], max(KS) + TAIL)
        _PEEL[size, P] = (init, acts, twin_trace(world, init, acts))
    return _PEEL[size, P]


@gpu
@pytest.mark.parametrize("max_steps", [None, "1", "2"])
@pytest.mark.parametrize("nt", ["1", "0"])
@pytest.mark.parametrize("P", [5, 64])
@pytest.mark.parametrize("size", list(SIZES))
def test_peel_edges(size, P, nt, max_steps, gpu_lib):
    """K in {1, 2, 3, 9} x mark_after in {none, 0, 1, K-1, K}: a launch of the full step alone,
    one state-only step before it, several; SHIPENV_SEQ_MAX_STEPS 1 makes every launch the
    full step alone, 2 one state-only step plus the full one."""
    init, acts, trace = peel_reference(size, P)
    world = world_of(P)
    env = dict(SIZES[size][1], SHIPENV_SEQ_MAX_STEPS=max_steps)
    b = world.env(len(init["x"]), SHIPENV_NT_LOADS=nt, **env)
    dev = device_rows(b, acts)
    assert_generic_coverage(trace)
    for K in KS:
        for mark_after in [None] + sorted({0, 1, K - 1, K}):
            run_fused(b, init, dev, trace, K, mark_after, f"{size} P={P} nt={nt} max_steps={max_steps} K={K}")
    b.close()
