"""The state-only step of a fused se_step_seq carries each env's gate threshold from step to step
and looks it up again only where the cargo changes (a passed take, a loss, an arrival), decodes the
action by two unsigned range compares and updates the fuel with one FMA (step_seq.h, step_lean.h).

What can go wrong: a threshold that is stale after one of the three changes, or filled from the
wrong cargo or without the clamp when a group is loaded; an action at a range's end, or at an int32
end, decoded as another kind; a world without ports that moves a ship; fuel bits at the values where
a fused multiply-add could round otherwise.

A stale threshold shows only when the gate's outcome under the stale cargo differs from the outcome
under the right one. So the CPU companion counts, on the C oracle alone, the discriminating gate
tests of the cargo run: a test by a moving carrier in an inner step after its cargo changed in an
earlier inner step, whose GATE word lies between gate_thr(cargo before the change) and
gate_thr(cargo now). It asserts at least 16 of them for every kind of change in every kind of wave:
waves that pool with windows of 8 and of 4, and waves that draw directly (more than 16 carrier
lanes, and the wave with lanes past the last full group). SHIPENV_SEQ_GATE_POOL=0 runs the same
inputs with every wave direct. For the loaded values no change precedes the test: a cargo of 50 and
above counts when its word is above gate_thr(49), the nearest entry a wrong clamp would read, and
a cargo of 0 or below counts always (no entry is right: only the kept `cargo > 0` stops it).

The method is test_gpu_step_seq_gatepool's: a twin env stepped by K VecEnv.step calls (equal to the
oracle step by step) is the reference, one step_seq call must end in the same bits, and 2 plain
steps follow."""
import collections

import numpy as np
import pytest

from step_seq_support import (AMOUNT, BAD_INDEX, NO_DEST, NO_PORTS, NONE, NOT_AT_PORT, OK, OOB, SAME_PORT, TAIL, assert_same,  # noqa: F401
                              device_rows, empty_state, gpu_lib, oracle_trace, run_fused, twin_trace)
from test_gpu_step_seq_gatepool import (LANES, POOLW, SEED, WAVE, gate_thr, gate_word, ids_of, launches_of, sea_run, windows)
from test_gpu_step_seq_trim import E_, N_, S_, W_, World

gpu = pytest.mark.gpu
_REF = {}


def reference(name, world, make, seed=SEED):
    """The twin's recorded steps of a run (read-only, shared by the cases)."""
    if name not in _REF:
        init, acts = make()
        _REF[name] = (init, acts, twin_trace(world, init, acts, seed))
    return _REF[name]


# ----------------------------------------------------------------- the cargo run
K_CARGO = 32
KINDS = ("take", "loss", "arrive_take", "raise50", "loaded50", "nonpos")
# (waves, actor lanes of each): carrier lanes stay at 8 or below, between 9 and 16, above 16
CLASSES = ((8, [0, 63, 5, 17, 30, 47]), (5, list(range(1, 64, 4))), (2, list(range(40))))
PART_LANES = 20  # the last wave: 20 lanes, all actors, then a tail of 3 envs
N_CARGO = sum(w for w, _ in CLASSES) * WAVE + 4 * PART_LANES + 3
K_TAKE = 2  # every take of the run is in row 2: one window cut per wave
PORT0, BESIDE = tuple(POOLW.ports[0]), (3, 2)  # W_ from port 0 is (3, 2), then (4, 2): water


def cargo_run():
    """Sea ships that shuttle (test_gpu_step_seq_gatepool.sea_run); the actor lanes hold four envs
    of one kind each:
      take         on port 0 with no cargo: takes 10 .. 49 in row 2, then moves off and shuttles;
      loss         at sea with 30 .. 49: every fired gate with a partial loss lowers the cargo;
      arrive_take  beside port 0, its destination, with 20: arrives in row 0 (cargo 0), takes 10 .. 49
                   in row 2, moves off and shuttles;
      raise50      on port 0 with 5 .. 24: takes 49 in row 2 (54 .. 73), moves off and shuttles;
      loaded50     at sea with 50, 51, 55, 59;
      nonpos       at sea with 0, -1, -7, -50."""
    rows = K_CARGO + TAIL
    st, acts = sea_run(N_CARGO, rows)
    kinds = {}
    lanes, wave = [], 0
    for waves, actor in CLASSES:
        for _ in range(waves):
            lanes += [wave * LANES + l for l in actor]
            wave += 1
    lanes += [wave * LANES + l for l in range(PART_LANES)]
    shuttle = [W_, W_] + [E_ if k % 2 == 0 else W_ for k in range(rows)]
    for q, lane in enumerate(lanes):
        kind = KINDS[q % len(KINDS)]
        for j in range(4):
            i, v = 4 * lane + j, 4 * q + j
            kinds[i] = kind
            if kind in ("take", "raise50", "arrive_take"):
                st["origin"][i], st["dest"][i] = 1, 2
                st["x"][i], st["y"][i] = PORT0
                st["cargo"][i] = 0 if kind == "take" else 5 + v % 20
                acts[:K_TAKE, i] = [4 + 3, 4 + 2]
                acts[K_TAKE, i] = POOLW.cargo(49 if kind == "raise50" else 10 + (7 * v) % 40)
                acts[K_TAKE + 1:, i] = shuttle[:rows - K_TAKE - 1]
                if kind == "arrive_take":
                    st["x"][i], st["y"][i] = BESIDE
                    st["dest"][i], st["cargo"][i] = 0, 20
                    acts[0, i] = E_
            elif kind == "loss":
                st["cargo"][i] = 30 + v % 20
            elif kind == "loaded50":
                st["cargo"][i] = (50, 51, 55, 59)[j]
            else:
                st["cargo"][i] = (0, -1, -7, -50)[j]
    return st, acts, kinds


def discriminating(O, world, init, acts, trace, K, kinds, seed=SEED):
    """{(kind of change, kind of wave): discriminating gate tests} over the inner steps of one launch
    of K steps from init (the module's docstring), and {kind of wave: loaded cargo >= 50 tests}."""
    rec = windows(world, init, acts, trace, launches_of(K))
    prev = [init] + list(trace)
    n, P = len(init["x"]), world.P
    old, how, arrived = {}, {}, set()
    out, loaded50 = collections.Counter(), collections.Counter()
    for k in range(K - 1):
        a, before, after = acts[k], prev[k], trace[k]
        mover = (a >= -4) & (a < 4) & (after["err"] == OK)
        for i in np.nonzero(mover[:n & ~3])[0]:
            mode, W = rec[k][i // WAVE][:2]
            cls = "direct" if mode == "direct" else f"pool{W}"
            c = int(before["cargo"][i])
            if i not in how:  # as loaded
                if c >= 50:
                    loaded50[cls] += 1
                    out["fifty", cls] += gate_word(O, i, k, seed) > gate_thr(49)
                elif c <= 0:
                    out["nonpos", cls] += 1
                    assert after["cargo"][i] == c
                continue
            lo, hi = sorted((gate_thr(old[i]), gate_thr(c)))
            if not lo < gate_word(O, i, k, seed) <= hi:
                continue
            kind = "fifty" if c >= 50 else "zeroed" if c <= 0 else how[i]
            out[kind, cls] += 1
        changed = np.nonzero(after["cargo"] != before["cargo"])[0]
        for i in changed:
            old[i] = int(before["cargo"][i])
            if a[i] >= 4 + P:
                how[i] = "arrive_take" if i in arrived else "take"
            elif after["origin"][i] != before["origin"][i]:
                how[i] = "arrival"
                arrived.add(i)
            else:
                how[i] = "loss"
    return out, loaded50


WAVE_KINDS = ("pool8", "pool4", "direct")
CHANGES = ("take", "loss", "arrive_take", "fifty", "zeroed", "nonpos")


def assert_cargo_scenario(O, init, acts, trace, kinds):
    prev = [init] + list(trace)
    for i, kind in kinds.items():
        if kind in ("take", "raise50", "arrive_take"):
            assert trace[K_TAKE]["err"][i] == OK and trace[K_TAKE]["cargo"][i] > prev[K_TAKE]["cargo"][i], (i, kind)
            assert (trace[K_TAKE]["cargo"][i] >= 50) == (kind == "raise50")
        if kind == "arrive_take":
            assert trace[0]["cargo"][i] == 0 and trace[0]["origin"][i] == 0, (i, "arrives in row 0")
    out, loaded50 = discriminating(O, POOLW, init, acts, trace, K_CARGO, kinds)
    print({k: out[k] for k in sorted(out)}, dict(loaded50))
    for cls in WAVE_KINDS:
        for change in CHANGES:
            assert out[change, cls] >= 16, f"{change} in {cls} waves: {out[change, cls]} discriminating gate tests"
        assert loaded50[cls] >= 16, f"loaded cargo >= 50 in {cls} waves: {loaded50[cls]} gate tests"


def test_cargo_scenario_on_the_oracle(oracle_mod):
    init, acts, kinds = cargo_run()
    assert N_CARGO < 5000 and (N_CARGO & ~3) % WAVE == 4 * PART_LANES
    assert_cargo_scenario(oracle_mod, init, acts, oracle_trace(oracle_mod, POOLW, init, acts), kinds)


# plain, every wave direct, one workgroup (iters > 1: its threads step several groups in turn, so
# Carried.thr is refilled per group), the other kind of load, launches of at most 7 steps
CARGO_SETTINGS = [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}, {"SHIPENV_NT_LOADS": "0"},
                  {"SHIPENV_SEQ_MAX_STEPS": "7"}]


@gpu
@pytest.mark.parametrize("env", CARGO_SETTINGS, ids=ids_of)
def test_cargo_changes_fused_equals_step_calls(env, gpu_lib, oracle_mod):
    """Takes, partial and whole losses, arrivals followed by takes, cargo raised to and loaded at 50
    and above, cargo 0 and negative: in waves with windows of 8 and 4 and in waves that draw
    directly, after 32 steps in one launch and after 12."""
    init, acts, trace = reference("cargo", POOLW, lambda: cargo_run()[:2])
    if not env:
        for k, want in enumerate(oracle_trace(oracle_mod, POOLW, init, acts)):
            assert_same(trace[k], want, f"cargo: twin vs oracle, step {k}")
    b = POOLW.env(N_CARGO, **env)
    dev = device_rows(b, acts)
    for K in (K_CARGO, 12):
        run_fused(b, init, dev, trace, K, None, f"cargo {env}")
    b.close()


# ----------------------------------------------------------------- decode edges
class Big(World):
    """18 x 17 cells: room for 254 ports (codes 1 .. 254, the most a world holds) in rows 1 .. 15."""

    H, W = 18, 17


def _stocks(p):
    return dict(fuel=[1 + i % 9 for i in range(p)], cargo=[1 + (5 * i) % 7 for i in range(p)])


DECODE_WORLDS = {
    0: World(ports=[], fuel=[], cargo=[], ground=[(4, 6)]),
    1: World(ports=[(4, 4)], ground=[(4, 6)], **_stocks(1)),
    5: World(ports=[(1, 2), (2, 10), (4, 4), (7, 1), (7, 11)], ground=[(4, 6)], **_stocks(5)),
    254: Big(ports=[(1 + i // 17, i % 17) for i in range(254)], ground=[(16, 3)], **_stocks(254)),
}
K_DECODE = 4  # rows 0 .. 2 are inner steps
N_DECODE = 2 * WAVE + 4 * 9 + 3  # two whole waves, a wave of 9 lanes, a tail


def edge_actions(P):
    return [-2 ** 31, -5, -4, -1, 0, 3, 4, 3 + P, 4 + P, 53 + P, 54 + P, 2 ** 31 - 1]


def decode_ships(world):
    """(cell, origin, dest, the move that matters or None) per kind of ship."""
    H, W, P = world.H, world.W, world.P
    o, d = (0, 1 % P) if P else (0, 0)  # P = 0: a loaded destination that no world backs
    gx, gy = (16, 3) if P == 254 else (4, 6)
    return [
        ((H - 2, 8), o, d, None),            # at sea with a destination
        ((H - 2, 8), o, NONE, None),         # without one
        ((H - 2, 9), P - 1 if P else 0, d, None),  # origin P - 1: 3 + P is the SELECT of the origin (0: 4 is)
        ((0, 6), o, d, E_), ((H - 1, 6), o, d, W_), ((4, 0), o, d, N_), ((4, W - 1), o, d, S_),  # the four borders, moving out
        ((0, 6), o, NONE, E_),               # on a border without a destination
        ((gx, gy + 1), o, d, N_),            # against ground (and, with P = 1, out of the one port's reach:
                                             # an arrival there has no other port to draw, which no reference run meets)
    ]


def decode_run(P):
    """Every kind of ship meets every edge action in each of rows 0, 1 and 2 (env e starts the list
    at e % 12); the border and ground ships make their move in rows 0 and 2 of every second env.
    Every fifth env carries cargo, so the waves pool."""
    world = DECODE_WORLDS[P]
    ships, edges = decode_ships(world), edge_actions(P)
    rows = K_DECODE + TAIL
    st = empty_state(N_DECODE)
    acts = np.zeros((rows, N_DECODE), np.int64)
    for i in range(N_DECODE):
        (x, y), o, d, mv = ships[(i // 12) % len(ships)]
        st["x"][i], st["y"][i], st["origin"][i], st["dest"][i] = x, y, o, d
        st["fuel"][i] = 50.0 + 0.25 * i
        st["cargo"][i] = 30 if i % 5 == 0 else 0
        acts[:, i] = [edges[(i + k) % 12] for k in range(rows)]
        if mv is not None and (i // (12 * len(ships))) % 2:
            acts[0, i], acts[2, i] = mv, mv - 4  # -4 .. -1 wrap to the same moves
    return st, acts.astype(np.int32)


def assert_decode_scenario(P, init, acts, trace):
    world = DECODE_WORLDS[P]
    assert world.P == P and len({tuple(p) for p in world.ports}) == P
    inner = range(K_DECODE - 1)
    seen = {(int(acts[k][i]), int(init["dest"][i]) != NONE) for k in inner for i in range(N_DECODE & ~3)}
    assert seen >= {(a, d) for a in edge_actions(P) for d in (True, False)}
    errs = {int(e) for k in inner for e in trace[k]["err"]}
    prev = [init] + list(trace)
    if P == 0:
        assert errs == {NO_PORTS, BAD_INDEX}  # a bad index is told first; nothing passes
        assert all((trace[k][f] == init[f]).all() for k in inner for f in ("x", "y", "dest", "cargo")), "no ship moves or selects"
        return
    assert errs >= {OK, OOB, SAME_PORT, NO_DEST, BAD_INDEX} and errs & {NOT_AT_PORT, AMOUNT}
    for k in inner:
        a, s0, s1 = acts[k], prev[k], trace[k]
        mv, sel = (a >= -4) & (a < 4), (a >= 4) & (a < 4 + P)
        same_cell = (s1["x"] == s0["x"]) & (s1["y"] == s0["y"])
        assert same_cell[~mv].all() and (s1["dest"][~sel & ~mv] == s0["dest"][~sel & ~mv]).all()
        # a move that passed and found water moved; one into ground or out of the map did not
        assert (~same_cell[mv & (s1["err"] == OK)]).any()
        assert (s1["dest"][sel & (s1["err"] == OK)] == a[sel & (s1["err"] == OK)] - 4).all()
    if P == 1:
        assert all((s["origin"] == init["origin"]).all() for s in trace), "no arrival where no other port exists"
    assert any(((trace[k]["err"] == OOB) & (acts[k] >= -4) & (acts[k] < 4)).any() for k in inner)
    ground = [i for i in range(N_DECODE & ~3) if (init["x"][i], init["y"][i]) in ((16, 4), (4, 7)) and acts[0][i] == N_]
    assert ground and all(trace[0]["err"][i] == OK and trace[0]["y"][i] == init["y"][i] for i in ground), "blocked by ground"


@pytest.mark.parametrize("P", list(DECODE_WORLDS))
def test_decode_scenario_on_the_oracle(P, oracle_mod):
    init, acts = decode_run(P)
    assert_decode_scenario(P, init, acts, oracle_trace(oracle_mod, DECODE_WORLDS[P], init, acts))


@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}], ids=ids_of)
@pytest.mark.parametrize("P", list(DECODE_WORLDS))
def test_decode_edges_fused_equals_step_calls(P, env, gpu_lib, oracle_mod):
    """Actions at both ends of every range and of int32 as inner steps, for ships with and without
    a destination, on the four borders, against ground and selecting their origin, in worlds with 0,
    1, 5 and 254 ports."""
    world = DECODE_WORLDS[P]
    init, acts, trace = reference(f"decode{P}", world, lambda: decode_run(P))
    if not env:
        assert_decode_scenario(P, init, acts, trace)
        for k, want in enumerate(oracle_trace(oracle_mod, world, init, acts)):
            assert_same(trace[k], want, f"decode P={P}: twin vs oracle, step {k}")
    b = world.env(N_DECODE, **env)
    dev = device_rows(b, acts)
    for K in (K_DECODE, 2, 3):
        run_fused(b, init, dev, trace, K, None, f"decode P={P} {env}")
    b.close()


# ----------------------------------------------------------------- fuel
FUELS = (0.0, -0.0, 5e-324, 2.2250738585072014e-308 / 2, 1e308, float("inf"), 0.9, 1.0, 1.1)
K_FUEL = 4
N_FUEL = WAVE + 4 * 11 + 3


def fuel_run():
    """Each fuel value for a ship that moves every step, one that selects (stays), one without a
    destination (refused, stays) and one that runs against ground (passes, stays)."""
    rows = K_FUEL + TAIL
    st, acts = sea_run(N_FUEL, rows)
    for i in range(N_FUEL):
        st["fuel"][i] = FUELS[i % len(FUELS)]
        st["cargo"][i] = 30 if i % 7 == 0 else 0
        how = (i // len(FUELS)) % 4
        if how == 1:
            acts[:, i] = [4 + 3 if k % 2 == 0 else 4 + 2 for k in range(rows)]
        elif how == 2:
            st["dest"][i] = NONE
        elif how == 3:
            st["x"][i], st["y"][i] = 2, 0  # N_ moves to (2, -1): out; S_ to (2, 1): ground
            acts[:, i] = S_
    return st, acts


def assert_fuel_scenario(init, acts, trace):
    bits = lambda v: np.asarray(v, np.float64).view(np.int64)  # noqa: E731
    prev = [init] + list(trace)
    seen = set()
    for k in range(K_FUEL - 1):
        s0, s1 = prev[k], trace[k]
        moved = (s1["x"] != s0["x"]) | (s1["y"] != s0["y"])
        assert (bits(s1["fuel"])[~moved] == bits(s0["fuel"])[~moved]).all(), "a ship that stays keeps its fuel's bits"
        assert (s1["fuel"][moved & np.isfinite(s0["fuel"]) & (s0["fuel"] < 1e300)] < s0["fuel"][moved & np.isfinite(s0["fuel"]) & (s0["fuel"] < 1e300)]).all()
        if k == 0:
            seen = {(int(b), bool(m)) for b, m in zip(bits(init["fuel"]), moved)}
    assert seen >= {(int(bits(f)), m) for f in FUELS for m in (True, False)}
    assert any(((trace[k]["err"] == OK) & (acts[k] == S_) & (trace[k]["y"] == 0)).any() for k in range(K_FUEL - 1)), "ground"
    assert any((trace[k]["err"] == NO_DEST).any() for k in range(K_FUEL - 1))
    assert (bits(trace[K_FUEL - 2]["fuel"]) == bits(-0.0)).any() and np.isinf(trace[K_FUEL - 2]["fuel"]).any()


def test_fuel_scenario_on_the_oracle(oracle_mod):
    init, acts = fuel_run()
    assert_fuel_scenario(init, acts, oracle_trace(oracle_mod, POOLW, init, acts))


@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}], ids=ids_of)
def test_fuel_edges_fused_equals_step_calls(env, gpu_lib, oracle_mod):
    """Loaded fuel of +0.0, -0.0, subnormals, 1e308, +inf and values about the cost, for movers and
    for ships that stay, through three inner steps."""
    init, acts, trace = reference("fuel", POOLW, fuel_run)
    if not env:
        assert_fuel_scenario(init, acts, trace)
        for k, want in enumerate(oracle_trace(oracle_mod, POOLW, init, acts)):
            assert_same(trace[k], want, f"fuel: twin vs oracle, step {k}")
    b = POOLW.env(N_FUEL, **env)
    dev = device_rows(b, acts)
    for K in (K_FUEL, 3):
        run_fused(b, init, dev, trace, K, None, f"fuel {env}")
    b.close()
