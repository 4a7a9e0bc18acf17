"""The state-only steps of a fused se_step_seq run a regular form in a wave all of whose envs are
inside the map and have a destination (step_seq.h, step_group_ring): the position is carried biased
by one, the one cell lookup reads a bordered cell table at the move's target, whose code says "off
the map", "ground" or neither, one ballot of "some ship of the wave is on a non-water cell" is the
arrival vote of a step and the first take vote of the next, and the firing gates and arrivals stay
lane masks until a wave has one. A wave with an irregular env, and every wave of a launch without
the table (more than 253 ports, no LDS room, SHIPENV_SEQ_RING=0), runs the general step.

What can go wrong: a move off the map that draws the gate or tests an arrival, a move blocked by
ground that does neither, a table index with the sides swapped or the bias left on (or taken off
twice) when the state is packed, a stale vote word right after an arrival or for a ship that sits
on a port, port 252's code 253 taken for the border's 254, and a wave that takes the regular path
with an env off the map or without a destination.

The method is step_seq_support's: a twin env stepped by plain steps, the C oracle's trace, and one
step_seq call of 2, 17 and 40 steps, all equal bit for bit, with 2 plain steps after. The envs are
three whole waves, a wave of 20 lanes and a tail of 3 envs, in three worlds: a hand-built 7 x 9 map
with ground and ports on a corner, on two edges, in the interior and two on one cell; a 20 x 20 map
with 253 ports (the most that leave the table its border code); the same with 254 ports (no
table). In the hand-built world wave 0 is regular and holds the scripted ships, wave 1 is at sea
(no ship on a port's cell for the whole run) but for one ship loaded at x = 200, wave 2 is regular
but for one env without a destination, and the wave of 20 lanes holds a ship loaded at x = H. The
companion test without the gpu mark asserts on the oracle alone that the trace holds what the
scripts claim."""
import numpy as np
import pytest

from step_seq_support import (AMOUNT, NO_DEST, NONE, OK, OOB, TAIL, assert_same, device_rows, gpu_lib, oracle_trace,  # noqa: F401
                              run_fused, twin_trace)
from test_gpu_step_seq_trim import E_, N_, S_, W_, World, generic_run

gpu = pytest.mark.gpu

WAVE, PART_LANES = 256, 20
N = 3 * WAVE + 4 * PART_LANES + 3
KS = (2, 17, 40)
K = max(KS)
LAST_CLAIM = min(KS[1:]) - 2  # a claim is about an inner step of the runs of 17 and of 40 steps
HEAVY = 55  # cargo >= 50: the gate, where it is drawn, fires with certainty
SETTINGS = [{}, {"SHIPENV_SEQ_RING": "0"}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}]


def ids_of(env):
    return "-".join(f"{k[8:].lower()}{v}" for k, v in env.items()) or "plain"


class Hand(World):
    """7 x 9: W != H, and no side a multiple of anything."""

    H, W = 7, 9


class Twenty(World):
    H, W = 20, 20


# ports 0 on a corner, 1 and 5 on edges, 2 in the interior with ground north of it, 3 and 4 on one cell
HAND = Hand(ports=[(0, 0), (0, 5), (3, 4), (5, 2), (5, 2), (3, 8)], fuel=[7, 5, 9, 4, 8, 6], cargo=[3, 6, 9, 2, 8, 5],
            ground=[(3, 3), (1, 7), (5, 6)])
LAST_PORT, BESIDE_LAST = (10, 10), (10, 11)


def twenty(P):
    """P ports on distinct cells of a 20 x 20 map, the last at LAST_PORT with water south of it, 20
    cells of ground."""
    rng = np.random.default_rng(P)
    cells = [(x, y) for x in range(20) for y in range(20) if (x, y) not in (LAST_PORT, BESIDE_LAST)]
    cells = [cells[i] for i in rng.permutation(len(cells))]
    return Twenty(ports=cells[:P - 1] + [LAST_PORT], fuel=[1 + i % 9 for i in range(P)], cargo=[1 + (5 * i) % 7 for i in range(P)],
                  ground=cells[P - 1:P + 19])


WORLDS = {"hand": HAND, "p253": twenty(253), "p254": twenty(254)}


def ship(cell, origin, dest, cargo=0):
    return dict(cell=cell, origin=origin, dest=dest, cargo=cargo)


def hand_scripts():
    """[(label, wave, copies, ship, first rows, row repeated after them (None: selects, the ship
    stays), claims)]; a claim (k, field, value) holds after step k <= LAST_CLAIM, "all" for k: after
    every step up to LAST_CLAIM."""
    tc, tf = HAND.cargo, HAND.fuel
    stay = [(k, f, v) for k in ("all",) for f, v in (("err", OOB), ("cargo", HEAVY))]
    return [
        # a carrier off each edge and off two corners: an error, no gate draw (cargo 55 would be lost)
        ("off_north", 0, 4, ship((2, 0), 0, 2, HEAVY), [], N_, stay + [("all", "pos", (2, 0))]),
        ("off_south", 0, 4, ship((2, 8), 0, 2, HEAVY), [], S_, stay + [("all", "pos", (2, 8))]),
        ("off_east", 0, 4, ship((0, 3), 0, 2, HEAVY), [], E_, stay + [("all", "pos", (0, 3))]),
        ("off_west", 0, 4, ship((6, 3), 0, 2, HEAVY), [], W_, stay + [("all", "pos", (6, 3))]),
        ("off_corner_sw", 0, 4, ship((6, 0), 0, 2, HEAVY), [W_, N_, W_, N_], N_, stay + [("all", "pos", (6, 0))]),
        ("off_corner_ne", 0, 4, ship((0, 8), 0, 2, HEAVY), [E_, S_, S_, E_], E_, stay + [("all", "pos", (0, 8))]),
        # the same carrier blocked by ground: a move, the gate fires (step 0: cargo 55) and cargo is lost
        ("blocked_carrier", 0, 4, ship((3, 2), 0, 2, HEAVY), [], S_, [("all", "err", OK), ("all", "pos", (3, 2)), (LAST_CLAIM, "lost", HEAVY)]),
        # blocked by the ground north of port 2 while standing on it, its destination: an arrival
        ("blocked_arrival", 0, 4, ship((3, 4), 0, 2, 20), [4 + 2, N_], None,
         [(0, "cargo", 20), (1, "err", OK), (1, "pos", (3, 4)), (1, "origin", 2), (1, "cargo", 0)]),
        # an arrival, and on the next step a take of cargo, of fuel: the vote word's hand-over
        ("arrive_take_cargo", 0, 4, ship((3, 5), 0, 2, 10), [4 + 2, 4 + 2, N_, tc(9)], None,
         [(2, "pos", (3, 4)), (2, "origin", 2), (2, "cargo", 0), (3, "err", OK), (3, "cargo", 9)]),
        ("arrive_take_fuel", 0, 4, ship((3, 5), 0, 2, 10), [4 + 2, N_, tf(9)], None,
         [(1, "pos", (3, 4)), (1, "origin", 2), (1, "cargo", 0), (2, "err", OK), (2, "fuel_gain", 9.0)]),
        # a take by a ship that has sat on port 1 for six steps
        ("sit_then_take", 0, 4, ship((0, 5), 0, 2), [4 + 2] * 6 + [tc(6)], None, [(5, "cargo", 0), (6, "err", OK), (6, "cargo", 6)]),
        # the shared cell answers with port 3's stocks; an arrival at port 4 happens there
        ("shared_cell", 0, 4, ship((5, 3), 0, 4, 10), [N_, tc(2), tc(3)], None,
         [(0, "pos", (5, 2)), (0, "origin", 4), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 2), (2, "err", AMOUNT), (2, "cargo", 2)]),
        # wave 1's only irregular env: loaded at x = 200, it moves and stays off the map
        ("loaded_off_map", 1, 1, ship((200, 3), 0, 1, HEAVY), [], E_, stay + [("all", "pos", (200, 3))]),
        # wave 2's only irregular env: no destination; it selects, moves onto port 2 (a gate draw) and arrives
        ("no_dest_then_arrives", 2, 1, ship((2, 4), 0, NONE, HEAVY), [W_, W_, 4 + 2, W_], None,
         [(0, "err", NO_DEST), (1, "err", NO_DEST), (1, "pos", (2, 4)), (1, "cargo", HEAVY), (2, "dest", 2), (3, "err", OK),
          (3, "pos", (3, 4)), (3, "origin", 2), (3, "cargo", 0)]),
        # in the wave of 20 lanes: loaded at x = H, it moves into the map
        ("loaded_at_H", 3, 1, ship((Hand.H, 2), 0, 1), [E_], None, [(0, "err", OK), (0, "pos", (Hand.H - 1, 2))]),
    ]


def script_envs(s, wave, copies):
    """Copy j of script s sits in lane 4 s + j of wave 0 as the lane's env j; a script of another
    wave (one copy) in one of that wave's first 20 lanes."""
    lane = 4 * s if wave == 0 else (4 * s) % PART_LANES
    return [wave * WAVE + 4 * (lane + j) + j for j in range(copies)]


def hand_run():
    rows = K + TAIL
    st, acts = generic_run(HAND, N, rows)
    # wave 1 at sea: pairs of water cells (x, y), (x + 1, y) with no port on or beside them
    ports = {tuple(p) for p in HAND.ports}
    free = lambda x, y: 0 <= x < Hand.H and 0 <= y < Hand.W and HAND.water[x, y] and (x, y) not in ports  # noqa: E731
    pairs = [(x, y) for x in range(Hand.H - 1) for y in range(Hand.W) if free(x, y) and free(x + 1, y)]
    for i in range(WAVE, 2 * WAVE):
        st["x"][i], st["y"][i] = pairs[i % len(pairs)]
        st["cargo"][i] = 30 if i % 7 == 0 else 0
        acts[:, i] = [W_ if k % 2 == 0 else E_ for k in range(rows)]
    for s, (_, wave, copies, sh, first, then, _) in enumerate(hand_scripts()):
        for i in script_envs(s, wave, copies):
            st["x"][i], st["y"][i] = sh["cell"]
            st["origin"][i], st["dest"][i], st["cargo"][i] = sh["origin"], sh["dest"], sh["cargo"]
            st["fuel"][i] = 100.0 + 0.125 * (i % 64)
            acts[:, i] = [then if then is not None else 4 + 2 + k % 2 for k in range(rows)]
            acts[:len(first), i] = first
    return st, acts


def twenty_run(world):
    st, acts = generic_run(world, N, K + TAIL)
    P = world.P
    a, b = 8, 4 * 13 + 1
    # a ship on the last port (code P) takes cargo and fuel there
    st["x"][a], st["y"][a] = LAST_PORT
    st["origin"][a], st["dest"][a], st["cargo"][a], st["fuel"][a] = 0, 1, 0, 50.0
    acts[:3, a] = [world.cargo(1), world.fuel(1), world.cargo(world.cargo_stock[P - 1] + 1)]
    # another arrives there and takes on the next step
    st["x"][b], st["y"][b] = BESIDE_LAST
    st["origin"][b], st["dest"][b], st["cargo"][b], st["fuel"][b] = 0, P - 1, 10, 50.0
    acts[:3, b] = [4 + P - 1, N_, world.cargo(1)]
    return st, acts


def run_of(name):
    return hand_run() if name == "hand" else twenty_run(WORLDS[name])


def irregular(world, st):
    return (st["dest"] == NONE) | (st["x"] >= world.H) | (st["y"] >= world.W)


def assert_claims(envs, claims, init, trace, label):
    prev = [init] + list(trace)
    for k, field, want in claims:
        for kk in (range(LAST_CLAIM + 1) if k == "all" else [k]):
            assert kk <= LAST_CLAIM, f"{label}: a claim about step {kk} is about no inner step of the run of {KS[1]}"
            if field == "pos":
                got = np.stack([trace[kk]["x"][envs], trace[kk]["y"][envs]], 1)
                assert (got == np.array(want)).all(), f"{label}: step {kk} position {got[0]} != {want}"
            elif field == "fuel_gain":
                assert (trace[kk]["fuel"][envs] - prev[kk]["fuel"][envs] == want).all(), f"{label}: step {kk} fuel"
            elif field == "lost":  # every copy fired at step 0 for certain; by step kk some cargo is gone
                assert (trace[kk]["cargo"][envs] < want).any(), f"{label}: no cargo lost by step {kk}"
            else:
                assert (trace[kk][field][envs] == want).all(), f"{label}: step {kk} {field} {trace[kk][field][envs]} != {want}"


def assert_scenario(name, init, acts, trace):
    world = WORLDS[name]
    assert N % 4 == 3 and (N & ~3) % WAVE == 4 * PART_LANES
    irr = irregular(world, init)
    per_wave = [int(irr[w * WAVE:(w + 1) * WAVE].sum()) for w in range(4)]
    if name != "hand":
        P = world.P
        assert per_wave == [0, 0, 0, 0] and not irr[-3:].any() and len({tuple(p) for p in world.ports}) == P
        assert tuple(world.ports[P - 1]) == LAST_PORT and world.water[BESIDE_LAST] and list(BESIDE_LAST) not in world.ports
        a, b = 8, 4 * 13 + 1
        c = world.cargo_stock[P - 1]
        assert_claims([a], [(0, "err", OK), (0, "cargo", 1), (1, "err", OK), (1, "fuel_gain", 1.0), (2, "cargo", 1)], init, trace, f"{name} a")
        assert trace[2]["err"][a] == AMOUNT and c >= 1
        assert_claims([b], [(0, "dest", P - 1), (1, "pos", LAST_PORT), (1, "origin", P - 1), (1, "cargo", 0), (2, "err", OK), (2, "cargo", 1)],
                      init, trace, f"{name} b")
        # the random ships move off the map, onto ground, lose cargo and arrive
        errs = np.stack([s["err"] for s in trace[:LAST_CLAIM + 1]])
        moves = (acts[:LAST_CLAIM + 1] >= -4) & (acts[:LAST_CLAIM + 1] < 4)
        assert (errs[moves] == OOB).sum() >= 20 and (errs[moves] == OK).sum() >= 1000
        return
    assert per_wave == [0, 1, 1, 1] and not irr[-3:].any()
    assert HAND.ports[3] == HAND.ports[4] and (HAND.fuel_stock[3], HAND.cargo_stock[3]) != (HAND.fuel_stock[4], HAND.cargo_stock[4])
    scripts = hand_scripts()
    assert 4 * len(scripts) <= 64
    for s, (label, wave, copies, _, _, _, claims) in enumerate(scripts):
        assert_claims(script_envs(s, wave, copies), claims, init, trace, label)
    # wave 1: no ship on any port's cell for the whole run
    ports = {tuple(p) for p in HAND.ports}
    for s in [init] + list(trace[:K - 1]):
        on = [(int(x), int(y)) in ports for x, y in zip(s["x"][WAVE:2 * WAVE], s["y"][WAVE:2 * WAVE])]
        assert not any(on)
    # and it moves: carriers among it draw the gate
    assert (trace[0]["x"][WAVE:2 * WAVE] != init["x"][WAVE:2 * WAVE]).sum() >= WAVE - 1
    # the ship loaded off the map in wave 1 is still there after the run; the one loaded at x = H is inside
    assert trace[K - 1]["x"][script_envs(12, 1, 1)[0]] == 200 and not irregular(HAND, trace[0])[3 * WAVE:].any()
    # wave 2 is regular once its env has selected (the kernel keeps the general step for the run)
    assert not irregular(HAND, trace[2])[2 * WAVE:3 * WAVE].any()


_REF = {}


def oracle_reference(O, name):
    """The oracle's recorded steps (read-only, shared by the cases)."""
    if name not in _REF:
        init, acts = run_of(name)
        trace = oracle_trace(O, WORLDS[name], init, acts)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _REF[name] = (init, acts, trace)
    return _REF[name]


_TWIN = {}


def twin_reference(O, name):
    """The twin's recorded steps, equal to the oracle's step by step."""
    if name not in _TWIN:
        init, acts, want = oracle_reference(O, name)
        trace = twin_trace(WORLDS[name], init, acts)
        for k in range(len(acts)):
            assert_same(trace[k], want[k], f"{name}: twin vs oracle, step {k}")
        _TWIN[name] = trace
    return _TWIN[name]


@pytest.mark.parametrize("name", list(WORLDS))
def test_scenario_on_the_oracle(name, oracle_mod):
    init, acts, trace = oracle_reference(oracle_mod, name)
    assert_scenario(name, init, acts, trace)


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("name", list(WORLDS))
def test_fused_run_equals_the_twin_and_the_oracle(name, env, gpu_lib, oracle_mod):
    """Runs of 2, 17 and 40 steps from the same state end in the twin's bits, which are the oracle's."""
    init, acts, _ = oracle_reference(oracle_mod, name)
    trace = twin_reference(oracle_mod, name)
    b = WORLDS[name].env(N, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"ring {name} {env}")
    b.close()
