"""The SARSA restatement (tests/sarsa_support.py) against the session recorded from the
reference's SARSAAgent (tests/golden/sarsa_golden.json), event by event and in the final
q_table, exactly; the dense table's layout arithmetic, key <-> entry; and the restatement's
own rules for many envs on one table. No GPU."""
import json
import os
import types

import numpy as np
import pytest

import sarsa_support as SS
from conftest import GOLDEN
from rollout_support import MANY, ONE, OPEN, SHARED


@pytest.fixture(scope="module")
def session():
    with open(os.path.join(GOLDEN, "sarsa_golden.json")) as f:
        return json.load(f)


def golden_world(doc):
    return types.SimpleNamespace(H=doc["H"], W=doc["W"], P=len(doc["ports"]), px=[p[0] for p in doc["ports"]],
                                 py=[p[1] for p in doc["ports"]], pf=doc["port_fuel"], pc=doc["port_cargo"])


def plain(world):
    """A hand-made world of rollout_support as the restatement reads it."""
    return types.SimpleNamespace(H=world.H, W=world.W, P=world.P, px=[p[0] for p in world.ports],
                                 py=[p[1] for p in world.ports], pf=world.fuel_stock, pc=world.cargo_stock)


def test_golden_session_is_reproduced_exactly(session):
    """Every recorded uniform, sample, step, choice and update is asked for in the reference's
    order with the reference's arguments, every update has its q before and after bit for bit
    (float.hex), and the final table equals the reference's q_table, keys and values."""
    learner, steps = SS.replay_session(golden_world(session), session)
    updates = sum(1 for ev in session["events"] if ev[0] == "update")
    assert steps == updates >= 100
    want = {SS.key_from_json(k): float.fromhex(v) for k, v in session["q_table"]}
    assert learner.q.keys() == want.keys()
    for k, v in want.items():
        assert learner.q[k].hex() == v.hex(), k
    assert learner.collisions == 0


def test_golden_session_covers_what_it_is_for(session):
    ev = session["events"]
    world = golden_world(session)
    steps = [e for e in ev if e[0] == "step"]
    assert any("raise" in e[2] for e in steps), "no step raised: the retry loop never ran"
    assert any(e[2].get("done") for e in steps), "no done step"
    assert sum(1 for e in ev if e[0] == "reset") >= 3
    eps = {float.fromhex(e[2]) for e in ev if e[0] == "uniform"}
    assert 0.0 in eps and 1.0 in eps and any(0.0 < e < 1.0 for e in eps)
    types_chosen = {e[1][0] for e in ev if e[0] == "chose"}
    assert types_chosen == {SS.MOVE, SS.SELECT, SS.TAKE_FUEL, SS.TAKE_CARGO}
    placed = [SS.ship_from_json(e[1]) for e in ev if e[0] == "place"]
    assert {9.99, 10.0, 20.0, 39.99, 40.0, 80.0} <= {s[2] for s in placed}
    assert any((s[0], s[1]) == (0, 0) for s in placed)
    assert any(SS.port_at(world, s[0], s[1]) != SS.NONE and s[5] == SS.NONE for s in placed)
    assert any(SS.port_at(world, s[0], s[1]) != SS.NONE and s[5] != SS.NONE for s in placed)
    # every fuel class is a key of the final table
    assert {(k[2], k[3]) for k, _ in session["q_table"]} == set(SS.BUCKETS)


def test_discretiser_is_the_reference_formula_at_every_boundary():
    for fuel, want in ((0.0, (0, 0)), (9.99, (0, 0)), (10.0, (1, 0)), (19.999, (1, 0)), (20.0, (2, 1)),
                       (29.99, (2, 1)), (30.0, (3, 1)), (39.99, (3, 1)), (40.0, (4, 2)), (59.99, (4, 2)),
                       (60.0, (4, 3)), (79.99, (4, 3)), (80.0, (4, 4)), (200.0, (4, 4)), (1e9, (4, 4)),
                       (-0.5, (0, 0)), (-9.99, (0, 0))):
        assert SS.buckets(fuel) == want, fuel
        assert SS.BUCKETS[SS.fuel_class(fuel)] == want
    assert SS.fuel_class(-10.0) == 0 and SS.fuel_class(-1e9) == 0  # outside the domain: clamped
    # the seven pairs are all that occur
    seen = {SS.buckets(f) for f in np.arange(-9.99, 250.0, 0.01)}
    assert seen == set(SS.BUCKETS)


@pytest.mark.parametrize("world", [OPEN, ONE, SHARED, MANY], ids=["open", "one", "shared", "many"])
def test_layout_round_trips_every_key_kind(world):
    w = plain(world)
    lay = SS.Layout(w)
    assert lay.cmax == max(20, max(w.pc)) and lay.A == w.P + 4 + lay.cmax + 20
    assert lay.rows == w.H * w.W * 7 * (w.P + 1) ** 2
    actions = [(SS.SELECT, p, 0) for p in range(w.P)] + [(SS.MOVE, a, b) for a, b in SS.MOVES] + \
              [(SS.TAKE_CARGO, m, 0) for m in range(1, lay.cmax + 1)] + [(SS.TAKE_FUEL, m, 0) for m in range(1, 21)]
    assert [lay.slot(a) for a in actions] == list(range(lay.A))  # the slots in order, none missing
    assert [lay.action(s) for s in range(lay.A)] == actions
    ports = [SS.NONE] + list(range(w.P))
    cells = [(0, 0), (0, w.W - 1), (w.H - 1, 0), (w.H - 1, w.W - 1), (w.H // 2, w.W // 3)]
    seen = set()
    for cell in cells:
        for cb, fb in SS.BUCKETS:
            for origin in (ports[0], ports[1], ports[-1]):
                for dest in (ports[0], ports[1], ports[-1]):
                    for action in (actions[0], actions[w.P - 1], actions[w.P], actions[w.P + 3], actions[w.P + 4],
                                   actions[w.P + 3 + lay.cmax], actions[w.P + 4 + lay.cmax], actions[-1]):
                        key = ((cell,) + (cb, fb, origin, dest), action)
                        e = lay.entry(key)
                        assert 0 <= e < lay.rows * lay.A
                        assert lay.key(e) == key
                        seen.add(e)
    # the first and the last entry are keys
    assert lay.key(0) == (((0, 0), 0, 0, SS.NONE, SS.NONE), actions[0])
    assert lay.key(lay.rows * lay.A - 1) == (((w.H - 1, w.W - 1), 4, 4, w.P - 1, w.P - 1), actions[-1])
    assert 0 not in seen or lay.entry(lay.key(0)) == 0


class ScriptDriver:
    """Every env takes the same scripted step: never explores, the step goes through with a
    reward that depends on the env index."""

    def __init__(self):
        self.i = 0

    def begin(self, i, t):
        self.i = i

    def uniform(self, which):
        return 0.5

    def sample(self, ship, which):
        raise AssertionError("nothing explores")

    def step(self, ship, action, j):
        return ship, 1.0 + self.i, False

    def restart(self):
        return (1, 1, 200.0, 0, 0, 1)

    def chose(self, action):
        pass

    def updated(self, key, before, after):
        pass


def test_reads_are_synchronous_and_the_lowest_index_wins():
    w = plain(OPEN)
    learner = SS.Learner(w, lr=0.5, gamma=0.0)
    envs = [SS.Env((3, 3, 100.0, 0, 0, 1)) for _ in range(3)]
    learner.vector_step(envs, 0.0, True, ScriptDriver(), 0)
    key = (SS.discretize(envs[0].ship), (SS.SELECT, 0, 0))
    assert learner.q == {key: 0.5} and learner.collisions == 2  # env 0's reward 1.0, not 2.0 or 3.0
    learner.vector_step(envs, 0.0, True, ScriptDriver(), 1)
    assert learner.q == {key: 0.75}  # every env read 0.5; env 0 wrote 0.5 + 0.5 * (1.0 - 0.5)
    learner.vector_step(envs, 0.0, False, ScriptDriver(), 2)
    assert learner.q == {key: 0.75}  # learn = 0
