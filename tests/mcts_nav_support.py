"""se_mcts_choose_nav restated on the CPU, for tests/test_mcts_nav_cpu.py and
tests/test_gpu_mcts_nav.py: mcts_support.choose_action (imported, not copied) with a driver whose
rollout() is the navigated rollout nav_support.nav_rollout under the simulation's id. The tree
steps, the choice word and the root fallback are mcts_support.PhiloxDriver's, unchanged.

choose_action treats a rollout kind it does not know as "ok": a playout that ended where the
navigator had no action ("stuck") is backpropagated with its partial return, and decide() sets the
sticky status STUCK afterwards unless the decision raised.

Two scenario tables: mcts_support.SCENARIOS as it stands, and NAV_SCENARIOS on nav_support's
worlds (an unreachable port, a walled-in cell, a detour, one-cell-wide maps, a 1 x 1 map).
"""
import mcts_support as MS
import nav_support as NS
import plan_support as PS

NONE = MS.NONE
OK, CUT, RAISED, NEVER_RETURNS, STUCK = MS.OK, MS.CUT, MS.RAISED, MS.NEVER_RETURNS, 4  # SE_MCTS_*
SEED, SIMS, REPS, TAIL = MS.SEED, MS.SIMS, MS.REPS, MS.TAIL
MAX_STEPS, REFUEL_BELOW, LOAD, C_PARAM = 6, 3.0, 3, 1.4


class NavDriver(MS.PhiloxDriver):
    """PhiloxDriver with the navigator's playout: position k of simulation `id` draws what
    se_rollout_nav's position k draws for ids[r] = id. world is a rollout_support.World.
    playouts keeps every playout's NavRollout (res.ret, res.status, res.raised, stuck_at,
    arrivals, ...) in the order they were asked for."""

    def __init__(self, O, world, seed, id0, max_steps, refuel_below, load, oracle_world=None):
        ow = oracle_world or world.oracle(O)
        super().__init__(O, ow, seed, id0, max_steps, 0)
        self.nav_world, self.refuel_below, self.load = world, refuel_below, load
        self.stepper = PS.Stepper(O, ow, seed)
        self.playouts = []

    def rollout(self, ship):
        r = NS.nav_rollout(self.O, self.nav_world, ship, self.max_steps, self.refuel_below, self.load, self.seed,
                           self.id, stepper=self.stepper)
        self.playouts.append(r)
        return r.res.ret, "stuck" if r.res.status == NS.STUCK else "ok"


def decide(O, world, ship, *, seed, id0, S, c=C_PARAM, max_steps=MAX_STEPS, refuel_below=REFUEL_BELOW, load=LOAD,
           oracle_world=None):
    """One env's decision with navigator playouts; id0 = mcts_base + (the env's global id) * S.
    The Decision also carries the driver's playouts."""
    drv = NavDriver(O, world, seed, id0, max_steps, refuel_below, load, oracle_world)
    d = MS.choose_action(ship, world.P, [int(v) for v in world.cargo_stock], S, c, drv)
    if d.status not in (RAISED, NEVER_RETURNS) and any(p.res.status == NS.STUCK for p in drv.playouts):
        d.status = STUCK
    d.playouts = drv.playouts
    return d


def restated_playout(O, world, ship, *, seed, ident, max_steps=MAX_STEPS, refuel_below=REFUEL_BELOW, load=LOAD):
    """What the driver's rollout() answers for `ship` as the playout of simulation `ident`."""
    drv = NavDriver(O, world, seed, ident, max_steps, refuel_below, load)
    drv.simulation(0)
    return drv.rollout(ship)


# ---------------------------------------------------------------------------- scenarios
def _ship(cell, origin, dest, fuel=100.0):
    return MS.ship(cell, origin, NONE if dest is None else dest, fuel=fuel)


# name -> (world, [(label, ship)]): fuel 100 and cargo 0 unless noted
NAV_SCENARIOS = {
    "lake": (NS.LAKE, [
        ("to_pocket", _ship((0, 7), 0, 1)),            # bound for the pocket port, unreachable from outside
        ("from_pocket", _ship((3, 3), 1, 0)),          # from inside the pocket
        ("outside", _ship((0, 7), 0, 2)),              # between the two outside ports
        ("walled_in", _ship((3, 7), 0, 2)),            # the walled-in cell
        ("pocket_select", _ship((3, 3), 1, None)),     # no destination in the pocket: none is reachable
        ("outside_select", _ship((0, 7), 0, None)),    # no destination outside: port 2 is, port 1 is not
    ]),
    "wall": (NS.WALL, [
        ("at_the_wall", _ship((2, 3), 0, 1)),          # port 1 lies east, the way is south-about
        ("detour", _ship((2, 1), 0, 1, fuel=200.0)),
        ("detour_dry", _ship((2, 1), 0, 1, fuel=2.0)),
    ]),
    "row": (NS.ROW, [
        ("row_port", _ship((0, 1), 0, 1)),
        ("row_end", _ship((0, 0), 0, 1)),
    ]),
    "col": (NS.COL, [
        ("col_port", _ship((1, 0), 0, 1)),
        ("col_select", _ship((5, 0), 2, None)),
    ]),
    "dot": (NS.DOT, [
        ("dot_select", _ship((0, 0), 0, None)),
        ("dot_home", _ship((0, 0), 0, 0)),
    ]),
}
SCENARIOS = {name: (world, [(label, sh) for label, sh, _ in rows]) for name, (world, rows) in MS.SCENARIOS.items()}
SCENARIOS.update(NAV_SCENARIOS)


def scenario_actors(name, reps=REPS):
    """The actor index of every env: each actor `reps` times in a row, then the first TAIL actors
    (cyclically) once more, so n = 64 k + 3."""
    k = len(SCENARIOS[name][1])
    return [a for a in range(k) for _ in range(reps)] + [j % k for j in range(TAIL)]


def scenario_ships(name, reps=REPS):
    return [SCENARIOS[name][1][a][1] for a in scenario_actors(name, reps)]


_DECISIONS = {}


def decisions(O, name, S, *, reps=REPS, mcts_base=0, env_id_base=0, **kw):
    """The restatement's decision for every env of the scenario table (computed once per argument
    set and shared: callers leave it unchanged). Env i's simulation 0 has id mcts_base +
    (env_id_base + i) * S."""
    key = (name, S, reps, mcts_base, env_id_base, tuple(sorted(kw.items())))
    if key not in _DECISIONS:
        world = SCENARIOS[name][0]
        ow = world.oracle(O)
        _DECISIONS[key] = [decide(O, world, sh, seed=SEED, id0=mcts_base + (env_id_base + i) * S, S=S,
                                  oracle_world=ow, **kw)
                           for i, sh in enumerate(scenario_ships(name, reps))]
    return _DECISIONS[key]


def by_actor(O, name, label):
    """[(S, decision)] of every env of actor `label` at every S of SIMS."""
    a = [lb for lb, _ in SCENARIOS[name][1]].index(label)
    return [(S, d) for S in SIMS for d, who in zip(decisions(O, name, S), scenario_actors(name)) if who == a]
