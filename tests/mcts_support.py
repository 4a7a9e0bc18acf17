"""MCTSAgent.choose_action (agents/mcts.py:240-292) restated in plain Python over a tree of
small records, for the tests of se_mcts_choose / VecMCTSAgent.

The restatement is written against a *driver* that supplies everything random or
environment-made:

    simulation(s)            simulation s begins (a fresh env copy, :257)
    choice(k) -> index       random.choice over k untried actions (:274)
    step(ship, action)       env_copy.step(action): (next ship, reward, done), or None if it raised
    rollout(ship)            _rollout from the env copy (:282): (return, kind), kind one of
                             "ok", "cut" (stopped at max_attempts), "raised", "never"
    sample(ship)             the root fallback's env.sample_action() (:292): action, or
                             "raised" / "never"

Two drivers: PhiloxDriver states the kernel's draw contract a second time through the C oracle
(oracle.philox, oracle.step with a tape, oracle.rollout); GoldenDriver replays a decision
recorded from the reference itself (tests/golden/make_mcts_golden.py) and checks that the
restatement asks for the same choices, steps and rollouts in the same order.

A ship is the tuple (x, y, fuel, cargo, origin, dest) with NONE = -1; an action is (type, a, b).
"""
import math

import numpy as np

from rollout_support import MANY, ONE, OPEN, SHARED

NONE = -1
MOVE, SELECT, TAKE_CARGO = 1, 2, 4
SAMPLE_RAISES, SAMPLE_NO_OTHER_PORT = -1, -2
OK, CUT, RAISED, NEVER_RETURNS = 0, 1, 2, 3
MOVES = [(0, -1), (0, 1), (-1, 0), (1, 0)]  # get_possible_actions' order (:82-85)
SLOT_TREE, SLOT_TREE_B = 18, 19
M32 = 0xFFFFFFFF


class Node:
    __slots__ = ("parent", "action", "origin", "dest", "fuel_zero", "visits", "total", "children")

    def __init__(self, parent, action, ship):
        self.parent, self.action = parent, action
        # what get_possible_actions reads of the stored state (:61-74): the origin, the
        # destination, and state["ship"]["cargo"] == 0, which is the fuel (environment.py:206)
        self.origin, self.dest, self.fuel_zero = ship[4], ship[5], ship[2] == 0
        self.visits, self.total, self.children = 0, 0.0, []


def possible_actions(node, P, port_cargo):
    """get_possible_actions (:50-89) on the node's stored state."""
    if node.dest == NONE:
        return [(SELECT, i, 0) for i in range(P) if i != node.origin]
    if node.fuel_zero and node.origin != NONE:
        return [(TAKE_CARGO, k, 0) for k in range(1, port_cargo[node.origin] + 1)]
    return [(MOVE, a, b) for a, b in MOVES]


def best_child(nodes, node, c, log):
    """best_child (:109-128): the first maximum of UCB1 in f64, in the reference's order of
    operations. None where np.argmax raises on an empty list."""
    best, best_u = None, None
    for j in node.children:
        ch = nodes[j]
        if ch.visits == 0:
            u = math.inf
        else:
            u = ch.total / ch.visits + c * math.sqrt(2 * log[node.visits] / ch.visits)
        if best is None or u > best_u:
            best, best_u = j, u
    return best


class Decision:
    """What a decision ended with: action (None where it raised), status, nodes; and what it
    went through, for the scenario claims."""

    def __init__(self):
        self.action, self.status, self.nodes = None, OK, []
        self.depth = 0               # the deepest node created
        self.expansion_raised = 0    # simulations abandoned at :278
        self.broke_on_done = 0       # selections ended by a step that reported done (:265)
        self.broke_on_raise = 0      # ... by a step that raised (:267)
        self.root_possible = 0
        self.fallback = False


def choose_action(ship, P, port_cargo, S, c, driver):
    log = [0.0] + [math.log(v) for v in range(1, S + 1)]  # np.log(parent.visits), visits <= S
    out = Decision()
    nodes = out.nodes
    nodes.append(Node(NONE, None, ship))
    depth = {0: 0}
    out.root_possible = len(possible_actions(nodes[0], P, port_cargo))

    def raised(kind):
        out.status = NEVER_RETURNS if kind == "never" else RAISED
        out.action = (SAMPLE_NO_OTHER_PORT if kind == "never" else SAMPLE_RAISES, 0, 0)
        return out

    for s in range(S):
        driver.simulation(s)
        cur, at = ship, 0
        # selection (:260-268); is_terminal() is never true
        while len(nodes[at].children) == len(possible_actions(nodes[at], P, port_cargo)):
            at = best_child(nodes, nodes[at], c, log)
            if at is None:
                return raised("raised")  # argmax of an empty list
            res = driver.step(cur, nodes[at].action)
            if res is None:
                out.broke_on_raise += 1
                break
            cur, _, done = res
            if done:
                out.broke_on_done += 1
                break
        # expansion (:271-279)
        node = nodes[at]
        tried = {nodes[j].action for j in node.children}
        untried = [a for a in possible_actions(node, P, port_cargo) if a not in tried]
        if untried:
            action = untried[driver.choice(len(untried))]
            res = driver.step(cur, action)
            if res is None:
                out.expansion_raised += 1
                continue
            cur, reward, _ = res
            child = Node(at, action, cur)
            child.total = float(reward)  # child.total_reward = reward (:145)
            nodes.append(child)
            node.children.append(len(nodes) - 1)
            depth[len(nodes) - 1] = depth[at] + 1
            out.depth = max(out.depth, depth[at] + 1)
            at = len(nodes) - 1
        # simulation and backpropagation (:282-285)
        ret, kind = driver.rollout(cur)
        if kind in ("raised", "never"):
            return raised(kind)
        if kind == "cut":
            out.status = CUT
        while at != NONE:
            nodes[at].visits += 1
            nodes[at].total += ret
            at = nodes[at].parent
    if nodes[0].children:
        out.action = nodes[best_child(nodes, nodes[0], 0.0, log)].action  # :288-290
        return out
    out.fallback = True
    res = driver.sample(ship)  # :292
    if isinstance(res, str):
        return raised(res)
    out.action = res
    return out


# ---------------------------------------------------------------------------- Philox driver
def sample_action(ship, world, r):
    """sample_action() (environment.py:245-263) from one 32-bit word r under the draw rules of
    se_sample_actions: a port by multiply-high over the others, an amount 1 + mulhi(r, stock),
    a move r & 3 of N, E, S, W."""
    x, y, fuel, cargo, _, dest = ship
    cur = next((i for i in range(world.P) if world.px[i] == x and world.py[i] == y), NONE)
    if dest == NONE and cur != NONE:
        if world.P < 2:
            return "never"
        k = (r * (world.P - 1)) >> 32
        return (SELECT, k + (k >= cur), 0)
    if cargo == 0 and cur != NONE:
        stock = int(world.pc[cur])
        return "raised" if stock < 1 else (TAKE_CARGO, 1 + ((r * stock) >> 32), 0)
    if fuel == 0 and cur != NONE:
        return "raised"
    return (MOVE,) + [(0, -1), (-1, 0), (0, 1), (1, 0)][r & 3]


class PhiloxDriver:
    """The draw contract of se_mcts_choose: simulation s draws from Philox(seed, id0 + s); tree
    step d reads (d, slot 18) (word 0 the choice, words 1-3 u_fuel, u_gate, u_type as w * 2^-32)
    and (d, slot 19) (Beta(2,2) = the median of three words, the new destination by
    multiply-high over the other ports); the rollout is oracle.rollout with rollout_base = id."""

    def __init__(self, O, world, seed, id0, max_steps, max_attempts):
        self.O, self.world, self.seed, self.id0 = O, world, seed, id0
        self.max_steps, self.max_attempts = max_steps, max_attempts
        self.id, self.d = id0, 0

    def _block(self, ident, t, slot):
        return [int(v) for v in self.O.philox([ident & M32, ident >> 32, t, slot],
                                              [self.seed & M32, self.seed >> 32])]

    def _state(self, ship):
        st = self.O.OracleState(1)
        st.x[0], st.y[0], st.fuel[0], st.cargo[0], st.origin[0], st.dest[0] = ship
        return st

    @staticmethod
    def _ship(st):
        return (int(st.x[0]), int(st.y[0]), float(st.fuel[0]), int(st.cargo[0]), int(st.origin[0]), int(st.dest[0]))

    def simulation(self, s):
        self.id, self.d = self.id0 + s, 0

    def choice(self, k):
        return (self._block(self.id, self.d, SLOT_TREE)[0] * k) >> 32

    def step(self, ship, action):
        O = self.O
        a, b = self._block(self.id, self.d, SLOT_TREE), self._block(self.id, self.d, SLOT_TREE_B)
        self.d += 1
        tape = np.zeros(1, O.TAPE_DTYPE)
        tape["u_fuel"], tape["u_gate"], tape["u_type"] = a[1] / 2.0**32, a[2] / 2.0**32, a[3] / 2.0**32
        tape["beta"] = sorted(b[:3])[1] / 2.0**32
        k = (b[3] * max(self.world.P - 1, 0)) >> 32
        tape["arrive_dest"] = k + (k >= ship[5])
        st = self._state(ship)
        O.step(self.world, st, act_type=[action[0]], act_a=[action[1]], act_b=[action[2]], tape=tape)
        if st.err[0] != 0:
            return None
        return self._ship(st), float(st.reward[0]), bool(st.done[0])

    def rollout(self, ship):
        ret, _, status, log = self.O.rollout(self.world, self._state(ship), [0], max_steps=self.max_steps,
                                             max_attempts=self.max_attempts, seed=self.seed,
                                             rollout_base=self.id, trace=True)
        if status[0] == 2:  # SE_ROLL_RAISED: which way sample_action failed, from where it stood
            end = (int(log["x"][0]), int(log["y"][0]), float(log["fuel"][0]), int(log["cargo"][0]),
                   int(log["origin"][0]), int(log["dest"][0]))
            return 0.0, sample_action(end, self.world, 0)
        return float(ret[0]), "cut" if status[0] == 3 else "ok"

    def sample(self, ship):
        return sample_action(ship, self.world, self._block(self.id0, M32, SLOT_TREE)[0])


def decide(O, world, ship, *, seed, id0, S, c, max_steps, max_attempts):
    """One env's decision under the contract; id0 = mcts_base + (the env's global id) * S is
    the id of its simulation 0."""
    drv = PhiloxDriver(O, world, seed, id0, max_steps, max_attempts)
    return choose_action(ship, world.P, [int(v) for v in world.pc], S, c, drv)


# ---------------------------------------------------------------------------- golden driver
class GoldenMismatch(AssertionError):
    pass


def ship_from_json(s):
    return (s[0], s[1], float.fromhex(s[2]), s[3], s[4], s[5])


class GoldenDriver:
    """Replays the events of one recorded decision, in order, and fails where the restatement
    asks for something else than the reference did."""

    def __init__(self, events):
        self.events, self.at = events, 0

    def _next(self, kind):
        if self.at >= len(self.events):
            raise GoldenMismatch(f"the restatement asks for a {kind} after the last recorded event")
        ev = self.events[self.at]
        self.at += 1
        if ev[0] != kind:
            raise GoldenMismatch(f"event {self.at - 1}: the reference did {ev[0]}, the restatement {kind}")
        return ev

    def simulation(self, s):
        pass

    def choice(self, k):
        ev = self._next("choice")
        if ev[1] != k:
            raise GoldenMismatch(f"choice over {k} untried actions, the reference had {ev[1]}")
        return ev[2]

    def step(self, ship, action):
        ev = self._next("step")
        if tuple(ev[1]) != tuple(action):
            raise GoldenMismatch(f"step {action}, the reference stepped {ev[1]}")
        if "raise" in ev[2]:
            return None
        return ship_from_json(ev[2]["ship"]), float.fromhex(ev[2]["reward"]), ev[2]["done"]

    def rollout(self, ship):
        ev = self._next("rollout")
        want = ship_from_json(ev[1])
        if want != ship:
            raise GoldenMismatch(f"rollout from {ship}, the reference's from {want}")
        if isinstance(ev[2], dict):
            return 0.0, "raised"
        return float.fromhex(ev[2]), "ok"

    def sample(self, ship):
        ev = self._next("sample")
        return "raised" if isinstance(ev[1], dict) else tuple(ev[1])


# ---------------------------------------------------------------------------- GPU scenarios
def ship(cell, origin, dest, cargo=0, fuel=100.0):
    return (cell[0], cell[1], fuel, cargo, origin, dest)


SEED = 9
MAX_STEPS, MAX_ATTEMPTS = 6, 11  # tight: a rollout whose sixth raising step comes before its sixth counted one is cut
REPS = 64  # env 64 * a + j is actor a in lane j of a wave
SIMS = (1, 4, 5, 17)

# name -> (world, [(label, ship, claims)]). A claim holds for some rep of the actor at some S
# of SIMS under SEED (tests/test_mcts_cpu.py shows it on the Philox-driver restatement):
#   ("depth", k) a node at depth >= k;  ("expansion_raised",);  ("broke_on_done",);
#   ("status", s) some decision ends with status s;  ("all", s) every one does;
#   ("never", s) none does;  ("wide_root",) the root has more possible actions than S;
#   ("children", type) the root's children are of that action type;  ("fallback",) the root
#   stayed without children.
# The maps are a few cells wide, so most ships meet an edge within a rollout and under the tight
# budget some of their rollouts are cut; every actor says whether SE_MCTS_CUT occurs on it
# (("status", CUT)) or on none of its envs (("never", CUT), ("all", s)): which envs are cut is
# part of what the GPU is compared on.
SCENARIOS = {
    "open": (OPEN, [
        # a fresh reset: at the origin port, bound elsewhere; four moves, then a second level
        ("fresh", ship((1, 1), 0, 1, fuel=200.0), [("depth", 2), ("children", MOVE), ("status", CUT)]),
        # at a port without destination: SELECT children
        ("select", ship((5, 6), 1, NONE), [("children", SELECT), ("depth", 2), ("status", CUT)]),
        # fuel exactly 0 on the origin port (stock 5): TAKE_CARGO children; with cargo aboard the
        # rollout's sample_action takes the TAKE_FUEL branch, which raises
        ("fuel_zero", ship((1, 1), 0, 1, fuel=0.0), [("children", TAKE_CARGO), ("all", RAISED), ("never", CUT)]),
        # the same at sea: every TAKE_CARGO raises, the root stays bare and the fallback moves
        ("fuel_zero_at_sea", ship((3, 3), 0, 1, fuel=0.0), [("expansion_raised",), ("fallback",), ("all", OK)]),
        # in the map's corner two of the four moves leave the map: abandoned simulations, and
        # rollouts that run out of attempts
        ("corner", ship((0, 0), 0, 1), [("expansion_raised",), ("status", CUT)]),
        # a move costs 0.9 .. 1.1: three in four report done, also as a selection step
        ("low_fuel", ship((3, 3), 0, 1, fuel=0.95), [("broke_on_done",), ("never", CUT)]),
        # loaded: the gate fires, partial losses draw the second block
        ("loaded", ship((3, 4), 0, 1, cargo=30), [("depth", 2), ("status", CUT)]),
        # one cell from the destination: arrivals in the tree steps
        ("next_to_dest", ship((5, 5), 0, 1, cargo=10), [("depth", 2), ("status", CUT)]),
    ]),
    "one": (ONE, [
        # one port, no destination: no possible action, np.argmax([]) raises
        ("one_port", ship((2, 3), 0, NONE), [("all", RAISED)]),
        ("one_port_at_sea", ship((2, 4), 0, NONE), [("all", RAISED)]),
    ]),
    "shared": (SHARED, [
        ("shared_select", ship((3, 3), 1, NONE), [("children", SELECT), ("status", CUT)]),
        ("shared_arrive", ship((3, 4), 2, 1, cargo=7), [("depth", 2), ("status", CUT)]),
    ]),
    "many": (MANY, [
        # 63 other ports: more possible actions than any S of SIMS
        ("wide", ship((1, 1), 0, NONE), [("wide_root",), ("children", SELECT), ("status", CUT)]),
        ("many_fresh", ship((5, 6), 49, 3, fuel=200.0), [("depth", 2), ("never", CUT)]),
    ]),
}


TAIL = 3  # envs past the last whole wave: n = 64 k + 3


def scenario_actors(name, reps=REPS):
    """The actor index of every env of the scenario's table: each actor `reps` times in a row,
    then the first TAIL actors (cyclically) once more."""
    k = len(SCENARIOS[name][1])
    return [a for a in range(k) for _ in range(reps)] + [j % k for j in range(TAIL)]


def scenario_ships(name, reps=REPS):
    return [SCENARIOS[name][1][a][1] for a in scenario_actors(name, reps)]


_DECISIONS = {}


def decisions(O, name, S, *, reps=REPS, mcts_base=0, env_id_base=0, c=1.4, max_steps=MAX_STEPS,
              max_attempts=MAX_ATTEMPTS):
    """The restatement's decision for every env of the scenario table (computed once per
    argument set and shared: callers leave it unchanged)."""
    key = (name, S, reps, mcts_base, env_id_base, c, max_steps, max_attempts)
    if key not in _DECISIONS:
        world = SCENARIOS[name][0].oracle(O)
        _DECISIONS[key] = [
            decide(O, world, sh, seed=SEED, id0=mcts_base + (env_id_base + i) * S, S=S, c=c,
                   max_steps=max_steps, max_attempts=max_attempts)
            for i, sh in enumerate(scenario_ships(name, reps))]
    return _DECISIONS[key]


def assert_claims(O, name):
    """Show on the restatement that every actor of the scenario holds what it claims; returns
    the set of statuses seen."""
    rows = SCENARIOS[name][1]
    runs = {S: decisions(O, name, S) for S in SIMS}
    seen = set()
    for a, (label, _, claims) in enumerate(rows):
        mine = [(S, d) for S in SIMS for d, who in zip(runs[S], scenario_actors(name)) if who == a]
        seen |= {d.status for _, d in mine}
        for claim in claims:
            kind, arg = claim[0], claim[-1]
            if kind == "depth":
                assert any(d.depth >= arg for _, d in mine), f"{label}: no node at depth {arg}"
            elif kind == "expansion_raised":
                assert any(d.expansion_raised for _, d in mine), f"{label}: no expansion raised"
            elif kind == "broke_on_done":
                assert any(d.broke_on_done for _, d in mine), f"{label}: no selection broke on done"
            elif kind == "status":
                assert any(d.status == arg for _, d in mine), f"{label}: status {arg} never occurs"
            elif kind == "all":
                assert all(d.status == arg for _, d in mine), f"{label}: not every status is {arg}"
            elif kind == "never":
                assert all(d.status != arg for _, d in mine), f"{label}: status {arg} occurs"
            elif kind == "wide_root":
                assert all(d.root_possible > S for S, d in mine), f"{label}: the root is not wider than S"
            elif kind == "children":
                kids = {d.nodes[j].action[0] for _, d in mine for j in d.nodes[0].children}
                assert kids == {arg}, f"{label}: root children of types {kids}"
            elif kind == "fallback":
                assert all(d.fallback for _, d in mine), f"{label}: the root got children"
            else:
                raise KeyError(kind)
    return seen
