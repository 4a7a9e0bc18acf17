"""The navigator restated on the CPU, for tests/test_nav_cpu.py and tests/test_gpu_nav.py.

Plain Python: a deque breadth-first pass per port over the non-ground cells (ports stamped
non-ground), the direction rule, the policy nav_action and the rollout nav_rollout, which steps a
private ship through plan_support.Stepper: position k of the rollout with id `ident` draws what
se_rollout_plan's position k draws, so the action list a navigated rollout emitted, played as a
plan, must give the same Result (tests/test_nav_cpu.py shows it).

A ship is the tuple (x, y, fuel, cargo, origin, dest) with NONE = -1; a typed action is
(type, a, b). Cell (x, y) has x the map row; the moves are the agent index's, k = 0..3 =
N (0,-1), E (-1,0), S (0,1), W (1,0) applied to (x, y)."""
from collections import deque

import numpy as np

import plan_support as PS
import rollout_support as RS

NONE = -1
INF, NO_DIR = 0xFFFF, 255  # SE_NAV_INF, SE_NAV_NONE
OK, NO_DEST, UNREACHABLE = 0, 1, 2  # SE_NAV_*
STUCK = 5  # SE_PLAN_STUCK
MOVES = ((0, -1), (-1, 0), (0, 1), (1, 0))
NO_ACTION = (0, 0, 0)


# ---------------------------------------------------------------------------- worlds
def _world(H, W, ports, fuel, cargo, ground=()):
    return RS.World(H, W, ports=ports, fuel=fuel, cargo=cargo, ground=ground)


def _lake():
    """7 x 9: a ground ring around a 3 x 3 pocket that holds port 1; ports 0 and 2 outside; the
    water cell (3, 7) walled in alone at the map's edge."""
    ring = [(x, y) for x in range(1, 6) for y in range(1, 6) if x in (1, 5) or y in (1, 5)]
    return _world(7, 9, [(0, 7), (3, 3), (6, 7)], [9, 4, 7], [5, 6, 8], ground=ring + [(2, 7), (4, 7), (3, 6), (3, 8)])


def _snake():
    """256 x 256 serpentine: the even rows are water, an odd row is ground but for one cell at
    alternating ends. Port 0 at the head, port 1 at the tail: a long field in the largest map."""
    ground = [(x, y) for x in range(1, 256, 2) for y in range(256) if y != (255 if x % 4 == 1 else 0)]
    return _world(256, 256, [(0, 0), (254, 0)], [9, 9], [5, 5], ground=ground)


LAKE = _lake()
# a ground wall in column 4 with its gap in the last row: from (2, 3) port 1 lies east, the way south-about
WALL = _world(5, 9, [(2, 1), (2, 7)], [9, 4], [5, 6], ground=[(x, 4) for x in range(4)])
ROW = _world(1, 12, [(0, 1), (0, 10)], [9, 4], [5, 6])
COL = _world(12, 1, [(1, 0), (10, 0), (5, 0)], [9, 4, 7], [5, 6, 8])
DOT = _world(1, 1, [(0, 0)], [6], [3])
_SNAKE = []


def snake():
    if not _SNAKE:
        _SNAKE.append(_snake())
    return _SNAKE[0]


SMALL = {"lake": LAKE, "wall": WALL, "row": ROW, "col": COL, "dot": DOT, "open": RS.OPEN, "one": RS.ONE,
         "shared": RS.SHARED, "many": RS.MANY}


def default_world(water, seed=0):
    """The builtin map with the default ports and the stocks VecEnv draws for `seed`."""
    import random

    rng = random.Random(seed)
    fuel, cargo = [], []
    for _ in range(5):
        fuel.append(rng.randint(5, 20))
        cargo.append(rng.randint(5, 20))
    ports = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]
    w = _world(water.shape[0], water.shape[1], ports, fuel, cargo)
    w.water = np.ascontiguousarray(water, np.uint8)
    return w


# ---------------------------------------------------------------------------- tables
def open_mask(world):
    """True where a ship may stand: water, and every port's cell."""
    m = np.asarray(world.water) != 0
    for x, y in world.ports:
        m[x, y] = True
    return m


def bfs(mask, start):
    """Moves from every cell to `start` over True cells of mask, INF where there is no way."""
    H, W = mask.shape
    f = np.full((H, W), INF, np.int64)
    f[start] = 0
    todo = deque([start])
    while todo:
        x, y = todo.popleft()
        for dx, dy in MOVES:
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and mask[nx, ny] and f[nx, ny] == INF:
                f[nx, ny] = f[x, y] + 1
                todo.append((nx, ny))
    return f


def directions(f):
    """The direction rule on one port's field: the lowest k whose in-map neighbour has the
    smallest finite value, NO_DIR where none is finite."""
    H, W = f.shape
    d = np.full((H, W), NO_DIR, np.int64)
    for x in range(H):
        for y in range(W):
            best = INF
            for k, (dx, dy) in enumerate(MOVES):
                nx, ny = x + dx, y + dy
                if 0 <= nx < H and 0 <= ny < W and f[nx, ny] < best:
                    best, d[x, y] = f[nx, ny], k
    return d


def components(mask):
    """Labels of the 4-connected components of mask's True cells (-1 elsewhere) and their count."""
    H, W = mask.shape
    lab = np.full((H, W), -1, np.int64)
    n = 0
    for x in range(H):
        for y in range(W):
            if mask[x, y] and lab[x, y] < 0:
                lab[bfs(mask, (x, y)) < INF] = n
                n += 1
    return lab, n


class Tables:
    """A world's route tables, each port's made when first asked for."""

    def __init__(self, world):
        self.world, self.mask = world, open_mask(world)
        self._f, self._d = {}, {}

    def field(self, p):
        if p not in self._f:
            self._f[p] = bfs(self.mask, tuple(self.world.ports[p]))
        return self._f[p]

    def dir(self, p):
        if p not in self._d:
            self._d[p] = directions(self.field(p))
        return self._d[p]

    def fields(self):
        return np.array([self.field(p) for p in range(self.world.P)], np.uint16).reshape(self.world.P, *self.mask.shape)

    def dirs(self):
        return np.array([self.dir(p) for p in range(self.world.P)], np.uint8).reshape(self.world.P, *self.mask.shape)

    def max_leg(self):
        legs = [self.field(p)[tuple(q)] for p in range(self.world.P) for q in self.world.ports]
        return max([int(v) for v in legs if v < INF] + [0])


_TABLES = {}


def tables(world):
    if id(world) not in _TABLES:
        _TABLES[id(world)] = (world, Tables(world))
    return _TABLES[id(world)][1]


# ---------------------------------------------------------------------------- the policy
def port_at(world, x, y):
    for i, p in enumerate(world.ports):
        if (p[0], p[1]) == (x, y):
            return i
    return -1


def nav_action(world, tab, ship, refuel_below, load):
    """-> (action, status, dist): the policy of include/shipenv.h, its rules in order."""
    x, y, fuel, cargo, origin, dest = ship
    if not (0 <= x < world.H and 0 <= y < world.W):
        return NO_ACTION, UNREACHABLE, -1
    cur = port_at(world, x, y)
    if dest == NONE:
        best, pick = INF, -1
        if cur >= 0:
            for q in range(world.P):
                f = int(tab.field(q)[x, y])
                if q != origin and 0 < f < best:
                    best, pick = f, q
        return ((2, pick, 0), OK, -1) if pick >= 0 else (NO_ACTION, NO_DEST, -1)
    if not 0 <= dest < world.P:
        return NO_ACTION, UNREACHABLE, -1
    f = int(tab.field(dest)[x, y])
    dist = -1 if f == INF else f
    if cur >= 0:
        if fuel < refuel_below and world.fuel_stock[cur] >= 1:
            return (3, int(world.fuel_stock[cur]), 0), OK, dist
        if cargo == 0 and load > 0 and world.cargo_stock[cur] >= 1:
            return (4, min(load, int(world.cargo_stock[cur])), 0), OK, dist
    k = int(tab.dir(dest)[x, y])
    if k == NO_DIR:
        return NO_ACTION, UNREACHABLE, dist
    return (1,) + MOVES[k], OK, dist


def agent_index(P, action, status):
    """The agent index that decodes to the action (utils/preprocessing.py:111-137), -1 where the
    navigator has none or the amount has no index (the index holds cargo 0..49, fuel 0..199)."""
    ty, a, b = action
    if status != OK:
        return -1
    if ty == 1:
        return MOVES.index((a, b))
    if ty == 2:
        return 4 + a
    if ty == 4:
        return 4 + P + a if a <= 49 else -1
    return 54 + P + a if a <= 199 else -1


class NavRollout:
    """One navigated rollout: `res` as plan_support.Result has it (status STUCK added), the
    arrivals, why and where the navigator had no action, and the actions it emitted."""
    __slots__ = ("res", "arrivals", "nav_status", "stuck_at", "actions")


def nav_rollout(O, world, ship, steps, refuel_below, load, seed, ident, stepper=None, tab=None):
    """The navigated rollout of `steps` positions from `ship` under Philox(seed, ident). tab: other
    tables than the restated ones of `world` (anything with Tables' field(p) and dir(p))."""
    sp = stepper or PS.Stepper(O, world.oracle(O), seed)
    tab = tab or tables(world)
    out = NavRollout()
    out.res, out.arrivals, out.nav_status, out.stuck_at, out.actions = PS.Result(ship), 0, OK, -1, []
    res = out.res
    for k in range(steps):
        act, status, _ = nav_action(world, tab, ship, refuel_below, load)
        if status != OK:
            res.status, out.nav_status, out.stuck_at = STUCK, status, k
            break
        out.actions.append(act)
        err, ship, rw, done, used = sp.step(ship, act, ident, k)
        if err:
            if res.raised == 0:
                res.first_err, res.first_err_at = err, k
            res.raised += 1
            continue
        res.ret += rw
        res.steps += 1
        res.used |= used
        out.arrivals += 1 if used & PS.USED_ARRIVE else 0
        if done:
            res.status = PS.DONE
            break
    res.ship = ship
    return out
