"""Generate the step-edge fixture: what the reference's step does at the edges of its
arguments and of its variates.

TEST INFRASTRUCTURE. Like make_golden.py it runs only in the build container (it imports
the reference from /root/reference with ``cv2stub`` on the path); its outputs are the two
small committed files next to it. Usage:

    python tests/golden/make_step_edge_golden.py   # rewrites step_edges.npz, step_edges_meta.json

make_golden.py samples at random from a narrow box (moves of at most +-4, cargo 0..90, one
100x100 map, variates straight from random.Random), so no recorded variate sits on a
comparison boundary and no argument leaves the box. This generator enumerates the edges by
hand instead: a record is (world, pre-state, action, variates), the reference's
``Environment.step`` is run on it with a scripted ``random`` that returns exactly the
record's variates, and the outcome (post-state, reward, done, error class, which draws
were made) is stored. A step is a pure function of the record, so the C oracle, the host
build of the step and the kernels must each reproduce every record bit for bit.

Worlds are made by assigning ``size_game``, ``np_game`` and the port lists on a constructed
Environment (no resize). They are square (the reference is defective for non-square maps,
tests/test_reference_quirks.py), of side 1, 2, 3, 100 and 256, with ground next to ports
and on the map edge, ports on corners and edges, two ports on one cell, and stocks 1, 50,
200 and 2^30. A sixth world has no ports.

Columns: FIELDS_I32 / FIELDS_F64 of make_golden.py (pre_cargo / post_cargo as int64: the
reference's ints are unbounded) plus
  world            index of the record's world (tables w{k}_water, w{k}_port_*)
  raw_a, raw_b     the action's integers as given to the reference (int64); act_a / act_b
                   are these clamped to int32, the form the drop-in hands the stepper
  n_draws          calls the reference made on ``random`` (each randint of a redraw counts)
  draw_kinds       SE_USED_* bits of those calls: 1 uniform + gate random, 2 loss-type
                   random, 4 betavariate, 8 randint
  used             draw_kinds | 16 where the ship moved onto a non-ground cell: what
                   se_tape.used must equal
  reward_is_int, pre_fuel_is_int, post_fuel_is_int   the Python types
  beyond_contract  1 where the cargo is outside the int32 contract of include/shipenv.h
                   (|cargo| or |cargo + amount| above (2^31 - 1) / 3): recorded, not tested

Left out: NaN fuel. The reference's result there is a NaN whose sign and payload depend on
the operand order of the platform's subtraction, which the fixture cannot pin as bits.
"""
from __future__ import annotations

import io
import json
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "cv2stub"))
sys.path.insert(0, REF)

import shipping.environment as ref_env  # noqa: E402
from shipping import Environment  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import ERRORS, FIELDS_F64, FIELDS_I32, agent_index  # noqa: E402

MAP = os.path.join(REF, "mapa_mundi_binario.jpg")
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
BOUND = I32_MAX // 3  # 715827882: the largest cargo for which 3 * loss is exact in int32
BIG = 2 ** 30         # the large stock
NAN = math.nan
EDGE = [I32_MIN, -257, -256, -255, -1, 0, 1, 255, 256, 257, I32_MAX]
GROUND, BOAT = 0, 5


def clamp32(v):
    return I32_MIN if v < I32_MIN else (I32_MAX if v > I32_MAX else v)


def up(v):
    return math.nextafter(v, math.inf)


def down(v):
    return math.nextafter(v, -math.inf)


# ------------------------------------------------------------------ scripted random
class Scripted:
    """Drop-in for the ``random`` module as shipping/environment.py uses it: returns the
    variates of the record at hand and logs the calls."""

    def __init__(self):
        self.log = []
        self.v = None

    def load(self, u_fuel, u_gate, u_type, beta, arrive):
        self.v = {"uniform": [u_fuel], "random": [u_gate, u_type], "beta": [beta], "randint": list(arrive)}
        self.log = []

    def _next(self, kind):
        self.log.append(kind)
        return self.v[kind].pop(0)  # IndexError: the record did not supply this draw

    def uniform(self, a, b):  # CPython Lib/random.py: a + (b - a) * self.random()
        return a + (b - a) * self._next("uniform")

    def random(self):
        return self._next("random")

    def betavariate(self, a, b):
        return self._next("beta")

    def randint(self, a, b):
        v = self._next("randint")
        assert a <= v <= b
        return v


# ------------------------------------------------------------------ worlds
def _world(side, ground, ports, fuel, cargo):
    water = np.ones((side, side), np.uint8)
    for c in ground:
        water[c] = 0
    return {"side": side, "water": water, "ports": [list(p) for p in ports], "fuel": fuel, "cargo": cargo}


def make_worlds():
    g100 = [(0, y) for y in range(40, 60)] + [(x, 99) for x in range(10, 31)]
    g100 += [(x, y) for x in range(30, 36) for y in range(30, 36)]
    g100 += [(0, 1), (98, 99), (50, 1), (61, 22), (60, 21), (11, 11)]
    # 256: ground stripes on rows 8, 24, 40, ... (three cells of four), and by hand next to
    # the ports and on the edge
    g256 = [(x, y) for x in range(8, 256, 16) for y in range(256) if y % 4]
    g256 += [(0, 1), (1, 255), (254, 255), (255, 2), (127, 0), (128, 127), (0, 100), (255, 200)]
    return [
        _world(1, [], [(0, 0), (0, 0)], [1, 50], [50, 1]),
        _world(2, [(0, 1)], [(0, 0), (1, 1), (1, 1)], [1, 50, 200], [200, 1, 50]),
        _world(3, [(0, 1), (2, 0)], [(0, 0), (2, 2), (1, 2), (1, 2)], [1, 50, 200, BIG], [BIG, 200, 50, 1]),
        _world(100, g100, [(0, 0), (99, 99), (50, 0), (60, 22), (60, 22)],
               [1, 50, 200, BIG, 7], [50, 1, BIG, 200, 9]),
        _world(256, g256, [(0, 0), (255, 255), (255, 0), (0, 255), (128, 0), (128, 128), (128, 128), (1, 1)],
               [1, 50, 200, BIG, 5, 20, 13, 9], [20, 5, 1, 50, BIG, 200, 17, 6]),
        _world(3, [(1, 1)], [], [], []),  # no ports: every step raises "No ports available"
    ]


def make_env(w):
    env = Environment(MAP)
    s = w["side"]
    env.size_game = (s, s)
    g = w["water"].astype(int)
    for p in w["ports"]:
        g[p[0], p[1]] = 2  # Entity.PORT, as add_port stamps it
    env.np_game = g
    env.port_positions = [list(p) for p in w["ports"]]
    env.port_fuel = list(w["fuel"])
    env.port_cargo = list(w["cargo"])
    return env


# ------------------------------------------------------------------ records
EXTRA_I32 = ["world", "n_draws", "draw_kinds", "used", "reward_is_int", "pre_fuel_is_int", "beyond_contract"]
EXTRA_I64 = ["raw_a", "raw_b", "pre_cargo", "post_cargo"]


class Book:
    def __init__(self, worlds):
        self.worlds = worlds
        self.envs = [make_env(w) for w in worlds]
        self.rng = Scripted()
        ref_env.random = self.rng
        names = [f for f in FIELDS_I32 + FIELDS_F64 + EXTRA_I32 + EXTRA_I64]
        self.cols = {k: [] for k in dict.fromkeys(names)}
        self.tags = {}
        self.seen = set()

    def tag(self, *names):
        for n in names:
            self.tags[n] = self.tags.get(n, 0) + 1

    def add(self, w, pos, fuel, cargo, origin, dest, act_type, a, b=0, *, u_fuel=0.5, u_gate=0.5,
            u_type=0.5, beta=0.5, loop=False, tags=()):
        """Run one record through the reference and store it. loop: the arrival redraw first
        returns the new origin twice (the reference draws again), then another port."""
        key = (w, tuple(pos), repr(fuel), type(fuel).__name__, cargo, origin, dest, act_type, a, b,
               repr(u_fuel), repr(u_gate), repr(u_type), repr(beta), loop)
        if key in self.seen:  # the hand-written products overlap here and there
            self.tag(*tags)
            return None
        self.seen.add(key)
        env, world = self.envs[w], self.worlds[w]
        P = len(world["ports"])
        x, y = pos
        env.ship_position = [x, y]
        env.fuel, env.cargo = fuel, cargo
        env.origin_port_index, env.destination_port_index = origin, dest
        other = (dest + 1) % P if (dest is not None and P > 1) else 0
        self.rng.load(u_fuel, u_gate, u_type, beta, [dest, dest, other] if loop else [other])
        side = world["side"]
        cells = [(x, y)]
        if act_type == 1 and 0 <= x + a < side and 0 <= y + b < side:
            cells.append((x + a, y + b))
        saved = [int(env.np_game[c]) for c in cells]
        err, reward, done = 0, 0, False
        try:
            _, reward, done, _ = env.step([act_type, (a, b) if act_type == 1 else a])
        except Exception as e:  # noqa: BLE001 - exceptions are the reference's control flow
            err = ERRORS[(type(e).__name__, str(e))]
        log = self.rng.log
        moved = act_type == 1 and err == 0 and int(env.np_game[cells[-1]]) == BOAT
        for c, v in zip(cells, saved):
            env.np_game[c] = v
        assert log == ["uniform", "random", "random", "beta"][:len([k for k in log if k != "randint"])] + \
            ["randint"] * log.count("randint"), log
        kinds = (1 if "uniform" in log else 0) | (2 if log.count("random") == 2 else 0) | \
            (4 if "beta" in log else 0) | (8 if "randint" in log else 0)
        px, py = env.ship_position
        c = self.cols
        post_cargo = int(env.cargo)
        beyond = abs(cargo) > BOUND or abs(post_cargo) > BOUND
        row = {
            "kind": 2 if P == 0 else 0, "act_type": clamp32(act_type), "act_a": clamp32(a), "act_b": clamp32(b),
            "agent_idx": agent_index(act_type, a, b, P),
            "pre_x": x, "pre_y": y, "pre_origin": -1 if origin is None else origin,
            "pre_dest": -1 if dest is None else dest,
            "post_x": int(px), "post_y": int(py),
            "post_origin": -1 if env.origin_port_index is None else env.origin_port_index,
            "post_dest": -1 if env.destination_port_index is None else env.destination_port_index,
            "arrive_dest": other if kinds & 8 else -1, "reset_origin": -1, "reset_dest": -1,
            "err": err, "done": int(bool(done)), "post_fuel_is_int": int(isinstance(env.fuel, int)),
            "pre_fuel": float(fuel), "post_fuel": float(env.fuel),
            "u_fuel": u_fuel if kinds & 1 else NAN, "u_gate": u_gate if kinds & 1 else NAN,
            "u_type": u_type if kinds & 2 else NAN, "beta": beta if kinds & 4 else NAN,
            "reward": float(reward),
            "world": w, "n_draws": len(log), "draw_kinds": kinds, "used": kinds | (16 if moved else 0),
            "reward_is_int": int(isinstance(reward, int)), "pre_fuel_is_int": int(isinstance(fuel, int)),
            "beyond_contract": int(beyond),
            "raw_a": a, "raw_b": b, "pre_cargo": cargo, "post_cargo": post_cargo,
        }
        for k, v in row.items():
            c[k].append(v)
        # classes that can be read off the record
        t = [f"world_side_{side}" if P else "world_no_ports", f"err_{err}"] + list(tags)
        if beyond:
            t.append("beyond_contract")
        if act_type == 1:
            for v in (a, b):
                if v in EDGE:
                    t.append(f"move_component_{v}")
            if a != clamp32(a) or b != clamp32(b):
                t.append("move_beyond_int32_clamped")
            on_port = [x, y] in world["ports"]
            if (a, b) == (0, 0):
                t.append("move_zero_on_port" if on_port else "move_zero_off_port")
            if err == 0:
                t.append("move_moved" if moved else "move_blocked_by_ground")
                if max(abs(a), abs(b)) > 1:
                    tgt = [x + a, y + b]
                    if not moved:
                        t.append("long_jump_onto_ground")
                    elif tgt == world["ports"][dest]:
                        t.append("long_jump_onto_destination")
                    elif tgt in world["ports"]:
                        t.append("long_jump_onto_other_port")
                    else:
                        t.append("long_jump_onto_water")
                if done:
                    t.append("fuel_out")
                if kinds & 8:
                    t.append("arrival")
                    if not moved:
                        t.append("arrival_while_blocked")
                if kinds & 2:
                    t.append("gate_fired")
                if kinds & 4:
                    t.append("beta_drawn")
            if dest is None:
                t.append("dest_none_move_out_of_range" if not len(cells) == 2 else "dest_none_move_in_range")
        elif dest is None:
            t.append("dest_none_other_action")
        self.tag(*t)
        return row


def enumerate_records(bk):
    W = bk.worlds
    add = bk.add

    # ---- MOVE (a, b) over the argument edges, from corners, edge cells and around ports
    starts = {
        0: [(0, 0)],
        1: [(x, y) for x in range(2) for y in range(2)],
        2: [(x, y) for x in range(3) for y in range(3)],
        3: [(0, 0), (99, 99), (0, 99), (99, 0), (50, 0), (0, 50), (99, 50), (50, 99), (60, 22), (60, 23),
            (59, 22), (49, 49)],
        4: [(0, 0), (255, 255), (255, 0), (0, 255), (128, 0), (0, 128), (255, 128), (128, 255), (128, 128),
            (127, 128), (128, 129), (1, 0), (254, 254)],
    }
    dests = {0: [1], 1: [1, 2], 2: [1, 3], 3: [1, 4], 4: [1, 6]}
    for w in range(5):
        for d in dests[w]:
            for pos in starts[w]:
                for a in EDGE:
                    for b in EDGE:
                        add(w, pos, 200, 0, 0, d, 1, a, b)
    # mid-range jumps: onto the destination, another port, ground, and over ground onto water
    for w, pos, mv, d in [
        (3, (0, 0), (99, 99), 1), (3, (0, 0), (50, 0), 1), (3, (0, 0), (60, 22), 4), (3, (0, 0), (60, 22), 1),
        (3, (0, 0), (0, 45), 1), (3, (0, 0), (32, 32), 1), (3, (0, 0), (15, 15), 1), (3, (0, 0), (36, 36), 1),
        (3, (99, 99), (-99, -99), 0), (3, (99, 99), (-49, -99), 2), (3, (49, 49), (3, -4), 1),
        (3, (49, 49), (-3, 4), 1), (3, (60, 23), (0, -2), 1), (3, (99, 0), (-99, 99), 1),
        (4, (0, 0), (128, 128), 5), (4, (0, 0), (128, 128), 6), (4, (0, 0), (128, 0), 1), (4, (0, 0), (8, 1), 1),
        (4, (0, 0), (9, 1), 1), (4, (0, 0), (8, 4), 1), (4, (0, 0), (255, 1), 1), (4, (0, 0), (1, 255), 1),
        (4, (255, 255), (-127, -127), 5), (4, (255, 255), (-254, -254), 7), (4, (0, 255), (255, -255), 2),
        (4, (255, 0), (-255, 255), 3), (4, (255, 255), (-255, -255), 0), (4, (128, 128), (127, 127), 1),
        (4, (128, 128), (-128, -128), 0), (4, (1, 0), (254, 255), 1), (4, (1, 0), (-1, 0), 0),
    ]:
        for cargo in (0, 30):
            add(w, pos, 400.5, cargo, 0 if d else 1, d, 1, mv[0], mv[1], tags=("move_mid_range_jump",))
    # a Python int beyond int32: the reference sees the unclamped value, the stepper the clamp
    for w, pos in ((3, (49, 49)), (4, (0, 0)), (2, (1, 1))):
        for a, b in ((2 ** 40, -2 ** 40), (2 ** 31, 0), (0, -2 ** 31 - 1), (-2 ** 62, 2 ** 62), (2 ** 31, 2 ** 31)):
            add(w, pos, 200, 3, 0, 1, 1, a, b)
    # (0, 0) on and off a port, with the fuels a zero cost is compared to
    for w, pos, d in ((3, (99, 99), 1), (3, (60, 22), 1), (3, (49, 49), 1), (3, (60, 22), 4), (0, (0, 0), 1),
                      (4, (128, 128), 6), (2, (0, 1), 1)):
        for fuel in (-0.0, 0.0, 5e-324, 200, math.inf):
            add(w, pos, fuel, 7, 0, d, 1, 0, 0, tags=("move_zero_fuel_edges",))

    # ---- scenarios on the 100 and 256 worlds for the variate products
    #   (world, start, move, origin, dest): onto water, into ground, onto the destination, and
    #   into ground while already standing on the destination
    WATER = (3, (10, 10), (1, 0), 0, 1)
    BLOCK = (3, (0, 0), (0, 1), 2, 1)
    ARRIVE = (3, (99, 98), (0, 1), 0, 1)
    ARRIVE_BLOCKED = (3, (0, 0), (0, 1), 1, 0)
    FAR = (3, (0, 0), (15, 15), 0, 1)
    FAR256 = (4, (0, 0), (255, 255), 0, 1)

    def go(sc, fuel, cargo, **kw):
        w, pos, mv, o, d = sc
        return add(w, pos, fuel, cargo, o, d, 1, mv[0], mv[1], **kw)

    # fuel against the cost: u_fuel on its boundaries, fuel on and around the cost
    for sc in (WATER, BLOCK, ARRIVE, FAR, FAR256):
        a, b = sc[2]
        for name, u in (("u_fuel_0", 0.0), ("u_fuel_2^-53", 2.0 ** -53), ("u_fuel_1-2^-53", 1.0 - 2.0 ** -53),
                        ("u_fuel_mid", 0.5)):
            # the reference's own expression for the cost (:103-104 with CPython's uniform)
            cost = float(ref_env.calculate_euclidean_distance([0, 0], [a, b]) * (1 + (-0.1 + (0.1 - -0.1) * u)))
            for fname, fuel in (("fuel_-0.0", -0.0), ("fuel_0.0", 0.0), ("fuel_5e-324", 5e-324),
                                ("fuel_eq_cost", cost), ("fuel_cost_minus_ulp", down(cost)),
                                ("fuel_cost_plus_ulp", up(cost)), ("fuel_int_200", 200), ("fuel_200.0", 200.0),
                                ("fuel_1e300", 1e300), ("fuel_inf", math.inf)):
                for cargo in (0, 30):
                    r = go(sc, fuel, cargo, u_fuel=u, tags=(name, fname))
                    if r is not None and fname == "fuel_eq_cost":
                        assert r["done"] == 0 and (r["post_fuel"] == 0.0 or sc is BLOCK), r
                    if r is not None and fname == "fuel_cost_minus_ulp":
                        assert r["done"] == 1, r

    # cargo x gate x (loss type | beta)
    cargos = [-7, -1, 0, 1, 24, 25, 49, 50, 51, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 24 + 1,
              BOUND - 1, BOUND, -BOUND]
    gates = [("u_gate_0.0", 0.0), ("u_gate_1-2^-53", 1.0 - 2.0 ** -53)]
    for c in (1, 25, 49):
        f = c / 50
        gates += [(f"u_gate_prev_{c}/50", down(f)), (f"u_gate_{c}/50", f), (f"u_gate_next_{c}/50", up(f))]
    types = [("u_type_0.0", 0.0), ("u_type_prev_0.1", down(0.1)), ("u_type_0.1", 0.1), ("u_type_next_0.1", up(0.1)),
             ("u_type_prev_0.9", down(0.9)), ("u_type_0.9", 0.9), ("u_type_next_0.9", up(0.9))]
    betas = [("beta_0.0", 0.0), ("beta_2^-30", 2.0 ** -30), ("beta_1/3", 1 / 3), ("beta_1-2^-53", 1.0 - 2.0 ** -53)]
    for i, sc in enumerate((WATER, BLOCK, ARRIVE, ARRIVE_BLOCKED, FAR256)):
        for cargo in cargos:
            for gname, ug in gates:
                for tname, ut in types:
                    go(sc, 150.25, cargo, u_gate=ug, u_type=ut, beta=1 / 3, loop=bool(i & 1) ^ (cargo == 25),
                       tags=(f"cargo_{cargo}", gname, tname))
                for bname, bv in betas:
                    go(sc, 150.25, cargo, u_gate=ug, u_type=0.5, beta=bv, tags=(f"cargo_{cargo}", gname, bname))
    # the record of the issue: negative cargo with a gate draw of exactly 0.0
    add(3, (10, 10), 150.25, -5, 0, 1, 1, 1, 0, u_gate=0.0, u_type=0.5, beta=0.5,
        tags=("negative_cargo_gate_0.0",))
    for cargo in (-7, -1, -BOUND):
        for sc in (WATER, BLOCK, ARRIVE, FAR256):
            go(sc, 150.25, cargo, u_gate=0.0, tags=("negative_cargo_gate_0.0",))

    # beta * cargo one ulp either side of an integer
    for cargo in (3, 49, 51, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 24 + 1, BOUND):
        for k in sorted({1, cargo // 3, cargo // 2 + 1, cargo - 1}):
            if not 0 < k < cargo:
                continue
            lo = hi = ab = None
            cand = k / cargo
            for _ in range(64):
                cand = down(cand)
            for _ in range(128):
                p = cand * cargo
                if p == down(float(k)):
                    lo = cand
                if p == float(k) and hi is None:
                    hi = cand
                if p == up(float(k)) and ab is None:
                    ab = cand
                cand = up(cand)
            for name, bv in (("beta_product_ulp_below_integer", lo), ("beta_product_on_integer", hi),
                             ("beta_product_ulp_above_integer", ab)):
                if bv is None:
                    continue
                for sc in (WATER, ARRIVE):
                    r = go(sc, 150.25, cargo, u_gate=0.0, u_type=0.5, beta=bv, tags=(name,))
                    if r is not None and sc is WATER:
                        assert r["pre_cargo"] - r["post_cargo"] == (k - 1 if bv is lo else k), (cargo, k, r)

    # beyond the int32 contract: recorded for the record, skipped by the tests (few on purpose)
    for cargo in (BOUND + 1, 2 ** 30, 2 ** 30 + 5, -BOUND - 1, I32_MAX, I32_MIN):
        for sc in (WATER, ARRIVE):
            for ut in (0.05, 0.5, 0.95):
                go(sc, 150.25, cargo, u_gate=0.5, u_type=ut, beta=1 / 3)

    # ---- SELECT_PORT
    for w in range(5):
        P = len(W[w]["ports"])
        pos = starts[w][0]
        for origin in (0, P - 1, None):
            vals = [I32_MIN, -1, 0, 1, P - 1, P, 255, 256, I32_MAX, 2 ** 40, -2 ** 40]
            if origin is not None:
                vals.append(origin)
            for a in vals:
                for dest in (0, None):
                    name = {I32_MIN: "min", -1: "-1", 0: "0", P - 1: "P-1", P: "P", 255: "255", 256: "256",
                            I32_MAX: "max"}.get(a, "other")
                    tg = [f"select_{name}"]
                    if a == origin:
                        tg.append("select_origin")
                    add(w, pos, 200, 5, origin, dest, 2, a, tags=tg)

    # ---- TAKE_CARGO / TAKE_FUEL: at every port cell (the first port of a shared cell wins),
    # and off port on water and on ground
    for w in range(5):
        ports, side = W[w]["ports"], W[w]["side"]
        cells = []
        for p in ports:
            if tuple(p) not in cells:
                cells.append(tuple(p))
        off = [c for c in starts[w] + [(0, 1), (1, 0)] if list(c) not in ports and max(c) < side][:3]
        for act_type, stocks, nm in ((4, W[w]["cargo"], "take_cargo"), (3, W[w]["fuel"], "take_fuel")):
            for cell in cells + off:
                here = [i for i, p in enumerate(ports) if tuple(p) == cell]
                amounts = {I32_MIN: "min", -1: "-1", 0: "0", 1: "1", I32_MAX: "max", 2 ** 40: "other"}
                for i in here:
                    amounts.setdefault(stocks[i], "stock" if i == here[0] else "stock_of_second_port")
                    amounts.setdefault(stocks[i] + 1, "stock+1" if i == here[0] else "other")
                for a, name in amounts.items():
                    tg = [f"{nm}_{name}", f"{nm}_{'at_port' if here else 'off_port'}"]
                    if len(here) > 1:
                        tg.append(f"{nm}_shared_cell")
                    for fuel, cargo in ((200, 0), (0.5, 49), (1e300, -1), (math.inf, 2 ** 21)):
                        add(w, cell, fuel, cargo, 0, 1 if len(ports) > 1 else 0, act_type, a, tags=tg)
    # cargo on the bound and one take below it; beyond it for the record
    for cargo, a, tg in ((BOUND - 1, 1, "take_cargo_onto_bound"), (BOUND - 50, 50, "take_cargo_onto_bound"),
                         (0, BOUND, "take_cargo_onto_bound"), (-BOUND, 1, "take_cargo_from_negative_bound"),
                         (BOUND, 1, None), (2 ** 30, 2 ** 30, None), (1, BOUND, None)):
        add(3, (50, 0), 200, cargo, 0, 1, 4, a, tags=(tg,) if tg else ())

    # ---- categories
    for w in (0, 3, 4, 5):
        for cat in (I32_MIN, -1, 0, 5, I32_MAX):
            for dest in (0, None):
                add(w, (0, 0), 200, 3, 0 if w != 5 else None, dest if w != 5 else None, cat, 0,
                    tags=(f"category_{cat}",))
    # ---- no ports: whatever the action
    for act_type, a, b in ((1, 1, 0), (1, 0, 0), (1, -1, 0), (1, 300, 0), (2, 0, 0), (2, -1, 0), (3, 1, 0),
                           (4, 1, 0), (4, 0, 0)):
        for pos in ((0, 0), (1, 1), (2, 2)):
            add(5, pos, 200, 3, None, None, act_type, a, b)
    # ---- destination None: alone and with a move out of range (the error order, :276 before :284)
    for w, pos in ((2, (0, 0)), (3, (0, 0)), (3, (49, 49)), (4, (255, 255))):
        for a, b in ((1, 0), (0, 0), (-1, 0), (0, -1), (257, 0), (0, 256), (I32_MIN, I32_MAX), (2 ** 40, 0)):
            add(w, pos, 200, 3, 0, None, 1, a, b)
        for act_type, a in ((3, 1), (4, 1), (3, 0), (2, 1)):
            add(w, pos, 200, 3, 0, None, act_type, a)


# ------------------------------------------------------------------ output
def write_npz(path, arrays):
    """np.load-able, deflated, and byte-identical from run to run (np.savez stamps the time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    worlds = make_worlds()
    bk = Book(worlds)
    enumerate_records(bk)
    out = {}
    for k, v in bk.cols.items():
        if k in FIELDS_F64:
            out[k] = np.asarray(v, np.float64)
        elif k in EXTRA_I64:
            out[k] = np.asarray(v, np.int64)
        else:
            out[k] = np.asarray(v, np.int32)
    n = len(out["kind"])
    assert all(len(v) == n for v in out.values())
    for i, w in enumerate(worlds):
        out[f"w{i}_water"] = w["water"]
        out[f"w{i}_port_x"] = np.asarray([p[0] for p in w["ports"]], np.int32)
        out[f"w{i}_port_y"] = np.asarray([p[1] for p in w["ports"]], np.int32)
        out[f"w{i}_port_fuel"] = np.asarray(w["fuel"], np.int32)
        out[f"w{i}_port_cargo"] = np.asarray(w["cargo"], np.int32)
    write_npz(os.path.join(HERE, "step_edges.npz"), out)
    meta = {
        "records": n, "worlds": len(worlds), "bound": BOUND,
        "beyond_contract": int(out["beyond_contract"].sum()),
        "per_world": [int((out["world"] == i).sum()) for i in range(len(worlds))],
        "counts": dict(sorted(bk.tags.items())),
    }
    with open(os.path.join(HERE, "step_edges_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: meta[k] for k in ("records", "beyond_contract", "per_world")}))
    print(os.path.getsize(os.path.join(HERE, "step_edges.npz")), "bytes")


if __name__ == "__main__":
    main()
