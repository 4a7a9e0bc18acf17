"""Hand-made worlds and ships for the random policy (se_sample_actions) and the MCTS rollouts
(se_rollout): each actor is a ship placed so that its rollouts meet one thing the kernels can
get wrong (a status, a retry, the second Philox block, a world edge, cargo past 2^21). A claim
names that thing; tests/test_rollout_cpu.py shows on the C oracle's rollout trace that the
actor's 64 rollouts hold it, and tests/test_gpu_rollout_edges.py compares the same rollouts on
the GPU with the oracle bit for bit."""
import numpy as np

NONE = -1  # origin / dest None in the oracle's state (255 on the device)
MOVE, SELECT, TAKE_CARGO = 1, 2, 4
SAMPLE_RAISES, SAMPLE_NO_OTHER_PORT = -1, -2
DONE, MAX_STEPS, RAISED, ATTEMPTS, BAD_SRC = 0, 1, 2, 3, 4
USED_LOSS_TYPE, USED_BETA, USED_ARRIVE = 2, 4, 8
BIG = 1 << 21  # beta_part takes the f64 product from this cargo on
REPS = 64  # rollouts per actor: rollout 64 * a + j puts actor a in lane j of a wave
SEED = 5
BUDGET = (20, 21)  # (max_steps, max_attempts) the claims are made under: one retry to spare


class World:
    """An H x W map (W != H, so a cell index with the sides swapped shows), water but for
    `ground`, with hand-placed ports and stocks."""

    def __init__(self, H, W, ports, fuel, cargo, ground=()):
        self.H, self.W = H, W
        self.water = np.ones((H, W), np.uint8)
        for x, y in ground:
            self.water[x, y] = 0
        self.ports = [list(p) for p in ports]
        self.fuel_stock, self.cargo_stock = list(fuel), list(cargo)
        self.P = len(self.ports)

    def env(self, n, seed=SEED, env_id_base=0):
        from shippingenv_amd.vec import VecEnv

        return VecEnv(n, water=self.water, ports=self.ports, port_fuel=self.fuel_stock,
                      port_cargo=self.cargo_stock, seed=seed, env_id_base=env_id_base)

    def oracle(self, O):
        return O.OracleWorld(self.water, [p[0] for p in self.ports], [p[1] for p in self.ports],
                             self.fuel_stock, self.cargo_stock)


# ports 0 .. 3; port 3 has no cargo in stock; (2, 5) is ground in open water
OPEN = World(7, 9, ports=[(1, 1), (5, 6), (3, 7), (5, 2)], fuel=[9, 4, 7, 3], cargo=[5, 6, 8, 0], ground=[(2, 5)])
ONE = World(5, 6, ports=[(2, 3)], fuel=[6], cargo=[3])
# ports 0 and 1 on one cell: the cell answers as port 0, an arrival at port 1 happens there
SHARED = World(6, 7, ports=[(3, 3), (3, 3), (1, 5)], fuel=[5, 9, 4], cargo=[2, 8, 6])
# port 0 stocks 2^23 cargo: a sampled TAKE_CARGO there loads 2^21 or more three times in four
HEAVY = World(7, 9, ports=[(2, 2), (4, 5), (1, 6)], fuel=[9, 4, 7], cargo=[1 << 23, 6, 8])
# 64 ports, port i at cell (1 + i // 11, 1 + i % 11): port 63 has the last cell code
MANY = World(9, 13, ports=[(1 + i // 11, 1 + i % 11) for i in range(64)], fuel=[1 + i % 9 for i in range(64)],
             cargo=[1 + (5 * i) % 7 for i in range(64)])
WORLDS = {"open": OPEN, "one": ONE, "shared": SHARED, "heavy": HEAVY}


def max_world():
    """The largest world the ABI takes, as test_max_map_and_ports_vs_oracle draws it: a 256 x 256
    map, 254 ports, 14 cells holding two ports each."""
    rng = np.random.default_rng(77)
    water = (rng.random((256, 256)) < 0.6).astype(np.uint8)
    cells = np.argwhere(water != 0)
    pick = rng.choice(len(cells), size=240, replace=False)
    ports = [[int(a), int(b)] for a, b in cells[pick]]
    ports += ports[:14]
    w = World(256, 256, ports, [5 + i % 16 for i in range(254)], [5 + (7 * i) % 16 for i in range(254)])
    w.water = water
    return w


def ship(cell, origin, dest, cargo=0, fuel=100.0):
    return dict(cell=cell, origin=origin, dest=dest, cargo=cargo, fuel=fuel)


def actors(name):
    """name -> [(label, ship, claims)]. A claim holds under BUDGET and SEED:
    ("status", s): some of the actor's rollouts end with status s; ("all", s): all of them;
    ("used", bit): some rollout's counted steps made that draw; ("raised",): some rollout
    retried a raising step; ("cut_short",): some rollout ran out of attempts after at least one
    counted step; ("big_beta",): some partial loss was taken from cargo >= 2^21;
    ("steps_le", k): no rollout counts more than k steps (0: it ends at the first attempt);
    ("sample", type): what the random policy answers on the actor's state."""
    if name == "open":
        return [
            # at sea without a destination every sampled move raises NO_DEST
            ("no_dest_at_sea", ship((3, 3), 0, NONE),
             [("all", ATTEMPTS), ("raised",), ("sample", MOVE)]),
            # in the map's corners half the moves leave the map: retried, not counted
            ("corner_first", ship((0, 0), 0, 1),
             [("status", ATTEMPTS), ("cut_short",), ("raised",)]),
            ("corner_last", ship((6, 8), 1, 0),
             [("status", ATTEMPTS), ("cut_short",), ("raised",)]),
            # a move costs 0.9 .. 1.1: the second one runs dry
            ("low_fuel", ship((3, 3), 0, 1, fuel=1.5), [("all", DONE), ("steps_le", 2)]),
            # one cell north of port 1: a quarter arrive at the first attempt
            ("next_to_dest", ship((5, 5), 0, 1, cargo=10),
             [("used", USED_ARRIVE), ("status", MAX_STEPS)]),
            # the gate fires on three moves in five, and on every move
            ("loaded_30", ship((3, 4), 0, 1, cargo=30), [("used", USED_LOSS_TYPE), ("used", USED_BETA)]),
            ("loaded_60", ship((3, 4), 0, 1, cargo=60), [("used", USED_LOSS_TYPE), ("used", USED_BETA)]),
            # on port 0 without a destination: the sampled port is 1, 2 or 3, and 2 is the origin
            ("select_other_origin", ship((1, 1), 2, NONE), [("raised",), ("sample", SELECT)]),
            # cargo 0 on the port without stock: randint(1, 0) raises
            ("empty_stock", ship((5, 2), 0, 1), [("all", RAISED), ("steps_le", 0), ("sample", SAMPLE_RAISES)]),
            ("fuel_zero_at_port", ship((1, 1), 2, 1, cargo=5, fuel=0.0),
             [("all", RAISED), ("steps_le", 0), ("sample", SAMPLE_RAISES)]),
            # a sampled take on a stocked port
            ("take_at_port", ship((5, 6), 0, 2), [("status", MAX_STEPS), ("sample", TAKE_CARGO)]),
        ]
    if name == "one":
        return [
            ("one_port_world", ship((2, 3), 0, NONE), [("all", RAISED), ("steps_le", 0), ("sample", SAMPLE_NO_OTHER_PORT)]),
            ("one_port_at_sea", ship((2, 4), 0, NONE), [("all", ATTEMPTS), ("sample", MOVE)]),
        ]
    if name == "shared":
        return [
            # one cell south of the shared cell, bound for the second port there
            ("shared_cell", ship((3, 4), 2, 1, cargo=7), [("used", USED_ARRIVE)]),
            # on the shared cell (port 0 answers) with origin 1: the sampled port is 1 or 2
            ("shared_select", ship((3, 3), 1, NONE), [("raised",), ("sample", SELECT)]),
        ]
    if name == "heavy":
        return [
            ("big_stock", ship((2, 2), 2, 1), [("big_beta",), ("sample", TAKE_CARGO)]),
        ] + [
            (f"big_cargo_{c}", ship((3, 4), 0, 1, cargo=c), [("used", USED_BETA)] + ([("big_beta",)] if c >= BIG else []))
            for c in (BIG - 1, BIG, BIG + 1, (1 << 24) + 3, 1 << 28)
        ]
    raise KeyError(name)


def table(O, name, reps=1):
    """The world's actors as an oracle state, each `reps` times in a row (a fresh state per call)."""
    rows = actors(name)
    st = O.OracleState(len(rows) * reps)
    for a, (_, sh, _) in enumerate(rows):
        sl = slice(a * reps, (a + 1) * reps)
        st.x[sl], st.y[sl] = sh["cell"]
        st.fuel[sl], st.cargo[sl], st.origin[sl], st.dest[sl] = sh["fuel"], sh["cargo"], sh["origin"], sh["dest"]
    return st


def table_src(name):
    """Rollout 64 * a + j starts from actor a: every actor sits in every lane of a wave."""
    return np.repeat(np.arange(len(actors(name)), dtype=np.int32), REPS)


def assert_claims(O, name):
    """Show on the oracle's trace that every actor holds what it claims; returns the statuses
    and used bits seen, and the largest cargo a partial loss was taken from."""
    world, st = WORLDS[name].oracle(O), table(O, name)
    ms, ma = BUDGET
    _, steps, status, log = O.rollout(world, st, table_src(name), max_steps=ms, max_attempts=ma, seed=SEED, trace=True)
    sampled = O.sample_actions(world, st, seed=SEED, t=0)[0]
    for a, (label, _, claims) in enumerate(actors(name)):
        sl = slice(a * REPS, (a + 1) * REPS)
        for claim in claims:
            kind, arg = claim[0], claim[-1]
            if kind == "status":
                assert (status[sl] == arg).any(), f"{label}: no rollout ends with status {arg}: {np.bincount(status[sl])}"
            elif kind == "all":
                assert (status[sl] == arg).all(), f"{label}: statuses {np.bincount(status[sl])}, all {arg} claimed"
            elif kind == "used":
                assert (log["used"][sl] & arg).any(), f"{label}: no rollout drew used bit {arg}"
            elif kind == "raised":
                assert (log["raised"][sl] > 0).any(), f"{label}: no raising step was retried"
            elif kind == "cut_short":
                assert ((status[sl] == ATTEMPTS) & (steps[sl] > 0) & (steps[sl] < ms)).any(), label
            elif kind == "big_beta":
                assert (log["beta_cargo"][sl] >= BIG).any(), f"{label}: no partial loss from cargo >= 2^21"
            elif kind == "steps_le":
                assert (steps[sl] <= arg).all() and (arg > 0 or (log["raised"][sl] == 0).all()), f"{label}: steps {steps[sl].max()}"
            elif kind == "sample":
                assert sampled[a] == arg, f"{label}: sampled type {sampled[a]}, {arg} claimed"
            else:
                raise KeyError(kind)
    return set(status.tolist()), int(np.bitwise_or.reduce(log["used"])), int(log["beta_cargo"].max()), int(log["raised"].max())
