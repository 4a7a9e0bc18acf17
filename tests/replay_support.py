"""Scripted replay-ring scenarios: the worlds, the per-step roles, the fuel tags, the action
scripts and the sampler tables of test_gpu_replay_edges.py, and what the C oracle says they hold.
Shared by test_replay_support_cpu.py (the tables are what they claim to be) and
test_gpu_replay_edges.py (the kernels against them).

World: all water, the ports on a grid at least 2 cells from every border and at least 3 cells
apart, so a ship that steps off its port and back never leaves the map and never reaches
another port: which envs raise and which finish follows from the script alone, never from a draw.

Per step every env has a role:
* RAISE: an agent index past the action space, 4 + P + 250 or 2^31 - 1 in turn. Both decode as
  TAKE_FUEL of an amount above every stock (the decode only refuses indices below -4), so the
  step raises whatever the state: SE_ERR_AMOUNT at a port, SE_ERR_NOT_AT_PORT at sea.
* FINISH: fuel 0.25 is written before the step and the action is a move; a unit move costs at
  least 0.9 (environment.py:103-104), so the ship runs out of fuel and done is set.
* PLAIN: a move; at a port also a take of 1..5 units (every stock holds at least 5) or the
  selection of another port than the origin.
A ship on a port moves any way, a ship beside one moves back onto it.

Before every step the fuel of the envs that do not finish is overwritten with 10 + id / 256, id
the running transition counter mod 2^14: exact in f32, so column 2 of a stored observation row
names its transition.

numpy and the oracle only: nothing here needs a GPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

SEED = 90125
PLAIN, FINISH, RAISE = 0, 1, 2
REC_DONE, REC_INVALID = 1, 2  # the ring's flags byte (csrc/step_io.h kRecDone, kRecInvalid)
FLAG_OF_ROLE = np.array([0, REC_DONE, REC_INVALID], np.uint8)
ROTATION = np.array([PLAIN, PLAIN, FINISH, RAISE], np.int8)
FINISH_FUEL = 0.25
BIG_ACTION = 2**31 - 1
MOVES = ((0, -1), (-1, 0), (0, 1), (1, 0))  # N, E, S, W as (dx, dy), utils/preprocessing.py:126
T_LAST = 2**32 - 1
TAG_IDS = 2**14


class World:
    """H x W cells of water and P ports on a grid; pid[x, y] is the port on a cell or -1."""

    def __init__(self, P):
        if P == 5:
            self.H, self.W = 12, 16
            cells = [(3, 3), (3, 8), (3, 12), (8, 5), (8, 11)]
        elif P == 64:
            self.H = self.W = 36
            cells = [(3 + 4 * i, 3 + 4 * j) for i in range(8) for j in range(8)]
        elif P == 254:
            self.H = self.W = 256
            cells = [(8 + 15 * i, 8 + 15 * j) for i in range(16) for j in range(16)][:254]
        else:
            raise ValueError(P)
        self.P = P
        self.ports = [list(c) for c in cells]
        self.port_fuel = [5 + i % 16 for i in range(P)]
        self.port_cargo = [5 + (7 * i) % 16 for i in range(P)]
        self.pid = np.full((self.H, self.W), -1, np.int32)
        for k, (x, y) in enumerate(cells):
            self.pid[x, y] = k

    def water(self):
        return np.ones((self.H, self.W), np.uint8)

    def env_kwargs(self):
        return dict(water=self.water(), ports=self.ports, port_fuel=self.port_fuel, port_cargo=self.port_cargo,
                    seed=SEED)

    def oracle(self, O):
        return O.OracleWorld(self.water(), [p[0] for p in self.ports], [p[1] for p in self.ports],
                             self.port_fuel, self.port_cargo)


@functools.lru_cache(maxsize=None)
def world(P):
    return World(P)


def roles(n, t, salt=0):
    """The role of every env at step t. Up to 8 envs they rotate through plain, plain, finish,
    raise by (i + t) mod 4 (two plain steps in a row, so an episode reaches length 2 unraised);
    beyond, a fixed draw (60 % plain, 20 % finish, 20 % raise) whose first four envs still rotate."""
    rot = ROTATION[(np.arange(n) + t) % 4]
    if n <= 8:
        return rot
    r = np.random.default_rng([SEED, salt, t]).choice(3, size=n, p=[0.6, 0.2, 0.2]).astype(np.int8)
    r[:4] = rot[:4]
    return r


def ring_roles(size, flagged):
    """One step's roles that flag exactly the envs of `flagged` (a bool array): they raise, the
    others are plain and finish in turn."""
    return np.where(np.asarray(flagged, bool), RAISE, np.arange(size) % 2).astype(np.int8)


def tags(n, t):
    """The fuel tag of env i's transition at step t, as the f64 written into env.fuel."""
    ids = (t * n + np.arange(n, dtype=np.int64)) % TAG_IDS
    return 10.0 + ids.astype(np.float64) / 256.0


def fuel_for(role, t):
    return np.where(role == FINISH, FINISH_FUEL, tags(len(role), t))


def actions_for(w, role, x, y, origin, t, salt=0):
    """The step's agent indices from the roles and the ships' cells (see the module docstring)."""
    n, P = len(role), w.P
    rng = np.random.default_rng([SEED, salt, t, 1])
    at = w.pid[x, y]
    back = np.full(n, -1, np.int64)
    for k, (dx, dy) in enumerate(MOVES):
        nx, ny = np.clip(x + dx, 0, w.H - 1), np.clip(y + dy, 0, w.W - 1)
        back = np.where((at < 0) & (w.pid[nx, ny] >= 0), k, back)
    assert ((at >= 0) | (back >= 0)).all(), "a ship is neither on a port nor beside one"
    move = np.where(at >= 0, rng.integers(0, 4, n), back)
    kind = rng.integers(0, 4, n)
    amount = rng.integers(1, 6, n)
    take = np.where(rng.random(n) < 0.5, 4 + P + amount, 4 + P + 50 + amount)
    select = 4 + (origin + 1 + rng.integers(0, P - 1, n)) % P
    plain = np.where((at >= 0) & (kind == 2), take, np.where((at >= 0) & (kind == 3), select, move))
    i = np.arange(n)
    past = np.where((i + (i + t) // 4) % 2 == 0, 4 + P + 250, BIG_ACTION)  # in turn, per env and per round
    return np.where(role == RAISE, past, np.where(role == FINISH, move, plain)).astype(np.int32)


def steps_for(n, cap):
    """ceil(2 cap / n) + 2 steps: the ring wraps at least twice."""
    return -(-2 * cap // n) + 2


def _freeze(obj):
    for v in vars(obj).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return obj


@functools.lru_cache(maxsize=None)
def _scenario(P, n, steps, auto_reset, max_steps, reset_cut, salt, fixed_roles):
    from oracle import oracle as O

    O.build()
    w = world(P)
    ow = w.oracle(O)
    st = O.OracleState(n)
    O.reset(ow, st, seed=SEED, epoch=0)
    epoch = 1
    out = []
    for t in range(steps):
        role = roles(n, t, salt) if fixed_roles is None else np.frombuffer(fixed_roles, np.int8).copy()
        fuel = fuel_for(role, t)
        st.fuel[:] = fuel
        acts = actions_for(w, role, st.x, st.y, st.origin, t, salt)
        if auto_reset:
            O.step_autoreset(ow, st, acts, seed=SEED, t=t)
        else:
            O.step(ow, st, actions=acts, seed=SEED, t=t)
        err, done = st.err.copy(), st.done.copy()
        cut = err != 0
        if max_steps > 0:
            cut = cut | (st.ep_len >= max_steps)
        if reset_cut:  # as env.reset(cut): one epoch per call, cut envs or not
            O.reset(ow, st, mask=cut.astype(np.uint8), seed=SEED, epoch=epoch)
            epoch += 1
            st.ep_len[cut] = 0
            st.ep_return[cut] = 0
        out.append(_freeze(SimpleNamespace(t=t, role=role, fuel=fuel, tags=tags(n, t), actions=acts, err=err,
                                           done=done, cut=cut)))
    return tuple(out)


def scenario(P, n, steps, *, auto_reset, max_steps=0, reset_cut=True, salt=0, fixed_roles=None):
    """The scripted steps of n envs from reset (computed once with the oracle and shared,
    read-only): per step its roles, the fuel to write, the fuel tags, the actions, and the oracle's
    err, done and cut mask (err != 0 | ep_len >= max_steps). After every step the cut envs are
    restarted as env.reset(cut) restarts them, unless reset_cut is False. fixed_roles: the roles
    of every step (ring_roles) instead of roles()."""
    if max_steps > 0 and not auto_reset:
        raise ValueError("max_steps needs the auto-reset env")
    fr = None if fixed_roles is None else np.asarray(fixed_roles, np.int8).tobytes()
    return _scenario(int(P), int(n), int(steps), bool(auto_reset), int(max_steps), bool(reset_cut), int(salt), fr)


# ------------------------------------------------------------------ section 1: ring geometries (n, cap)
SCALAR = [(1, 1), (1, 3), (2, 3), (3, 3), (5, 7), (6, 8), (4, 6), (4, 10), (63, 64), (65, 130), (257, 300)]
WIDE = [(4, 4), (4, 8), (4, 12), (8, 12), (64, 64), (256, 260), (260, 520), (1024, 1028)]
ODD_CUT = (8, 12)          # with the cut mask one byte into its buffer: not 4-byte aligned
ITERS_8 = (8192, 8192)     # one workgroup: 8 groups per thread, se_step_record's last one-launch case
ITERS_9 = (8196, 8200)     # one workgroup: 9 groups per thread, its first fallback
RECORD_FALLBACK = [(6, 8), (4, 6)]
POLICY = [(5, 7), (37, 40), (64, 64), (260, 264), (1024, 1028)]


def takes_wide_kernel(n, cap):
    """replay_end's host-side choice with an aligned cut mask: head stays a multiple of 4 when
    n and cap are."""
    return n % 4 == 0 and cap % 4 == 0


# ------------------------------------------------------------------ section 2: the sampler's tables
SIZES = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
PARTIAL = [17, 65, 257, 1025]  # also read from a ring of size + 5 slots
SIZES_P64 = [5, 65, 1025]
P254_SIZE, P254_BATCHES = 65, [1, 65, 66]
KEYS = [0, T_LAST]
PATTERNS = ["none", "first", "first3", "all4", "mixed", "everything"]
TRIES = 4


def batches(size):
    """B per size, in order, without repeats and without values below 1."""
    out = []
    for b in (1, 63, 64, 65, size, size + 1, 4 * size, 4 * size + 1):
        if b >= 1 and b not in out:
            out.append(b)
    return out


def candidates(O, size, B, t):
    """Peeling with the oracle: row j's first, second, third and fourth candidate slot ([4, B]),
    and a fifth pick with all of them flagged (all -1 when 4 B <= size)."""
    inv = np.zeros(max(size, 1), np.uint8)
    peels = []
    for _ in range(TRIES):
        p = O.replay_pick(size, B, inv, seed=SEED, t=t)
        peels.append(p)
        inv[p[p >= 0]] = 1
    fifth = O.replay_pick(size, B, inv, seed=SEED, t=t)
    return np.stack(peels), fifth


def pattern_depth(pattern, B):
    """How many of each row's candidates the pattern flags (everything: the whole ring)."""
    if pattern in ("none", "everything"):
        return np.zeros(B, np.int64)
    if pattern == "first":
        return np.ones(B, np.int64)
    if pattern == "first3":
        return np.full(B, 3, np.int64)
    if pattern == "all4":
        return np.full(B, 4, np.int64)
    if pattern == "mixed":
        return np.random.default_rng([SEED, 77, B]).integers(0, 5, B)
    raise ValueError(pattern)


def pattern_flags(O, pattern, size, B, t):
    """The slots to flag, as a bool array over the ring, for the pattern at (size, B, t)."""
    flags = np.zeros(size, bool)
    if pattern == "everything":
        flags[:] = True
        return flags
    cand, _ = candidates(O, size, B, t)
    depth = pattern_depth(pattern, B)
    for k in range(TRIES):
        rows = depth > k
        assert (cand[k][rows] >= 0).all()
        flags[cand[k][rows]] = True
    return flags


# ------------------------------------------------------------------ section 3: the update's rings
def union_first_flags(O, size, B, keys):
    """Every row's first candidate under each of the keys, flagged: the later tries run at
    every one of the updates."""
    flags = np.zeros(size, bool)
    for t in keys:
        flags |= pattern_flags(O, "first", size, B, t)
    return flags


UPDATE_KEYS = (0, 1, 2)  # three updates from a zero counter
UPDATE_CASES = {
    # name: (ring size, batch, pattern, every update ends with all weights 0)
    "short_ring": (40, 64, "none", False),
    "first_tile_of_1": (1025, 33, "first", False),
    "mixed": (1025, 200, "mixed", False),
    "all4": (64, 16, "all4", True),
    "empty": (0, 32, "none", True),
}


def update_flags(O, name):
    size, batch, pattern, _ = UPDATE_CASES[name]
    if pattern == "first":
        return union_first_flags(O, size, batch, UPDATE_KEYS)
    if size == 0:
        return np.zeros(0, bool)
    return pattern_flags(O, pattern, size, batch, 0)
