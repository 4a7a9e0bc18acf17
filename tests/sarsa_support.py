"""SARSAAgent's learning step (agents/sarsa.py:135-195, 201-220, 255-272) restated in plain
Python for n envs on one table, for the tests of se_sarsa_step / VecSARSAAgent.

One vector step runs the body of train's inner loop for every env: a fresh env first chooses
its pending action (:256); _try_action steps it and, if it raises, samples and steps until one
goes through (max_attempts in all); choose_action on the new state; the update, keyed by the
state before and the action as chosen; then done, max_steps or a status other than OK restart
the env. Every env reads the table as the previous vector step left it, and of several updates
of one entry in a step the lowest env index wins (`collisions` counts the dropped ones).

The restatement is written against a *driver* that supplies everything random or
environment-made, per env:

    begin(i, t)               env i's part of vector step t begins
    uniform(which)            random.random() of choose_action: which is "first" (a fresh
                              env's first choice) or "next"
    sample(ship, which)       env.sample_action(): which is "first", "next" or the attempt
                              number j >= 1; an action, or "raised" / "never"
    step(ship, action, j)     env.step(action) as attempt j: (next ship, reward, done), or None
                              if it raised
    restart()                 env.reset(): the new ship
    chose(action), updated(key, before, after)    told what the restatement did (the golden
                              driver checks it against the record)

Two drivers: PhiloxDriver states the kernel's draw contract a second time through the C oracle
(oracle.philox, oracle.step with a tape); GoldenDriver replays a session recorded from the
reference itself (tests/golden/make_sarsa_golden.py) and fails where the restatement asks for
something else than the reference did.

A ship is the tuple (x, y, fuel, cargo, origin, dest) with NONE = -1; an action is (type, a, b).
"""
import numpy as np

from mcts_support import sample_action  # sample_action() from one 32-bit word, se_sample_actions' rules

NONE = -1
MOVE, SELECT, TAKE_FUEL, TAKE_CARGO = 1, 2, 3, 4
OK, CUT, RAISED, NEVER_RETURNS = 0, 1, 2, 3
MOVES = [(0, -1), (0, 1), (-1, 0), (1, 0)]  # _get_possible_actions' order (:105-110)
BUCKETS = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (4, 3), (4, 4)]  # fuel class -> (cargo_bucket, fuel_bucket)
SLOT_CHOOSE, SLOT_RESTART, SLOT_TRY = 20, 21, 32
M32 = 0xFFFFFFFF
FUEL_INIT = 200.0


# ---------------------------------------------------------------------------- the discretiser
def buckets(fuel):
    """discretize_state's (cargo_bucket, fuel_bucket) (utils/preprocessing.py:79-80): both from
    the fuel, since state["ship"]["cargo"] is the fuel (environment.py:206)."""
    return min(int(fuel / 10), 4), min(int(fuel / 20), 4)


def fuel_class(fuel):
    """The index of buckets(fuel) in BUCKETS; fuel <= -10, outside the domain, is class 0."""
    cb, fb = buckets(fuel)
    if cb < 0:
        return 0
    return BUCKETS.index((cb, fb))


def discretize(ship):
    """discretize_state (:65-90) -> ((x, y), cargo_bucket, fuel_bucket, prev, dest)."""
    x, y, fuel, _, origin, dest = ship
    cb, fb = BUCKETS[fuel_class(fuel)]
    return ((x, y), cb, fb, origin, dest)


def port_at(world, x, y):
    """find_current_port_index (utils/actions.py:118-132): the first port on the cell."""
    return next((i for i in range(world.P) if world.px[i] == x and world.py[i] == y), NONE)


def possible_actions(ship, world):
    """_get_possible_actions (:81-133), in its order."""
    acts = [(SELECT, p, 0) for p in range(world.P)] + [(MOVE, a, b) for a, b in MOVES]
    cur = port_at(world, ship[0], ship[1])
    if cur != NONE:
        acts += [(TAKE_CARGO, m, 0) for m in range(1, min(21, int(world.pc[cur]) + 1))]
        acts += [(TAKE_FUEL, m, 0) for m in range(1, min(21, int(world.pf[cur]) + 1))]
    return acts


# ---------------------------------------------------------------------------- the table's layout
class Layout:
    """include/shipenv.h's layout of the dense table for a world: rows, A, cmax; entry(key) and
    key(entry) for keys (discretised state, action)."""

    def __init__(self, world):
        self.W, self.P = int(world.W), int(world.P)
        self.cmax = max([20] + [int(c) for c in world.pc])
        self.A = self.P + 4 + self.cmax + 20
        self.rows = int(world.H) * self.W * 7 * (self.P + 1) * (self.P + 1)

    def slot(self, action):
        ty, a, b = action
        if ty == SELECT:
            return a
        if ty == MOVE:
            return self.P + MOVES.index((a, b))
        if ty == TAKE_CARGO:
            return self.P + 3 + a
        return self.P + 3 + self.cmax + a

    def action(self, slot):
        P = self.P
        if slot < P:
            return (SELECT, slot, 0)
        if slot < P + 4:
            return (MOVE,) + MOVES[slot - P]
        if slot < P + 4 + self.cmax:
            return (TAKE_CARGO, slot - (P + 3), 0)
        return (TAKE_FUEL, slot - (P + 3 + self.cmax), 0)

    def entry(self, key):
        ((x, y), cb, fb, origin, dest), action = key
        row = (((x * self.W + y) * 7 + BUCKETS.index((cb, fb))) * (self.P + 1) + origin + 1) * (self.P + 1) + dest + 1
        return row * self.A + self.slot(action)

    def key(self, entry):
        row, slot = divmod(entry, self.A)
        row, dest = divmod(row, self.P + 1)
        row, origin = divmod(row, self.P + 1)
        cell, cls = divmod(row, 7)
        x, y = divmod(cell, self.W)
        return ((x, y),) + BUCKETS[cls] + (origin - 1, dest - 1), self.action(slot)


# ---------------------------------------------------------------------------- the learner
class Env:
    """What one env carries between vector steps."""

    def __init__(self, ship):
        self.ship, self.pending, self.fresh = ship, None, True
        self.ep_len, self.ep_return = 0, 0.0


class Learner:
    def __init__(self, world, lr=0.1, gamma=0.9, max_steps=0, max_attempts=8, dense=None):
        self.world, self.lr, self.gamma = world, lr, gamma
        self.dense = dense     # optional: the table's initial content, a flat array in Layout's order
        self.layout = Layout(world) if dense is not None else None
        self.max_steps, self.max_attempts = max_steps, max_attempts
        self.q = {}            # (discretised state, action) -> value; a missing key reads 0.0
        self.collisions = 0    # updates dropped because a lower env index wrote the same entry
        self.explored = 0      # choices that explored

    def get(self, state, action):
        v = self.q.get((state, action))
        if v is not None:
            return v
        return 0.0 if self.dense is None else float(self.dense[self.layout.entry((state, action))])

    def choose(self, ship, eps, driver, which):
        """choose_action (:135-165): an action, or "raised" / "never"."""
        if driver.uniform(which) < eps:
            self.explored += 1
            return driver.sample(ship, which)
        state = discretize(ship)
        best, best_q = None, float("-inf")
        for action in possible_actions(ship, self.world):
            v = self.get(state, action)
            if v > best_q:
                best, best_q = action, v
        return best if best is not None else driver.sample(ship, which)

    def _one(self, env, eps, learn, driver):
        """One env's part of a vector step against the table as it stands: (out, write) where
        write is None or (key, new value)."""
        status = OK
        if env.fresh or env.pending is None:
            a = self.choose(env.ship, eps, driver, "first")  # :256
            if isinstance(a, str):
                status = NEVER_RETURNS if a == "never" else RAISED
            else:
                env.pending = a
                driver.chose(a)
        before, chosen = env.ship, env.pending
        reward, done, write = 0.0, False, None
        if status == OK:  # _try_action (:201-220)
            res, action = None, chosen
            for j in range(self.max_attempts):
                if j > 0:
                    action = driver.sample(env.ship, j)
                    if isinstance(action, str):
                        status = NEVER_RETURNS if action == "never" else RAISED
                        break
                res = driver.step(env.ship, action, j)
                if res is not None:
                    break
            if status == OK and res is None:
                status = CUT
            if status == OK:
                env.ship, reward, done = res
        if status == OK:
            nxt = self.choose(env.ship, eps, driver, "next")  # :263
            if isinstance(nxt, str):
                status = NEVER_RETURNS if nxt == "never" else RAISED
                reward = 0.0
            else:
                driver.chose(nxt)
                if learn:  # update (:187-195)
                    s0, s1 = discretize(before), discretize(env.ship)
                    curr_q, next_q = self.get(s0, chosen), self.get(s1, nxt)
                    new_q = curr_q + self.lr * (reward + self.gamma * next_q - curr_q)
                    write = ((s0, chosen), new_q)
                    driver.updated((s0, chosen), curr_q, new_q)
                env.pending = nxt
                env.ep_return += reward
                env.ep_len += 1
        restart = done or status != OK or (self.max_steps > 0 and env.ep_len >= self.max_steps)
        out = dict(reward=reward, ended=restart, status=status, fin_return=env.ep_return if restart else 0.0,
                   fin_len=env.ep_len if restart else 0)
        if restart:
            env.ship = driver.restart()
            env.fresh, env.ep_len, env.ep_return = True, 0, 0.0
        else:
            env.fresh = False
        return out, write

    def vector_step(self, envs, eps, learn, driver, t):
        outs, writes = [], {}
        for i, env in enumerate(envs):
            driver.begin(i, t)
            out, write = self._one(env, eps, learn, driver)
            outs.append(out)
            if write is not None:
                if write[0] in writes:
                    self.collisions += 1  # a lower index came first
                else:
                    writes[write[0]] = write[1]
        self.q.update(writes)  # after every read of this step
        return outs


# ---------------------------------------------------------------------------- Philox driver
class PhiloxDriver:
    """The draw contract of se_sarsa_step: key (seed, env_id_base + i), the t word the vector
    step. Slot 20: words 0, 1 the explore uniform and the sample word of the next action, words
    2, 3 those of a fresh env's first choice. Slot 21: words 0, 1 the restart's origin and dest
    by multiply-high, the dest over the other ports. Attempt j: slot 32 + 2j word 0 the sample
    word (j >= 1), words 1-3 u_fuel, u_gate, u_type as w * 2^-32; slot 33 + 2j Beta(2,2) = the
    median of three words, and the new destination by multiply-high over the other ports."""

    def __init__(self, O, world, seed, env_id_base=0):
        self.O, self.world, self.seed, self.base = O, world, seed, env_id_base
        self.id, self.t = env_id_base, 0

    def _block(self, slot):
        return [int(v) for v in self.O.philox([self.id & M32, self.id >> 32, self.t & M32, slot],
                                              [self.seed & M32, self.seed >> 32])]

    def begin(self, i, t):
        self.id, self.t = self.base + i, t

    def uniform(self, which):
        return self._block(SLOT_CHOOSE)[2 if which == "first" else 0] / 2.0**32

    def sample(self, ship, which):
        if which == "first":
            r = self._block(SLOT_CHOOSE)[3]
        elif which == "next":
            r = self._block(SLOT_CHOOSE)[1]
        else:
            r = self._block(SLOT_TRY + 2 * which)[0]
        return sample_action(ship, self.world, r)

    def step(self, ship, action, j):
        O = self.O
        a, b = self._block(SLOT_TRY + 2 * j), self._block(SLOT_TRY + 2 * j + 1)
        tape = np.zeros(1, O.TAPE_DTYPE)
        tape["u_fuel"], tape["u_gate"], tape["u_type"] = a[1] / 2.0**32, a[2] / 2.0**32, a[3] / 2.0**32
        tape["beta"] = sorted(b[:3])[1] / 2.0**32
        k = (b[3] * max(self.world.P - 1, 0)) >> 32
        tape["arrive_dest"] = k + (k >= ship[5])
        st = O.OracleState(1)
        st.x[0], st.y[0], st.fuel[0], st.cargo[0], st.origin[0], st.dest[0] = ship
        O.step(self.world, st, act_type=[action[0]], act_a=[action[1]], act_b=[action[2]], tape=tape)
        if st.err[0] != 0:
            return None
        nxt = (int(st.x[0]), int(st.y[0]), float(st.fuel[0]), int(st.cargo[0]), int(st.origin[0]), int(st.dest[0]))
        return nxt, float(st.reward[0]), bool(st.done[0])

    def restart(self):
        w, r = self.world, self._block(SLOT_RESTART)
        origin = (r[0] * w.P) >> 32
        k = (r[1] * (w.P - 1)) >> 32
        dest = k + (k >= origin) if w.P > 1 else NONE  # one port: the reference's reset never returns
        return (int(w.px[origin]), int(w.py[origin]), FUEL_INIT, 0, origin, dest)

    def chose(self, action):
        pass

    def updated(self, key, before, after):
        pass


# ---------------------------------------------------------------------------- golden driver
class GoldenMismatch(AssertionError):
    pass


def ship_from_json(s):
    return (s[0], s[1], float.fromhex(s[2]), s[3], s[4], s[5])


def key_from_json(k):
    return ((k[0], k[1]), k[2], k[3], k[4], k[5]), tuple(k[6])


class GoldenDriver:
    """Replays the events of a recorded session, in order."""

    def __init__(self, events):
        self.events, self.at = events, 0

    def peek(self):
        return self.events[self.at] if self.at < len(self.events) else None

    def next_epsilon(self):
        """The epsilon of the next recorded choice."""
        for ev in self.events[self.at:]:
            if ev[0] == "uniform":
                return float.fromhex(ev[2])
        raise GoldenMismatch("no further choice is recorded")

    def _next(self, kind):
        if self.at >= len(self.events):
            raise GoldenMismatch(f"the restatement asks for a {kind} after the last recorded event")
        ev = self.events[self.at]
        self.at += 1
        if ev[0] != kind:
            raise GoldenMismatch(f"event {self.at - 1}: the reference did {ev}, the restatement a {kind}")
        return ev

    def begin(self, i, t):
        pass

    def uniform(self, which):
        return float.fromhex(self._next("uniform")[1])

    def sample(self, ship, which):
        ev = self._next("sample")
        return "raised" if isinstance(ev[1], dict) else tuple(ev[1])

    def step(self, ship, action, j):
        ev = self._next("step")
        if tuple(ev[1]) != tuple(action):
            raise GoldenMismatch(f"event {self.at - 1}: step {action}, the reference stepped {ev[1]}")
        if "raise" in ev[2]:
            return None
        return ship_from_json(ev[2]["ship"]), float.fromhex(ev[2]["reward"]), ev[2]["done"]

    def restart(self):
        return ship_from_json(self._next("reset")[1])

    def chose(self, action):
        ev = self._next("chose")
        if tuple(ev[1]) != tuple(action):
            raise GoldenMismatch(f"event {self.at - 1}: chose {action}, the reference {ev[1]}")

    def updated(self, key, before, after):
        ev = self._next("update")
        want = (key_from_json(ev[1]), float.fromhex(ev[2]), float.fromhex(ev[3]))
        if want != (key, before, after):
            raise GoldenMismatch(f"event {self.at - 1}: update {(key, before, after)}, the reference {want}")


def replay_session(world, session):
    """The restatement under the golden driver over a whole recorded session -> (learner, steps).
    Top-level events: "reset" / "place" put the one env at a ship, fresh; "set_q" writes a table
    entry; anything else is the start of a step of train's inner loop."""
    drv = GoldenDriver(session["events"])
    learner = Learner(world, lr=session["lr"], gamma=session["gamma"], max_steps=0, max_attempts=10**9)
    env, steps = None, 0
    while drv.peek() is not None:
        ev = drv.peek()
        if ev[0] in ("reset", "place"):
            drv.at += 1
            env = Env(ship_from_json(ev[1]))
        elif ev[0] == "set_q":
            drv.at += 1
            learner.q[key_from_json(ev[1])] = float.fromhex(ev[2])
        else:
            learner.vector_step([env], drv.next_epsilon(), True, drv, steps)
            steps += 1
    return learner, steps
