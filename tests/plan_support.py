"""se_rollout_plan restated on the CPU, for tests/test_rollout_plan_cpu.py and
tests/test_gpu_rollout_plan.py.

A scripted rollout plays a list of actions on a private ship. The restatement steps it through
the C oracle's typed step with a tape, in the style of mcts_support.PhiloxDriver: plan position k
of the rollout with id `ident` reads Philox(seed, ident) at (k, slot 12), words 1-3 as u_fuel,
u_gate, u_type (u = w * 2^-32), and at (k, slot 13) the Beta(2, 2) variate (the median of three
words) and the new destination (multiply-high over the other ports). These are the blocks attempt
k of se_rollout's rollout with the same id reads, so a plan made of that rollout's attempts
(random_plan) must reproduce oracle.rollout bit for bit: tests/test_rollout_plan_cpu.py shows it.

A ship is the tuple (x, y, fuel, cargo, origin, dest) with NONE = -1; a typed action is
(type, a, b); an agent-index plan is a list of ints, decoded through oracle.decode_agent.
"""
import numpy as np

from mcts_support import sample_action

NONE = -1
M32 = 0xFFFFFFFF
SLOT_ROLLOUT, SLOT_ROLLOUT_B = 12, 13
DONE, END, BAD_SRC = 0, 1, 4  # SE_PLAN_*
USED_BETA, USED_ARRIVE = 4, 8
BAD_SHIP = (-1, -1, 0.0, -1, -1, -1)  # what a bad source reports as its end ship


class Result:
    """One scripted rollout's outputs, as se_rollout_plan writes them, and the OR of the
    SE_USED_* bits of its counted steps."""
    __slots__ = ("ret", "steps", "status", "raised", "first_err", "first_err_at", "ship", "used")

    def __init__(self, ship, status=END):
        self.ret, self.steps, self.status, self.raised = 0.0, 0, status, 0
        self.first_err, self.first_err_at, self.ship, self.used = 0, -1, ship, 0


class Stepper:
    """One ship's step at plan position k of rollout `ident` (buffers made once and reused)."""

    def __init__(self, O, world, seed):
        self.O, self.world, self.seed = O, world, seed
        self.st = O.OracleState(1)
        self.tape = np.zeros(1, O.TAPE_DTYPE)
        self.key = [seed & M32, seed >> 32]

    def block(self, ident, k, slot):
        return [int(v) for v in self.O.philox([ident & M32, (ident >> 32) & M32, k, slot], self.key)]

    def step(self, ship, action, ident, k):
        """-> (err, ship after, reward, done, used); a raising step returns the ship it was given."""
        st, tape, P = self.st, self.tape, self.world.P
        a, b = self.block(ident, k, SLOT_ROLLOUT), self.block(ident, k, SLOT_ROLLOUT_B)
        tape["u_fuel"], tape["u_gate"], tape["u_type"] = a[1] / 2.0**32, a[2] / 2.0**32, a[3] / 2.0**32
        tape["beta"] = sorted(b[:3])[1] / 2.0**32
        j = (b[3] * max(P - 1, 0)) >> 32
        tape["arrive_dest"] = j + (j >= ship[5])
        tape["used"] = 0
        st.x[0], st.y[0], st.fuel[0], st.cargo[0], st.origin[0], st.dest[0] = ship
        self.O.step(self.world, st, act_type=[action[0]], act_a=[action[1]], act_b=[action[2]], tape=tape)
        if st.err[0] != 0:
            return int(st.err[0]), ship, 0.0, False, 0
        after = (int(st.x[0]), int(st.y[0]), float(st.fuel[0]), int(st.cargo[0]), int(st.origin[0]), int(st.dest[0]))
        return 0, after, float(st.reward[0]), bool(st.done[0]), int(tape["used"][0])


def decode_plan(O, P, indices):
    """An agent-index plan -> [(type, a, b, decode error)] (oracle.decode_agent)."""
    ty, a, b, err = O.decode_agent(np.asarray(indices, np.int32), P)
    return [(int(t), int(x), int(y), int(e)) for t, x, y, e in zip(ty, a, b, err)]


def plan_rollout(O, world, ship, plan, seed, ident, length=None, agent=False, stepper=None):
    """The scripted rollout of `plan` from `ship` under Philox(seed, ident). length: the plan's
    length as se_rollout_plan's len gives it (clamped to [0, len(plan)]). agent: the plan holds
    agent indices; an index whose decode raises is a raising step with the decode's error."""
    sp = stepper or Stepper(O, world, seed)
    n = len(plan) if length is None else min(max(int(length), 0), len(plan))
    acts = decode_plan(O, world.P, plan) if agent else [tuple(p) + (0,) for p in plan]
    out = Result(ship)
    for k in range(n):
        ty, a, b, e_in = acts[k]
        if e_in:
            err, rw, done, used = e_in, 0.0, False, 0
        else:
            err, ship, rw, done, used = sp.step(ship, (ty, a, b), ident, k)
        if err:
            if out.raised == 0:
                out.first_err, out.first_err_at = err, k
            out.raised += 1
            continue
        out.ret += rw
        out.steps += 1
        out.used |= used
        if done:
            out.status = DONE
            break
    out.ship = ship
    return out


def random_plan(O, world, ship, seed, ident, max_steps, max_attempts, stepper=None):
    """The attempts se_rollout's rollout `ident` makes from `ship`: attempt k's action is
    sample_action on word 0 of (k, slot 12), the loop that of agents/mcts.py:211-238 (stop when
    done, at max_steps counted steps, at max_attempts attempts, or where sample_action raises)."""
    sp = stepper or Stepper(O, world, seed)
    plan, steps = [], 0
    for k in range(max_attempts):
        if steps >= max_steps:
            break
        act = sample_action(ship, world, sp.block(ident, k, SLOT_ROLLOUT)[0])
        if isinstance(act, str):
            break
        plan.append(act)
        err, ship, _, done, _ = sp.step(ship, act, ident, k)
        if err:
            continue
        steps += 1
        if done:
            break
    return plan


def ship_of(st, i):
    return (int(st.x[i]), int(st.y[i]), float(st.fuel[i]), int(st.cargo[i]), int(st.origin[i]), int(st.dest[i]))


_RANDOM = {}


def random_table(O, RS, name, base, budget=None):
    """For the world's actor table (rollout_support.table_src: 64 rollouts per actor) at rollout
    ids base + r: (the random plans, their restated results). Computed once per argument set and
    shared: callers leave it unchanged."""
    budget = budget or RS.BUDGET
    key = (name, base, budget)
    if key not in _RANDOM:
        world, st = RS.WORLDS[name].oracle(O), RS.table(O, name)
        sp = Stepper(O, world, RS.SEED)
        plans, results = [], []
        for r, i in enumerate(RS.table_src(name)):
            sh = ship_of(st, i)
            plans.append(random_plan(O, world, sh, RS.SEED, base + r, *budget, stepper=sp))
            results.append(plan_rollout(O, world, sh, plans[-1], RS.SEED, base + r, stepper=sp))
        _RANDOM[key] = (plans, results)
    return _RANDOM[key]


def pack(plans, K=None, pad=(0, 0, 0)):
    """Typed plans -> (type, a, b) int32 arrays [K, m] and their lengths; shorter plans are
    padded with `pad` (type 0 raises)."""
    m = len(plans)
    K = max([len(p) for p in plans] + [0]) if K is None else K
    out = np.empty((3, K, m), np.int32)
    out[0], out[1], out[2] = pad
    for r, p in enumerate(plans):
        for k, act in enumerate(p):
            out[:, k, r] = act
    return out[0], out[1], out[2], np.array([len(p) for p in plans], np.int32)
