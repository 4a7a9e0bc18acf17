"""A golden session of the reference's SARSAAgent (agents/sarsa.py).

TEST INFRASTRUCTURE, build container only (imports /root/reference with the cv2 stub of
cv2stub/ and a bare matplotlib). The agent runs unmodified; this process records it from
outside by wrapping, on the instances, Environment.reset / step / sample_action and the
agent's choose_action / update, and by giving the agents.sarsa module a `random` whose
random() is recorded (choose_action's explore draw, :151). test_policy is replaced on the
instance by a stub: greedy on a young table it never returns (it repeats a legal SELECT,
agents/sarsa.py:337), and train calls it at episode 0.

One session, one agent, one table, as a flat list of events in the order they happened:
    ["reset", ship] / ["place", ship]     env.reset() / a ship placed by hand (a fresh episode)
    ["set_q", key, value]                 a table entry written by hand before a placed step
    ["uniform", u, epsilon]               choose_action's random.random() and the epsilon it met
    ["sample", action | {"raise": ..}]    env.sample_action()
    ["chose", action]                     what choose_action returned
    ["step", action, {"ship", "reward", "done"} | {"raise": ..}]    env.step(action)
    ["update", key, q before, q after]    agent.update
First three short train() runs on the default five ports (epsilon 1, then 0.5, then 0), then
placed states, each one step of train's inner loop driven through the agent's own methods: at
sea, at a port with and without destination, at a map corner, fuel at 9.99 / 10 / 20 / 39.99 /
40 / 80 and just below a move's cost (a done step), and a chosen action that raises so that the
retry loop runs. A key is [x, y, cargo_bucket, fuel_bucket, prev, dest, [type, a, b]]; floats
are float.hex. The final q_table closes the file. tests/test_sarsa_cpu.py replays the session
through tests/sarsa_support.py.

    python tests/golden/make_sarsa_golden.py
"""
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "cv2stub"))
sys.path.insert(0, REF)
for name in ("matplotlib", "matplotlib.pyplot"):  # imported by agents/sarsa.py for its plots only
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
os.chdir(REF)  # the map is opened by its bare file name

import agents.sarsa as S  # noqa: E402
from shipping import Environment  # noqa: E402
from utils.preprocessing import discretize_state  # noqa: E402

MAP = "mapa_mundi_binario.jpg"
DEFAULT_PORTS = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]  # utils/constants.py:57-63
MOVE, SELECT, TAKE_FUEL, TAKE_CARGO = 1, 2, 3, 4

EVENTS = []
AGENT = [None]


def none(v):
    return -1 if v is None else int(v)


def ship_of(env):
    return [int(env.ship_position[0]), int(env.ship_position[1]), float(env.fuel).hex(), int(env.cargo),
            none(env.origin_port_index), none(env.destination_port_index)]


def action_of(action):
    t, v = action
    if isinstance(v, (list, tuple)):
        return [int(t), int(v[0]), int(v[1])]
    return [int(t), int(v), 0]


def key_of(state_key, action):
    (x, y), cb, fb, prev, dest = state_key
    return [int(x), int(y), int(cb), int(fb), int(prev), int(dest), action_of(action)]


class RecordingRandom:
    """The agents.sarsa module's `random`: random() is recorded with the epsilon it is compared to."""

    def random(self):
        u = random.random()
        EVENTS.append(["uniform", u.hex(), float(AGENT[0].epsilon).hex()])
        return u

    def __getattr__(self, name):
        return getattr(random, name)


def record(env, agent):
    AGENT[0] = agent
    S.random = RecordingRandom()
    reset, step, sample = env.reset, env.step, env.sample_action
    choose, update = agent.choose_action, agent.update

    def env_reset():
        out = reset()
        EVENTS.append(["reset", ship_of(env)])
        return out

    def env_step(action):
        try:
            out = step(action)
        except Exception as e:  # noqa: BLE001 - the reference's exception is the datum
            EVENTS.append(["step", action_of(action), {"raise": type(e).__name__}])
            raise
        EVENTS.append(["step", action_of(action), {"ship": ship_of(env), "reward": float(out[1]).hex(),
                                                   "done": bool(out[2])}])
        return out

    def env_sample():
        try:
            a = sample()
        except Exception as e:  # noqa: BLE001
            EVENTS.append(["sample", {"raise": type(e).__name__}])
            raise
        EVENTS.append(["sample", action_of(a)])
        return a

    def agent_choose(state, deterministic=False):
        a = choose(state, deterministic)
        EVENTS.append(["chose", action_of(a)])
        return a

    def agent_update(state, action, reward, next_state, next_action):
        key = (discretize_state(state), tuple(action))
        before = agent.get_q_value(*key)
        update(state, action, reward, next_state, next_action)
        EVENTS.append(["update", key_of(*key), float(before).hex(), float(agent.get_q_value(*key)).hex()])

    env.reset, env.step, env.sample_action = env_reset, env_step, env_sample
    agent.choose_action, agent.update = agent_choose, agent_update
    agent.test_policy = lambda *a, **k: {}


def place(env, cell, origin, dest, fuel=200.0, cargo=0):
    env.ship_position = list(cell)
    env.origin_port_index, env.destination_port_index = origin, dest
    env.fuel, env.cargo = fuel, cargo
    EVENTS.append(["place", ship_of(env)])


def set_q(agent, env, action, value):
    """Write the entry of (the env's current state, action) by hand."""
    key = (discretize_state(env._build_state()), tuple(action))
    agent.q_table[key] = value
    EVENTS.append(["set_q", key_of(*key), float(value).hex()])


def one_step(agent, env):
    """The first choice of an episode (:256) and one pass through train's inner loop (:262-269)."""
    state = env._build_state()
    action = agent.choose_action(state)
    next_state, reward, done, _ = agent._try_action(action)
    next_action = agent.choose_action(next_state)
    agent.update(state, action, reward, next_state, next_action)
    if done:
        env.reset()  # what train does next
    return done


def main(seed=23):
    random.seed(seed)
    env = Environment(MAP)
    for p in DEFAULT_PORTS:
        env.add_port(list(p))
    agent = S.SARSAAgent(env)
    record(env, agent)
    for eps, steps in ((1.0, 45), (0.5, 45), (0.0, 12)):
        agent.epsilon = eps
        agent.train(episodes=10**6, verbose=False, max_total_steps=steps)

    dones = 0
    sea = [50, 30]
    agent.epsilon = 0.0
    # at sea, an untouched row: the first maximum is SELECT 0
    place(env, sea, 0, 1)
    one_step(agent, env)
    # at sea with a move preferred; the later, equal entry does not replace it
    place(env, sea, 0, 1, fuel=150.0)
    set_q(agent, env, [MOVE, (0, 1)], 0.75)
    set_q(agent, env, [MOVE, (1, 0)], 0.75)
    set_q(agent, env, [SELECT, 3], -1.0)
    one_step(agent, env)
    # at a port with a destination: TAKE_CARGO and TAKE_FUEL join the scan
    place(env, DEFAULT_PORTS[1], 1, 3)
    set_q(agent, env, [TAKE_FUEL, 2], 0.5)
    one_step(agent, env)
    place(env, DEFAULT_PORTS[1], 1, 3)
    set_q(agent, env, [TAKE_CARGO, min(20, env.port_cargo[1])], 2.0)
    one_step(agent, env)
    # at a port without destination: the greedy SELECT of the origin raises, the retry loop runs
    place(env, DEFAULT_PORTS[2], 2, None)
    set_q(agent, env, [SELECT, 2], 1.0)
    one_step(agent, env)
    # ... and exploring there
    agent.epsilon = 1.0
    place(env, DEFAULT_PORTS[2], 2, None)
    one_step(agent, env)
    agent.epsilon = 0.0
    # a map corner: the preferred move leaves the map, sampled moves are retried until one stays
    place(env, [0, 0], 0, 1)
    set_q(agent, env, [MOVE, (0, -1)], 3.0)
    one_step(agent, env)
    # the fuel-class boundaries, before the step and (one move later) after it
    for fuel in (9.99, 10.0, 20.0, 39.99, 40.0, 80.0, 11.05, 61.0):
        place(env, sea, 0, 1, fuel=fuel)
        set_q(agent, env, [MOVE, (-1, 0)], 1.25)
        one_step(agent, env)
    # just below a move's cost (0.9 .. 1.1): done, and the update still adds gamma * next_q
    for fuel in (0.89, 0.5):
        place(env, sea, 0, 1, fuel=fuel)
        set_q(agent, env, [MOVE, (0, 1)], 0.25)
        dones += one_step(agent, env)
    # loaded, next to the destination
    place(env, [DEFAULT_PORTS[1][0], DEFAULT_PORTS[1][1] - 1], 0, 1, cargo=30)
    set_q(agent, env, [MOVE, (0, 1)], 0.5)
    one_step(agent, env)

    table = [[key_of(*k), float(v).hex()] for k, v in agent.q_table.items()]
    doc = {"seed": seed, "lr": agent.lr, "gamma": agent.gamma, "H": 100, "W": 100,
           "ports": [list(map(int, p)) for p in env.port_positions], "port_fuel": list(map(int, env.port_fuel)),
           "port_cargo": list(map(int, env.port_cargo)), "events": EVENTS, "q_table": table}
    path = os.path.join(HERE, "sarsa_golden.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    kinds = {}
    for ev in EVENTS:
        kinds[ev[0]] = kinds.get(ev[0], 0) + 1
    raised = sum(1 for ev in EVENTS if ev[0] == "step" and "raise" in ev[2])
    print(kinds, "raising steps", raised, "placed dones", dones, "table", len(table))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
