"""Golden MCTS decisions of the reference's MCTSAgent.choose_action (agents/mcts.py:240-292).

TEST INFRASTRUCTURE, build container only (imports /root/reference with the cv2 stub of
cv2stub/). The agent runs unmodified; this process records it from outside by wrapping
MCTSNode.__init__ (to list the nodes in creation order), Environment.step (the env copy's
tree steps; the steps inside _rollout are not recorded), MCTSAgent._rollout (where it starts
and what it returns) and the `random` the agents.mcts module sees (its random.choice over the
untried actions, :274). Per decision it records the world, the ship and S; in order every
choice (how many untried actions, the index taken), every tree step (action; the next ship,
reward and done, or the exception) and every rollout (start ship; return); the final tree
(parent, action, visits, total_reward); and what choose_action returned or raised. Floats are
float.hex. tests/test_mcts_cpu.py replays the decisions through tests/mcts_support.py.

    python tests/golden/make_mcts_golden.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "cv2stub"))
sys.path.insert(0, REF)
os.chdir(REF)  # _create_env_copy opens the map by its bare file name (:190, :199)

import agents.mcts as M  # noqa: E402
from shipping import Environment  # noqa: E402

MAP = "mapa_mundi_binario.jpg"
DEFAULT_PORTS = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]  # utils/constants.py:57-63

LOG = {"events": None, "nodes": None, "in_rollout": False}


def none(v):
    return -1 if v is None else int(v)


def ship_of(env):
    x, y = (int(env.ship_position[0]), int(env.ship_position[1])) if len(env.ship_position) else (0, 0)
    return [x, y, float(env.fuel).hex(), int(env.cargo), none(env.origin_port_index),
            none(env.destination_port_index)]


def action_of(action):
    t, v = action
    if isinstance(v, (list, tuple)):
        return [int(t), int(v[0]), int(v[1])]
    return [int(t), int(v), 0]


class RecordingRandom:
    """The agents.mcts module's `random`: choice() takes a recorded index."""

    def choice(self, seq):
        i = random.randrange(len(seq))
        LOG["events"].append(["choice", len(seq), i])
        return seq[i]

    def __getattr__(self, name):
        return getattr(random, name)


def install():
    node_init, env_step, rollout = M.MCTSNode.__init__, Environment.step, M.MCTSAgent._rollout

    def init(self, state, action=None, parent=None):
        node_init(self, state, action=action, parent=parent)
        LOG["nodes"].append(self)

    def step(self, action):
        if LOG["events"] is None or LOG["in_rollout"]:
            return env_step(self, action)
        try:
            out = env_step(self, action)
        except Exception as e:  # noqa: BLE001 - the reference's exception is the datum
            LOG["events"].append(["step", action_of(action), {"raise": type(e).__name__}])
            raise
        LOG["events"].append(["step", action_of(action),
                              {"ship": ship_of(self), "reward": float(out[1]).hex(), "done": bool(out[2])}])
        return out

    def roll(self, env_copy, state):
        start = ship_of(env_copy)
        LOG["in_rollout"] = True
        try:
            ret = rollout(self, env_copy, state)
        except Exception as e:  # noqa: BLE001
            LOG["events"].append(["rollout", start, {"raise": type(e).__name__}])
            raise
        finally:
            LOG["in_rollout"] = False
        LOG["events"].append(["rollout", start, float(ret).hex()])
        return ret

    M.MCTSNode.__init__ = init
    Environment.step = step
    M.MCTSAgent._rollout = roll
    M.random = RecordingRandom()


def make_env(ports, fuel=None, cargo=None):
    env = Environment(MAP)
    for p in ports:
        env.add_port(list(p))
    if fuel is not None:
        env.port_fuel = list(fuel)
    if cargo is not None:
        env.port_cargo = list(cargo)
    return env


def decide(name, env, S, max_rollout_steps=100):
    agent = M.MCTSAgent(env, num_simulations=S, max_rollout_steps=max_rollout_steps)
    LOG["events"], LOG["nodes"] = [], []
    rec = {"name": name, "S": S, "c": agent.exploration_param, "max_rollout_steps": max_rollout_steps,
           "ports": [list(map(int, p)) for p in env.port_positions], "port_fuel": list(env.port_fuel),
           "port_cargo": list(env.port_cargo), "ship": ship_of(env)}
    real_sample = env.sample_action

    def sample():  # the root fallback (:292) is the real env's sample_action
        try:
            a = real_sample()
        except Exception as e:  # noqa: BLE001
            LOG["events"].append(["sample", {"raise": type(e).__name__}])
            raise
        LOG["events"].append(["sample", action_of(a)])
        return a

    env.sample_action = sample
    try:
        rec["result"] = {"action": action_of(agent.choose_action(env._build_state()))}
    except Exception as e:  # noqa: BLE001
        rec["result"] = {"raise": type(e).__name__}
    del env.sample_action
    nodes = LOG["nodes"]
    index = {id(nd): i for i, nd in enumerate(nodes)}
    rec["tree"] = [[-1 if nd.parent is None else index[id(nd.parent)],
                    None if nd.action is None else action_of(nd.action), int(nd.visits),
                    float(nd.total_reward).hex()] for nd in nodes]
    rec["events"] = LOG["events"]
    LOG["events"] = LOG["nodes"] = None
    return rec


def place(env, cell, origin, dest, fuel=None, cargo=None):
    env.ship_position = list(cell)
    env.origin_port_index, env.destination_port_index = origin, dest
    if fuel is not None:
        env.fuel = fuel
    if cargo is not None:
        env.cargo = cargo


def main(seed=11):
    install()
    random.seed(seed)
    out = []
    env = make_env(DEFAULT_PORTS)
    # a fresh reset at the default five ports
    env.reset()
    out.append(decide("fresh_S50", env, 50))
    env.reset()
    out.append(decide("fresh_S3", env, 3))
    # at a port without destination: SELECT children
    env.reset()
    place(env, DEFAULT_PORTS[2], 2, None)
    out.append(decide("select_S12", env, 12, 20))
    # fuel exactly 0 on the origin port, stock 4: TAKE_CARGO children, fewer and more
    # simulations than actions. With cargo aboard and fuel 0 at a port the rollout's
    # sample_action raises (environment.py:258-260, :163), so the decision raises at its first
    # rollout; with max_rollout_steps = 0 the rollout draws nothing and the tree grows
    stocked = make_env(DEFAULT_PORTS, cargo=[7, 4, 9, 5, 6])
    for S, steps in ((2, 0), (9, 0), (9, 100)):
        stocked.reset()
        place(stocked, DEFAULT_PORTS[1], 1, 3, fuel=0)
        out.append(decide(f"fuel_zero_S{S}_steps{steps}", stocked, S, steps))
    # the same at sea: every TAKE_CARGO raises, the root stays bare, the fallback answers
    stocked.reset()
    place(stocked, [50, 30], 1, 3, fuel=0)
    out.append(decide("fuel_zero_at_sea_S3", stocked, 3, 20))
    # a map corner: two of the four moves raise and their simulations are skipped
    env.reset()
    place(env, [0, 0], 0, 1)
    out.append(decide("corner_S12", env, 12, 20))
    # fuel below a move's cost three times in four (0.9 .. 1.1): a selection step reports done
    env.reset()
    place(env, [50, 30], 0, 1, fuel=0.95)
    out.append(decide("low_fuel_S12", env, 12, 20))
    # loaded: cargo losses in the tree steps
    env.reset()
    place(env, [50, 30], 0, 1, cargo=30)
    out.append(decide("loaded_S17", env, 17, 20))
    # one port, no destination: no possible action, choose_action raises
    one = make_env([DEFAULT_PORTS[0]])
    place(one, DEFAULT_PORTS[0], 0, None)
    out.append(decide("one_port", one, 5, 20))
    path = os.path.join(HERE, "mcts_golden.json")
    with open(path, "w") as f:
        json.dump({"seed": seed, "decisions": out}, f, separators=(",", ":"))
    for rec in out:
        print(rec["name"], "nodes", len(rec["tree"]), "events", len(rec["events"]), rec["result"])
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
