"""Golden random rollouts of the reference Environment, for the draw laws' end-to-end check.

TEST INFRASTRUCTURE, build container only (imports /root/reference with the cv2
stub of cv2stub/). From each of five start states it runs R random rollouts with
the loop of agents/mcts.py:211-238 (sample_action, step, a raising step retried
without counting, at most 100 counted steps) on the reference's own `random`, and
records per state the sorted returns and the counts of (counted steps, done).
Every start state has a destination and fuel != 0, so neither the endless retry of
a move without destination nor the TypeError of _sample_random_fuel is reached.

Returns are stored in units of 1e-4 as int32: every reward of the reference is a
sum of multiples of 0.0001 (Penalty.USE_FUEL) and 0.05 (Reward.TAKE_*), so
rint(return * 1e4) is exact, and the same rounding of an f32 reward (|r| < 256,
half an f32 ulp < 1.6e-5) recovers the reference's value.

tests/test_draw_laws_cpu.py (the C oracle) and tests/test_gpu_draw_laws.py (the
kernels) compare their rollouts of the same states with these by two-sample tests.

    python tests/golden/make_law_golden.py
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "cv2stub"))
sys.path.insert(0, REF)

from shipping import Environment  # noqa: E402

MAP = os.path.join(REF, "mapa_mundi_binario.jpg")
DEFAULT_PORTS = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]  # utils/constants.py:57-63
MAX_STEPS = 100  # MCTSAgent's max_rollout_steps


def golden_water():
    with open(os.path.join(HERE, "map_water_100x100.bits"), "rb") as f:
        bits = np.frombuffer(f.read(), np.uint8)
    return np.unpackbits(bits)[:10000].reshape(100, 100)


def coast_cell(game):
    """The water cell nearest (50, 50) with ground on exactly one side and no port next to it."""
    best = None
    for x in range(2, 98):
        for y in range(2, 98):
            if game[x, y] != 1:
                continue
            near = [game[x + dx, y + dy] for dx, dy in ((0, -1), (-1, 0), (0, 1), (1, 0))]
            if near.count(0) != 1 or near.count(1) != 3:
                continue
            d = (x - 50) ** 2 + (y - 50) ** 2
            if best is None or d < best[0]:
                best = (d, x, y)
    return best[1], best[2]


def rollout(env):
    """agents/mcts.py:224-238, also returning the counted steps and done"""
    total_reward = 0.0
    done = False
    steps = 0
    while not done and steps < MAX_STEPS:
        action = env.sample_action()
        try:
            _, reward, done, _ = env.step(action)
            total_reward += reward
            steps += 1
        except Exception:  # noqa: BLE001 - the reference's own retry
            continue
    return total_reward, steps, done


def main(R=20000, seed=11):
    random.seed(seed)
    env = Environment(MAP)
    for p in DEFAULT_PORTS:
        env.add_port(list(p))
    game0 = env.np_game.copy()
    water = golden_water()
    port_cell = game0 == 2  # add_port stamps Entity.PORT over whatever the map had there
    assert np.array_equal((game0 != 0) | port_cell, (water != 0) | port_cell), "map differs from the fixture"
    cx, cy = coast_cell(game0)
    # a water cell next to a port other than port 0: the last port that has one
    near = [(d, DEFAULT_PORTS[d][0] + mx, DEFAULT_PORTS[d][1] + my) for d in range(1, 5)
            for mx, my in ((0, 1), (1, 0), (0, -1), (-1, 0))
            if game0[DEFAULT_PORTS[d][0] + mx, DEFAULT_PORTS[d][1] + my] == 1]
    nd, nx, ny = near[-1]
    # x, y, fuel, cargo, origin, dest
    states = np.array([
        [41, 40, 200, 0, 0, 1],
        [41, 40, 40, 0, 0, 1],
        [cx, cy, 200, 45, 0, 3],
        [nx, ny, 200, 30, 0, nd],
        [41, 40, 97, 0, 0, 1],  # the fuel for about as many moves as the rollout makes
    ], np.int32)
    out = {"states": states, "port_fuel": np.array(env.port_fuel, np.int32),
           "port_cargo": np.array(env.port_cargo, np.int32), "ports": np.array(DEFAULT_PORTS, np.int32)}
    for k, (x, y, fuel, cargo, origin, dest) in enumerate(states.tolist()):
        ret = np.zeros(R, np.float64)
        sd = np.zeros((MAX_STEPS + 1, 2), np.int32)
        for r in range(R):
            env.np_game = game0.copy()
            env.ship_position = [x, y]
            env.fuel, env.cargo = fuel, cargo
            env.origin_port_index, env.destination_port_index = origin, dest
            ret[r], steps, done = rollout(env)
            sd[steps, int(bool(done))] += 1
        q = np.rint(ret * 1e4)
        assert np.abs(ret * 1e4 - q).max() < 1e-5
        out[f"ret_{k}"] = np.sort(q.astype(np.int32))
        out[f"steps_done_{k}"] = sd
        print(k, states[k].tolist(), "mean return", ret.mean(), "done share", sd[:, 1].sum() / R)
    path = os.path.join(HERE, "law_rollouts.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
