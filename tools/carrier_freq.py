"""How many lanes of a wave the state-only step's GATE pool has to serve ("The
state-only step, pooled GATE"), on the C oracle alone (no GPU):

    python tools/carrier_freq.py [--envs 32768] [--warmup 50] [--timed 1000] [--prerolls 0 20 100 1000] > profiles/seq_gatepool/carriers.json

The bench's config 3 (Philox draws, the 5 default ports, seed 2026, its own action rows: the
pre-roll's at t = 1000000 + k, then rows 0 .. warmup - 1 as the warm-up and the timed steps from
row `warmup` on), stepped from reset. A wave is 256
consecutive envs: 64 lanes of 4. A lane is a carrier when one of its four envs has cargo > 0: only
such a lane's GATE words can be tested. Output:

* at reset and after each pre-roll: the share of envs with cargo > 0, the carrier lanes per wave
  (mean, p90, max) and the share of waves with at most 8 / 16 of them (the pool's windows of 8 and
  4 steps; above 16 a wave draws directly);
* the same at action rows of the run after the last pre-roll (row warmup + timed: the state the
  timed steps leave);
* through the timed steps: the share of wave-steps on which the take guard votes yes (the pool
  is invalid from the next step), and on which some env's cargo goes from <= 0 to > 0 (what the
  invalidation is for).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WAVE, LANE = 256, 4


def carriers(cargo):
    """The summary of one state: carrier lanes per wave."""
    per_wave = (cargo.reshape(-1, LANE) > 0).any(1).reshape(-1, WAVE // LANE).sum(1)
    return {"envs_with_cargo": round(float((cargo > 0).mean()), 4),
            "carrier_lanes_mean": round(float(per_wave.mean()), 2),
            "carrier_lanes_p90": int(np.percentile(per_wave, 90)), "carrier_lanes_max": int(per_wave.max()),
            "waves_with_none": round(float((per_wave == 0).mean()), 4),
            "waves_le_8": round(float((per_wave <= 8).mean()), 4), "waves_le_16": round(float((per_wave <= 16).mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 15)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--timed", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--prerolls", type=int, nargs="*", default=[0, 20, 100, 1000])
    ap.add_argument("--rows", type=int, nargs="*", default=[550, 1050], help="action rows before which to summarise")
    args = ap.parse_args()

    from oracle import oracle as O
    from shippingenv_amd.maps import builtin_water
    from shippingenv_amd.vec import DEFAULT_PORTS, draw_port_stocks

    O.build()
    water = np.asarray(builtin_water())
    P = len(DEFAULT_PORTS)
    pf, pc = draw_port_stocks(P, args.seed)
    world = O.OracleWorld(water, [p[0] for p in DEFAULT_PORTS], [p[1] for p in DEFAULT_PORTS], pf, pc)
    code = np.where(water != 0, 0, 255).astype(np.int32)  # the world image's cell codes
    for i in reversed(range(P)):
        code[DEFAULT_PORTS[i][0], DEFAULT_PORTS[i][1]] = i + 1
    n = args.envs - args.envs % WAVE
    st = O.OracleState(n)
    O.reset(world, st, seed=args.seed, epoch=0)
    last = max(args.prerolls)
    points = []
    for k in range(last + 1):
        if k in args.prerolls:
            points.append({"point": "reset" if k == 0 else f"pre-roll {k}", **carriers(np.asarray(st.cargo))})
            print(points[-1], file=sys.stderr, flush=True)
        if k < last:
            O.step(world, st, actions=O.gen_actions(n, P, args.seed, 0, 1_000_000 + k), seed=args.seed, t=k)
    t = last
    took_block = became = 0
    total = args.warmup + args.timed
    per_wave = lambda m: int(m.reshape(-1, WAVE).any(1).sum())  # noqa: E731
    for k in range(total + 1):
        if k in args.rows:
            points.append({"point": f"timed step {k}", **carriers(np.asarray(st.cargo))})
            print(points[-1], file=sys.stderr, flush=True)
        if k == total:
            break
        a = np.asarray(O.gen_actions(n, P, args.seed, 0, k))
        before = code[st.x, st.y]
        cargo0 = np.asarray(st.cargo).copy()
        O.step(world, st, actions=a, seed=args.seed, t=t)
        t += 1
        if k >= args.warmup:
            took_block += per_wave((a >= 4 + P) & (before != 0))
            became += per_wave((cargo0 <= 0) & (np.asarray(st.cargo) > 0))
    ws = (n // WAVE) * args.timed
    json.dump({"what": "carrier lanes (a lane = 4 consecutive envs, one of them with cargo > 0) per wave (256 consecutive "
                       "envs); C oracle, Philox draws, 5 default ports, the bench's action rows",
               "envs": n, "seed": args.seed, "waves": n // WAVE, "points": points,
               "warmup_steps": args.warmup, "timed_steps": args.timed, "timed_wave_steps": ws,
               "wave_steps_whose_take_block_runs": round(took_block / ws, 4),
               "wave_steps_in_which_an_env_becomes_a_carrier": round(became / ws, 4)}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
