"""How often the state-only step's two guards ("The state-only step, guarded") vote no,
on the C oracle alone (no GPU):

    python tools/guard_freq.py [--envs 65536] [--steps 100] [--prerolls 0 20 100 1000] > profiles/seq_guard/freq.json

The bench's config 3 (Philox draws, the 5 default ports, seed 2026, its own action rows: the
pre-roll's at t = 1000000 + k, the timed ones from row 0), stepped from reset through each
pre-roll and then `--steps` steps. A wave is 256 consecutive envs (64 lanes of 4). Per wave and
step, as the kernel votes:

* take guard: an env with a take action (act >= 4 + P) on a non-water cell before the move;
* arrival guard: an env whose move was accepted and that stands on a non-water cell after it.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WAVE = 256
OK = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--prerolls", type=int, nargs="*", default=[0, 20, 100, 1000])
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
    rows = []
    for pre in args.prerolls:
        st = O.OracleState(n)
        O.reset(world, st, seed=args.seed, epoch=0)
        t = 0
        for k in range(pre):
            O.step(world, st, actions=O.gen_actions(n, P, args.seed, 0, 1_000_000 + k), seed=args.seed, t=t)
            t += 1
        on_port = []
        c = {"take": 0, "arrival": 0, "took_fuel": 0, "took_cargo": 0, "arrived": 0}
        for k in range(args.steps):
            a = np.asarray(O.gen_actions(n, P, args.seed, 0, k))
            before = code[st.x, st.y].copy()
            fuel0, cargo0, org0 = st.fuel.copy(), st.cargo.copy(), st.origin.copy()
            on_port.append(float(((before > 0) & (before <= P)).mean()))
            O.step(world, st, actions=a, seed=args.seed, t=t)
            t += 1
            ok = np.asarray(st.err) == OK
            mover = ok & (a >= -4) & (a < 4)
            per_wave = lambda m: m.reshape(-1, WAVE).any(1)  # noqa: E731
            c["take"] += int(per_wave((a >= 4 + P) & (before != 0)).sum())
            c["arrival"] += int(per_wave(mover & (code[st.x, st.y] != 0)).sum())
            c["took_fuel"] += int(per_wave(ok & (a >= 54 + P) & (st.fuel > fuel0)).sum())
            c["took_cargo"] += int(per_wave(ok & (a >= 4 + P) & (a < 54 + P) & (st.cargo > cargo0)).sum())
            c["arrived"] += int(per_wave(mover & (st.origin != org0)).sum())
        ws = (n // WAVE) * args.steps
        rows.append({"preroll": pre,
                     "envs_on_a_port_cell": round(float(np.mean(on_port)), 5),
                     "take_guard_true": round(c["take"] / ws, 4), "take_guard_false": round(1 - c["take"] / ws, 4),
                     "arrival_guard_true": round(c["arrival"] / ws, 4), "arrival_guard_false": round(1 - c["arrival"] / ws, 4),
                     "wave_steps_with_a_passed_take_fuel": round(c["took_fuel"] / ws, 4),
                     "wave_steps_with_a_passed_take_cargo": round(c["took_cargo"] / ws, 4),
                     "wave_steps_with_an_arrival": round(c["arrived"] / ws, 4)})
        print(f"pre-roll {pre}: {rows[-1]}", file=sys.stderr, flush=True)
    json.dump({"what": "share of wave-steps (a wave = 256 consecutive envs) on which each guard of the state-only step votes "
                       "yes / no; C oracle, Philox draws, 5 default ports, the bench's action rows",
               "envs": n, "steps_after_preroll": args.steps, "seed": args.seed, "wave_steps": (n // WAVE) * args.steps,
               "by_preroll": rows}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
