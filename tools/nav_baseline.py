"""What a competent ship earns: the navigator's rollouts beside the random policy's, as a record.

From reset() on the default world, --m rollouts each of se_rollout (the random policy, max_steps =
steps, max_attempts = 8 * steps) and of se_rollout_nav with load in --loads, at every length in
--steps. One JSON line per (policy, load, steps): mean, standard deviation and quantiles of the
return, mean counted steps, mean arrivals and the shares of the endings. A recording, not a gate:
whether carrying cargo pays is not known beforehand (the loss gate fires with probability
cargo / 50 per move at -3 per unit lost, against +2 per unit delivered).

    python tools/nav_baseline.py [--m 65536] [--steps 100 1000] [--loads 0 5 20] [--out profiles/nav/baseline.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def describe(ret):
    q = torch.quantile(ret, torch.tensor(QUANTILES, dtype=ret.dtype, device=ret.device))
    return {"ret_mean": round(ret.mean().item(), 4), "ret_std": round(ret.std().item(), 4),
            "ret_min": round(ret.min().item(), 4), "ret_max": round(ret.max().item(), 4),
            "ret_quantiles": {str(k): round(v, 4) for k, v in zip(QUANTILES, q.tolist())}}


def share(status, code):
    return round((status == code).double().mean().item(), 6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=1 << 16)
    p.add_argument("--steps", type=int, nargs="+", default=[100, 1000])
    p.add_argument("--loads", type=int, nargs="+", default=[0, 5, 20])
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from shippingenv_amd import _native as N
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.vec import VecEnv

    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    env = VecEnv(a.m, seed=a.seed, device="cuda:0")
    env.reset()
    src = torch.arange(a.m, dtype=torch.int32, device=env.device)
    common = {"m": a.m, "seed": a.seed, "world": "builtin 100x100, default ports", "port_fuel": env.port_fuel.tolist(),
              "port_cargo": env.port_cargo.tolist(), "device": torch.cuda.get_device_name(0)}
    base = 0
    for K in a.steps:
        ret, steps, status = env.rollout(src, max_steps=K, max_attempts=8 * K, rollout_base=base)
        base += a.m
        emit({"policy": "random", "steps": K, **describe(ret), "counted_mean": round(steps.double().mean().item(), 3),
              "arrivals_mean": None, "share_done": share(status, N.ROLL_DONE), "share_max_steps": share(status, N.ROLL_MAX_STEPS),
              "share_raised": share(status, N.ROLL_RAISED), "share_attempts": share(status, N.ROLL_ATTEMPTS), **common})
        for load in a.loads:
            nav = VecNavigator(env, load=load)
            res = nav.rollout(src, steps=K, rollout_base=base)
            base += a.m
            emit({"policy": "navigator", "load": load, "refuel_below": nav.refuel_below, "max_leg": nav.max_leg, "steps": K,
                  **describe(res.ret), "counted_mean": round(res.steps.double().mean().item(), 3),
                  "arrivals_mean": round(res.arrivals.double().mean().item(), 4),
                  "raised_total": int(res.raised.sum().item()), "share_done": share(res.status, N.PLAN_DONE),
                  "share_end": share(res.status, N.PLAN_END), "share_stuck": share(res.status, N.PLAN_STUCK), **common})
            nav.close()
    env.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
