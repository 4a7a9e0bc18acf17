"""What a decision is worth: four policies played in closed loop on the env itself, as a record.

From reset() on the default world, --n envs take --decisions decisions each under the random
policy (sample_actions, and where the step raised one more sample, as MCTSAgent's loop does), the
navigator (VecNavigator.step), VecMCTSAgent with random playouts and VecMCTSAgent with navigator
playouts (--sims simulations, --steps playout positions, c = 1.4; navigator and playouts with the
derived refuel_below and --load). An env counts until its first step that reports done. One JSON
line per policy: the mean return per --decisions steps with its standard error, the mean arrivals
(a step after which the origin changed), the share of envs that ended, the decisions' status
counts. A recording, not a gate.

    python tools/mcts_quality.py [--n 4096] [--decisions 100] [--sims 50] [--steps 100] [--load 0] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICIES = ("random", "navigator", "mcts_random", "mcts_nav")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 12)
    p.add_argument("--decisions", type=int, default=100)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--load", type=int, default=0)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--policies", nargs="+", choices=POLICIES, default=list(POLICIES))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.vec import VecEnv

    sink = open(a.out, "a") if a.out else None
    for policy in a.policies:
        env = VecEnv(a.n, seed=a.seed, device="cuda:0")
        env.reset()
        nav = VecNavigator(env, load=a.load) if policy in ("navigator", "mcts_nav") else None
        agent = None
        if policy.startswith("mcts"):
            agent = VecMCTSAgent(env, num_simulations=a.sims, max_rollout_steps=a.steps, navigator=nav)
        ret = torch.zeros(a.n, dtype=torch.float64, device=env.device)
        arrivals = torch.zeros(a.n, dtype=torch.int64, device=env.device)
        alive = torch.ones(a.n, dtype=torch.bool, device=env.device)
        status_counts = torch.zeros(5, dtype=torch.int64, device=env.device)
        raised_steps = 0
        for t in range(a.decisions):
            origin = env.origin.clone()
            if policy == "random":
                reward, done, err = (v.clone() for v in env.step_typed(*env.sample_actions(2 * t)))
                failed = err != 0
                sty, sa, sb = env.sample_actions(2 * t + 1)
                zero = torch.zeros_like(sty)
                r2, d2, e2 = env.step_typed(torch.where(failed, sty, zero), torch.where(failed, sa, zero),
                                            torch.where(failed, sb, zero))
                reward, done, err = torch.where(failed, r2, reward), torch.where(failed, d2, done), torch.where(failed, e2, err)
            elif policy == "navigator":
                reward, done, err, _ = nav.step()
            else:
                reward, done, err = agent.step()
                status_counts += torch.bincount(agent._out[3][alive], minlength=5)
            ok = alive & (err == 0)
            ret += torch.where(ok, reward.double(), torch.zeros_like(ret))
            arrivals += (ok & (env.origin != origin)).long()
            raised_steps += int((alive & (err != 0)).sum().item())
            alive = alive & ~(ok & (done != 0))
        row = {"policy": policy, "n": a.n, "decisions": a.decisions, "load": a.load, "seed": a.seed,
               "ret_mean": round(ret.mean().item(), 3), "ret_sem": round(ret.std().item() / a.n ** 0.5, 3),
               "arrivals_mean": round(arrivals.double().mean().item(), 4),
               "share_ended": round(1.0 - alive.double().mean().item(), 5), "raised_steps": raised_steps,
               "world": "builtin 100x100, default ports", "device": torch.cuda.get_device_name(0)}
        if nav is not None:
            row["refuel_below"] = nav.refuel_below
        if agent is not None:
            row.update(sims=a.sims, playout_steps=a.steps, c=agent.exploration_param,
                       status_counts_ok_cut_raised_never_stuck=status_counts.tolist())
            agent.close()
        if nav is not None:
            nav.close()
        env.close()
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
