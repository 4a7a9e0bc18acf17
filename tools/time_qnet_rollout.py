"""Network-policy rollouts (se_rollout_qnet) on one GPU, the default world, by events, in
alternating rounds, against the only other way to the same answer: `steps` x (se_policy + se_step)
on a second env set holding the same states.

    rollout_qnet     one launch: m rollouts of --steps greedy positions (mode 0, the bf16 network)
    policy_step_loop --steps x (QPolicy.act(0) + VecEnv.step) on a copy of the envs: 2 x steps launches

Both legs play a seeded torch-default-init DQNNetwork, greedy, from the states after reset() and
--preroll random steps. The legs alternate within a round; a run of a leg is timed between two
events, the loop's env copy being put back to the start states before each run, outside the events;
--runs runs per leg and round, after --warm unrecorded runs of each. One JSON line per leg, size and
round, then a summary line per size with each leg's median and range over the rounds and the ratio
of the medians. The fp32-faithful rollout (mode 1) is not built and is not timed.

Then a recording with no target: a VecDQNAgent trained for --train iterations at --train-envs
auto-reset envs, its evaluate() beside the navigator's (load 0) and the random policy's rollouts
from the same states under the same rollout ids.

    python tools/time_qnet_rollout.py [--sizes 4096 65536 1048576] [--steps 100] [--rounds 5] [--runs 3]
                                      [--warm 3] [--preroll 50] [--train 3000 (0: no recording)] [--train-envs 4096]
                                      [--out profiles/qnet_rollout/time_qnet_rollout.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATE = ("x", "y", "fuel", "cargo", "origin", "dest")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[1 << 12, 1 << 16, 1 << 20])
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--warm", type=int, default=3)
    p.add_argument("--preroll", type=int, default=50)
    p.add_argument("--train", type=int, default=3000)
    p.add_argument("--train-envs", type=int, default=1 << 12)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_qnet_rollout.py measures on a GPU: none found")
    from shippingenv_amd.dqn import VecDQNAgent
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.policy import DQNNetwork, QPolicy
    from shippingenv_amd.vec import VecEnv

    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    K = a.steps
    for m in a.sizes:
        env = VecEnv(m, seed=a.seed, device="cuda:0")
        env.reset()
        for t in range(a.preroll):
            env.step(env.gen_actions(t))
        torch.manual_seed(a.seed)
        model = DQNNetwork(env.obs_size, env.action_space_size)
        pol = QPolicy(env, model)
        twin = VecEnv(m, seed=a.seed, device="cuda:0")  # the loop's envs
        tpol = QPolicy(twin, model)
        start = {f: getattr(env, f).clone() for f in STATE}
        src = torch.arange(m, dtype=torch.int32, device=env.device)

        def restore():
            for f in STATE:
                getattr(twin, f).copy_(start[f])

        def rollout_leg(base):
            r = pol.rollout(src, steps=K, epsilon=0.0, rollout_base=base)
            return r.counted

        def loop_leg(base):
            for k in range(K):
                twin.step(tpol.act(0.0, k))
            return None

        legs = {"rollout_qnet": rollout_leg, "policy_step_loop": loop_leg}
        for _ in range(max(a.warm, 1)):
            for run in legs.values():
                restore()
                run(0)
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        base = m
        for r in range(a.rounds):
            for name, run in legs.items():
                total, counted = 0.0, 0
                for _ in range(a.runs):
                    restore()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    c = run(base)
                    e1.record()
                    torch.cuda.synchronize()
                    total += e0.elapsed_time(e1)
                    counted += 0 if c is None else int(c.sum().item())
                    base += m
                ms = total / a.runs
                times[name].append(ms)
                emit({"leg": name, "m": m, "round": r, "runs": a.runs, "ms_per_run": round(ms, 4),
                      "launches_per_run": 1 if name == "rollout_qnet" else 2 * K,
                      "counted_steps_per_run": counted / a.runs if name == "rollout_qnet" else None})
        med = {name: statistics.median(v) for name, v in times.items()}
        emit({"summary": {name: {"median_ms": round(med[name], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                          for name, v in times.items()},
              "ratio_rollout_over_loop": round(med["rollout_qnet"] / med["policy_step_loop"], 4),
              "m": m, "steps": K, "rounds": a.rounds, "runs": a.runs, "warm": a.warm, "preroll": a.preroll,
              "mode": 0, "epsilon": 0.0, "device": torch.cuda.get_device_name(0)})
        for h in (tpol, pol, twin, env):
            h.close()

    if a.train <= 0:
        if sink:
            sink.close()
        return
    # a recording: what a trained network earns, beside the navigator and the random policy
    n = a.train_envs
    env = VecEnv(n, seed=a.seed, device="cuda:0", auto_reset=True)
    env.reset()
    agent = VecDQNAgent(env)
    agent.train(a.train)
    nav = VecNavigator(env, load=0)
    base = 1 << 32
    by_port = agent.evaluate(steps=K, rollout_base=base)
    greedy = agent.rollout(None, steps=K, epsilon=0.0, rollout_base=base)
    src = torch.arange(n, dtype=torch.int32, device=env.device)
    navr = nav.rollout(src, steps=K, rollout_base=base)
    rnd, _, _ = env.rollout(src, max_steps=K, max_attempts=K, rollout_base=base)
    status = greedy.status.cpu()
    emit({"recording": "trained_dqn", "train_iterations": a.train, "train_envs": n, "updates": agent.updates,
          "epsilon_after": agent.epsilon, "steps": K, "mean_cargo_aboard": round(float(env.cargo.double().mean().item()), 2),
          "evaluate_by_start_port": {str(k): round(v, 3) for k, v in by_port.items()},
          "dqn_greedy_mean_ret": round(float(greedy.ret.mean().item()), 3),
          "dqn_greedy_mean_counted": round(float(greedy.counted.double().mean().item()), 3),
          "dqn_status_counts": {str(s): int((status == s).sum().item()) for s in sorted(set(status.tolist()))},
          "navigator_mean_ret": round(float(navr.ret.mean().item()), 3),
          "random_mean_ret": round(float(rnd.mean().item()), 3)})
    for h in (nav, agent, env):
        h.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
