"""Table-policy rollouts (se_rollout_sarsa) on one GPU, the default world, by events, in alternating
rounds, beside the navigator's and the random policy's rollouts from the same states:

    sarsa_dense_eps0      the dense table, greedy
    sarsa_sparse_eps0     the sparse table holding the same map, greedy
    sarsa_dense_eps0.1    the dense table, one position in ten explored (slot 22 drawn everywhere)
    rollout_nav           se_rollout_nav (load 0)
    rollout               se_rollout (max_steps = max_attempts = steps)

The five legs alternate within a round, m = n rollouts of --steps positions each, every env once,
--launches launches per leg and round between two events, after --warm unrecorded launches of
every leg. Two phases: "untouched" (the dense table all zero, the sparse one empty: every greedy
choice is SELECT 0, which raises wherever the ship is at sea or the port is its origin, so every
other position is a fallback sample) and "trained" (the table after --train learning steps of a
dense learner at --train-envs envs on the same world, copied into the dense table and, its rows
with a non-zero entry, into the sparse one). One JSON line per leg and round (events ms per
launch, the counted steps and the stuck rollouts per launch), then a summary line per phase with
each leg's median and range over the rounds.

    python tools/time_table_rollout.py [--n 1048576] [--steps 100] [--rounds 7] [--launches 3]
                                       [--warm 10] [--preroll 50] [--train 3000] [--train-envs 4096]
                                       [--out profiles/table_rollout/time_table_rollout.jsonl]

The states are those after reset() and --preroll random steps. There is no target: the record is
what the tool is for.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rounds(legs, a, count, emit, phase, extra):
    for _ in range(max(a.warm, 1)):
        for run in legs.values():
            run(0)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    base = count
    for r in range(a.rounds):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kept = []
            e0.record()
            for _ in range(a.launches):
                kept.append(run(base))
                base += count
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.launches
            times[name].append(ms)
            emit({"phase": phase, "leg": name, "round": r, "n": count, "launches": a.launches, "kernel_ms": round(ms, 4),
                  "counted_steps_per_launch": sum(int(c.sum().item()) for c, _ in kept) / a.launches,
                  "stuck_per_launch": sum(int((s == 5).sum().item()) for _, s in kept) / a.launches})
    emit(dict({"phase": phase, "summary": {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                                                  "max_ms": round(max(v), 4)} for name, v in times.items()},
               "n": count, "steps": a.steps, "rounds": a.rounds, "launches": a.launches, "warm": a.warm, "preroll": a.preroll,
               "device": torch.cuda.get_device_name(0)}, **extra))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--launches", type=int, default=3)
    p.add_argument("--warm", type=int, default=10)
    p.add_argument("--preroll", type=int, default=50)
    p.add_argument("--train", type=int, default=3000)
    p.add_argument("--train-envs", type=int, default=1 << 12)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.sarsa import VecSARSAAgent
    from shippingenv_amd.vec import VecEnv

    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    n, K = a.n, a.steps
    env = VecEnv(n, seed=a.seed, device="cuda:0")
    env.reset()
    for t in range(a.preroll):
        env.step(env.gen_actions(t))
    nav = VecNavigator(env, load=0)
    dense = VecSARSAAgent(env)
    sparse = VecSARSAAgent(env, table="sparse", capacity=64)
    emit({"phase": "world", "P": env.P, "H": env.H, "W": env.W, "rows": dense.rows, "A": dense.A,
          "dense_table_bytes": dense.rows * dense.A * 8, "row_bytes": dense.A * 8})
    src = torch.arange(n, dtype=torch.int32, device=env.device)

    def table_leg(agent, eps):
        def run(base):
            r = agent.rollout(src, steps=K, epsilon=eps, rollout_base=base)
            return r.counted, r.status
        return run

    def nav_leg(base):
        r = nav.rollout(src, steps=K, rollout_base=base)
        return r.steps, r.status

    def random_leg(base):
        _, steps, status = env.rollout(src, max_steps=K, max_attempts=K, rollout_base=base)
        return steps, torch.where(status == 2, 5, status)  # SE_ROLL_RAISED is the stuck ending

    legs = {"sarsa_dense_eps0": table_leg(dense, 0.0), "sarsa_sparse_eps0": table_leg(sparse, 0.0),
            "sarsa_dense_eps0.1": table_leg(dense, 0.1), "rollout_nav": nav_leg, "rollout": random_leg}
    rounds(legs, a, n, emit, "untouched", {"sparse_capacity": sparse.capacity, "sparse_used": 0})

    # the trained table: a dense learner at train-envs envs on the same world (the same seed draws the same stocks)
    small = VecEnv(a.train_envs, seed=a.seed, device="cuda:0")
    assert small.port_cargo.tolist() == env.port_cargo.tolist() and small.port_fuel.tolist() == env.port_fuel.tolist()
    small.reset()
    learner = VecSARSAAgent(small)
    episodes, ret = learner.train(a.train)
    dense.q.copy_(learner.q)
    held = torch.nonzero((learner.q != 0).any(1)).view(-1)
    sparse._install(held.cpu().numpy(), learner.q[held].cpu().numpy())
    torch.cuda.synchronize()
    extra = {"train_steps": a.train, "train_envs": a.train_envs, "train_episodes": episodes, "epsilon_after": learner.epsilon,
             "rows_with_an_entry": int(held.numel()), "sparse_capacity": sparse.capacity, "sparse_used": sparse.stats()["used"]}
    learner.close()
    small.close()
    rounds(legs, a, n, emit, "trained", extra)
    for h in (sparse, dense, nav, env):
        h.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
