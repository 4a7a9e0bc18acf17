"""SARSA vector steps per second (se_sarsa_step through VecSARSAAgent) at the default world (the
100 x 100 map, five ports: a 0.99 GB table and 0.49 GB of claim words), n = 2^12 .. 2^20, with
epsilon 1.0 and 0.1, after a warm phase of `--warm` learning steps at epsilon 1 that puts values
into the table. Beside it the yardstick: a bare se_step of a second env of the same n on the
synthetic agent's actions. The three are timed with events over `--steps` steps each,
alternating, `--runs` times. One JSON line per n.

    python tools/time_sarsa.py [--log2n 12 20] [--runs 3] [--steps 1000] [--warm 300] [--out profiles/sarsa/time_sarsa.jsonl]

--table sparse times the sparse table (VecSARSAAgent(table="sparse")) instead, --table both the
two kinds on twin envs of one seed, window by window in turn (dense 1.0, sparse 1.0, dense 0.1,
sparse 0.1, se_step). Before the warm phase and before every window the sparse agent reserves
room for the rows the window can add (reserve(), outside the timed window), so that nothing is
dropped; each line carries the pages used, the capacity and the bytes held at the end.
--ports 64 puts 64 random water ports on the map (config 4's world: 2.96e8 rows of 108 entries,
which only the sparse table can hold); --max-table-gb bounds the sparse table.

--curve N STEPS records a learning curve instead: n = N envs train for STEPS vector steps with
epsilon_decay `--decay` (the reference's 0.999 per episode needs some 10^5 vector steps to leave
exploration), one JSON line per `--window` steps: the mean return of the episodes that finished
in the window, their number, epsilon.

--cpu-reference DIR times the reference's own SARSAAgent.train (DIR: a checkout of the
reference, for agents/ and utils/) on the N = 1 drop-in host stepper instead: steps per second
on one CPU core, for scale. It needs no GPU. test_policy is stubbed on the instance: greedy on a
young table it never returns.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = [None]  # --out: a file every result line is appended to as well (profiles/sarsa/*.jsonl)


def emit(doc):
    line = json.dumps(doc)
    print(line, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(line + "\n")


def cpu_reference(ref, steps, runs):
    import random

    sys.path.insert(0, ref)  # agents/ and utils/ only: `shipping` resolves to the drop-in
    sys.path.insert(0, os.path.join(ROOT, "shippingenv_amd", "dropin"))
    os.chdir(ref)
    from agents.sarsa import SARSAAgent
    from shipping import Environment

    random.seed(1)
    env = Environment("mapa_mundi_binario.jpg")
    for p in [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]:
        env.add_port(list(p))
    agent = SARSAAgent(env)
    agent.test_policy = lambda *a, **k: {}
    agent.train(episodes=10**9, verbose=False, max_total_steps=steps // 10)  # warm
    for _ in range(runs):
        t0 = time.perf_counter()
        res = agent.train(episodes=10**9, verbose=False, max_total_steps=steps)
        dt = time.perf_counter() - t0
        emit({"cpu_reference": True, "stepper": "host drop-in", "steps": steps,
              "episodes": len(res.episode_rewards), "steps_per_s": round(steps / dt, 1),
              "epsilon": round(agent.epsilon, 6), "table_entries": len(agent.q_table)})


def curve(a):
    from shippingenv_amd.sarsa import VecSARSAAgent
    from shippingenv_amd.vec import VecEnv

    n, steps = a.curve
    env = VecEnv(n, seed=a.seed, device="cuda:0")
    env.reset()
    agent = VecSARSAAgent(env, epsilon_decay=a.decay)
    done = 0
    while done < steps:
        k = min(a.window, steps - done)
        eps0 = agent.epsilon
        episodes, ret = agent.train(k, sync_every=a.sync)
        done += k
        emit({"curve": True, "n": n, "vector_steps": done, "episodes": episodes,
              "mean_return": round(ret / episodes, 3) if episodes else None,
              "epsilon_start": round(eps0, 5), "epsilon_end": round(agent.epsilon, 5), "epsilon_decay": a.decay})
    agent.close()
    env.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log2n", type=int, nargs=2, default=(12, 20))
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--warm", type=int, default=300)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--curve", type=int, nargs=2, metavar=("N", "STEPS"))
    p.add_argument("--decay", type=float, default=0.99)
    p.add_argument("--window", type=int, default=5000)
    p.add_argument("--sync", type=int, default=100)
    p.add_argument("--cpu-reference", metavar="DIR")
    p.add_argument("--out", metavar="FILE", help="append every result line to FILE as well")
    p.add_argument("--table", choices=("dense", "sparse", "both"), default="dense")
    p.add_argument("--ports", type=int, choices=(5, 64), default=5)
    p.add_argument("--max-table-gb", type=float, default=96.0)
    a = p.parse_args()
    OUT[0] = os.path.abspath(a.out) if a.out else None
    if a.cpu_reference:
        return cpu_reference(os.path.abspath(a.cpu_reference), a.steps, a.runs)
    if a.curve:
        return curve(a)
    import torch

    from shippingenv_amd.sarsa import VecSARSAAgent
    from shippingenv_amd.vec import VecEnv, builtin_water, random_water_ports

    ports = random_water_ports(builtin_water(), 64, seed=3) if a.ports == 64 else None
    kinds = ("dense", "sparse") if a.table == "both" else (a.table,)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps  # us per step

    for k in range(a.log2n[0], a.log2n[1] + 1):
        n = 1 << k
        envs, agents = {}, {}
        for kind in kinds:  # twins: the same seed, so the same episodes
            envs[kind] = VecEnv(n, seed=a.seed, ports=ports, device="cuda:0")
            envs[kind].reset()
            agents[kind] = VecSARSAAgent(envs[kind], table=kind, max_table_bytes=int(a.max_table_gb * 2**30)) \
                if kind == "sparse" else VecSARSAAgent(envs[kind])
        bare = VecEnv(n, seed=a.seed + 1, ports=ports, device="cuda:0")
        bare.reset()
        acts = [bare.gen_actions(t) for t in range(16)]  # a cycle of 16 action rows

        def room(kind, steps):
            if kind == "sparse":
                agents[kind].reserve(steps * n)

        filled = {}
        for kind, agent in agents.items():
            room(kind, a.warm)
            for _ in range(a.warm):
                agent.step(epsilon=1.0)
            torch.cuda.synchronize()
            filled[kind] = int(torch.count_nonzero(agent.pages if kind == "sparse" else agent.q))

        def sarsa(kind, eps):
            agent = agents[kind]
            for _ in range(a.steps):
                agent.step(epsilon=eps)

        def plain():
            for t in range(a.steps):
                bare.step(acts[t & 15])

        windows = [(kind, name, eps) for name, eps in (("eps_1.0", 1.0), ("eps_0.1", 0.1)) for kind in kinds]
        us = {kind: {"eps_1.0": [], "eps_0.1": []} for kind in kinds}
        ended = {kind: {"eps_1.0": [], "eps_0.1": []} for kind in kinds}
        us_plain = []
        for _ in range(a.runs):
            for kind, name, eps in windows:
                room(kind, a.steps)
                us[kind][name].append(timed(lambda: sarsa(kind, eps)))
                ended[kind][name].append(float(agents[kind].ended.sum().item()) / n)
            us_plain.append(timed(plain))
        med_plain = sorted(us_plain)[len(us_plain) // 2]
        for kind in kinds:
            agent = agents[kind]
            all_us = dict(us[kind], se_step=us_plain)
            med = {name: sorted(v)[len(v) // 2] for name, v in all_us.items()}
            status = torch.bincount(agent.status, minlength=4).tolist()
            doc = {"n": n, "steps": a.steps, "warm": a.warm}
            if a.table != "dense" or a.ports != 5:
                doc.update({"table": kind, "ports": a.ports})
            if kind == "sparse":
                st = agent.stats()
                doc.update({"capacity": st["capacity"], "pages_used": st["used"], "dropped": st["dropped"],
                            "table_bytes": st["capacity"] * (agent.A * 8 + 8), "claim_bytes": st["capacity"] * agent.A * 4,
                            "used_bytes": st["used"] * (agent.A * 8 + 8)})
            else:
                doc.update({"table_bytes": agent.q.numel() * 8, "claim_bytes": agent.q.numel() * 4})
            doc.update({"entries_nonzero_after_warm": filled[kind],
                        "us_per_step": {name: [round(x, 3) for x in v] for name, v in all_us.items()},
                        "env_steps_per_s": {name: round(n / (m * 1e-6), 1) for name, m in med.items()},
                        "ratio_sarsa_over_se_step": {name: round(med[name] / med_plain, 2) for name in ("eps_1.0", "eps_0.1")},
                        "ended_fraction_last_step": {name: round(sum(v) / len(v), 5) for name, v in ended[kind].items()},
                        "status_counts_last_step": status})
            emit(doc)
        for kind in kinds:
            agents[kind].close()
            envs[kind].close()
        bare.close()
        del agents, envs, bare, acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
