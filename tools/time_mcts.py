"""MCTS decisions per second (se_mcts_choose through VecMCTSAgent) at the reference's defaults:
S = 50 simulations, 100-step rollouts, the default map and five ports, from config-3 states
after a 50-step pre-roll, for n = 2^12 .. 2^18. Beside each decision batch the yardstick: one
se_rollout batch of n rollouts from the same states, S of which are nearly all of a decision's
env steps; ratio = decision / (S x rollout batch) is the tree's overhead. Both are timed with
events, alternating, `--runs` times. One JSON line per n.

    python tools/time_mcts.py [--log2n 12 18] [--runs 3] [--sims 50] [--steps 100] [--playout random|nav|both]

--playout nav times se_mcts_choose_nav instead (VecMCTSAgent with a VecNavigator of --load and the
derived refuel_below; its yardstick is one se_rollout_nav batch); both times the two decisions
of one build in alternating rounds from the same states (nav_* fields beside the random ones).

--cpu-reference DIR times the reference's own MCTSAgent.choose_action (DIR: a checkout of the
reference, for agents/ and utils/) on the N = 1 drop-in host stepper instead: a CPU number, for
scale. It needs no GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_reference(ref, decisions, sims, steps):
    import random

    sys.path.insert(0, ref)  # agents/ and utils/ only: `shipping` resolves to the drop-in
    sys.path.insert(0, os.path.join(ROOT, "shippingenv_amd", "dropin"))
    os.chdir(ref)  # the agent opens the map by its bare file name (agents/mcts.py:190)
    from agents.mcts import MCTSAgent
    from shipping import Environment

    random.seed(1)
    env = Environment("mapa_mundi_binario.jpg")
    for p in [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]:
        env.add_port(list(p))
    state = env.reset()
    agent = MCTSAgent(env, num_simulations=sims, max_rollout_steps=steps)
    agent.choose_action(state)  # warm
    ms = []
    for _ in range(decisions):
        t0 = time.perf_counter()
        action = agent.choose_action(state)
        ms.append((time.perf_counter() - t0) * 1e3)
        try:
            state = env.step(action)[0]
        except Exception:  # noqa: BLE001 - the reference's loop samples again; timing goes on
            pass
    ms.sort()
    print(json.dumps({"cpu_reference": True, "stepper": "host drop-in", "sims": sims, "steps": steps,
                      "decisions": decisions, "ms_per_decision_median": round(ms[len(ms) // 2], 2),
                      "ms_per_decision_min": round(ms[0], 2), "ms_per_decision_max": round(ms[-1], 2)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log2n", type=int, nargs=2, default=(12, 18))
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--sims", type=int, default=50)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--playout", choices=("random", "nav", "both"), default="random")
    p.add_argument("--load", type=int, default=0, help="--playout nav / both: the navigator's load")
    p.add_argument("--cpu-reference", metavar="DIR")
    p.add_argument("--decisions", type=int, default=10, help="--cpu-reference: decisions timed")
    a = p.parse_args()
    if a.cpu_reference:
        return cpu_reference(os.path.abspath(a.cpu_reference), a.decisions, a.sims, a.steps)
    import torch

    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.vec import VecEnv

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for k in range(a.log2n[0], a.log2n[1] + 1):
        n = 1 << k
        env = VecEnv(n, seed=a.seed, device="cuda:0")
        env.reset()
        for t in range(50):
            env.step(env.gen_actions(t))
        src = torch.arange(n, dtype=torch.int32, device=env.device)
        row = {"n": n, "sims": a.sims, "steps": a.steps}
        legs = []  # (field prefix, agent, one batch of n rollouts of its playout policy -> counted steps)
        nav = None
        if a.playout in ("random", "both"):
            agent = VecMCTSAgent(env, num_simulations=a.sims, max_rollout_steps=a.steps)
            legs.append(("", agent, lambda base: env.rollout(src, max_steps=a.steps, rollout_base=base)[1]))
        if a.playout in ("nav", "both"):
            nav = VecNavigator(env, load=a.load)
            agent = VecMCTSAgent(env, num_simulations=a.sims, max_rollout_steps=a.steps, navigator=nav)
            legs.append(("nav_", agent, lambda base: nav.rollout(src, steps=a.steps, rollout_base=base).steps))
            row.update(load=a.load, refuel_below=nav.refuel_below)
        for _, agent, rollouts in legs:  # warm
            agent.choose_action()
            rollouts(0)
        torch.cuda.synchronize()
        dec, roll, counted = ({pre: [] for pre, _, _ in legs} for _ in range(3))
        for r in range(a.runs):
            for pre, agent, rollouts in legs:
                dec[pre].append(timed(agent.choose_action))
                kept = []
                roll[pre].append(timed(lambda: kept.append(rollouts((r + 1) * n))))
                counted[pre].append(float(kept[0].sum().item()) / n)
        for pre, agent, _ in legs:
            status = torch.bincount(agent.choose_action()[3], minlength=5 if pre else 4).tolist()
            d, b = sorted(dec[pre])[a.runs // 2], sorted(roll[pre])[a.runs // 2]
            row.update({pre + "decision_ms": [round(v, 4) for v in dec[pre]],
                        pre + "rollout_batch_ms": [round(v, 4) for v in roll[pre]],
                        pre + "counted_steps_per_rollout": round(sum(counted[pre]) / a.runs, 2),
                        pre + "decisions_per_s": round(n / (d * 1e-3), 1),
                        pre + "ratio_decision_over_sims_x_rollout_batch": round(d / (a.sims * b), 3),
                        pre + "status_counts": status})
            agent.close()
        if nav is not None:
            nav.close()
        print(json.dumps(row), flush=True)
        env.close()


if __name__ == "__main__":
    main()
