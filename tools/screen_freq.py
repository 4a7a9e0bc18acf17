"""How often the screened GATE pool's steps are hot, on the C oracle alone (no GPU):

    python tools/screen_freq.py [--envs 32768] [--steps 1000] > profiles/seq_windows/freq.json
    python tools/screen_freq.py --rule parent      (the windows before: profiles/seq_screen/freq.json)

The bench's config 3 (Philox draws, the 5 default ports, seed 2026, its own action rows: the
pre-roll's at t = 1000000 + k, the warm-up's and the timed ones from row 0), stepped from reset
through the 1000-step pre-roll and the 50 warm-up steps, then `--steps` timed steps as one fused
launch. A wave is 256 consecutive envs (64 lanes of 4). The kernel's windows are modelled as
step_seq.h runs them (the vote, W = min(16, 64 / m) steps for m <= 16 carrier lanes, the direct run
above 16 or after two early cuts, a passed take of cargo ends a window; --rule parent: W = 8 up to 8
carrier lanes and 4 up to 16, and any step whose take block ran ends a window), and for every pooled window the GATE words
themselves are drawn (Philox4x32-10 in numpy, checked against the oracle's) and screened against
the carriers' thresholds at the vote, as the refill does. Per wave-step: is its screen bit set,
does a gate fire (the exact test), does a fire follow a fall of cargo inside the window; the hot
steps past window offset 7 and the take blocks that leave their window standing (a take of fuel, a
refused take); and the rarer events of the step (the take block, a passed take of cargo, `near`,
an arrival, a loss). It asserts that cargo never rises inside a window and that no fire falls on
a cold step.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WAVE, LANES = 256, 64
OK = 0
LIMIT, DIRECT_RUN, EARLY_CUT = 16, 16, 2  # step_seq.h: kGatePoolLimit, kGateDirectRun, kGateEarlyCut
SLOT_GATE = 7
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_word(quad, t, seed, j):
    """Word j (per element) of Philox4x32-10 at counter (quad lo, quad hi, t, SLOT_GATE), key = seed."""
    c = [(quad & 0xffffffff).astype(np.uint64), (quad >> 32).astype(np.uint64), np.full(quad.shape, t & 0xffffffff, np.uint64),
         np.full(quad.shape, SLOT_GATE, np.uint64)]
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xffffffff), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & np.uint64(0xffffffff)]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.choose(j, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 15)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rule", choices=("windows", "parent"), default="windows")
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
    thr = np.array([int(np.floor(np.ldexp(c / 50.0, 32))) for c in range(50)] + [0xffffffff], np.uint64)
    n = args.envs - args.envs % WAVE
    nw = n // WAVE
    ids = np.arange(n, dtype=np.int64)
    for i in (0, 5, n - 1):  # the numpy draw against the oracle's
        want = O.philox([i >> 2, 0, 77, SLOT_GATE], [args.seed & 0xffffffff, args.seed >> 32])[i & 3]
        assert int(philox_word(np.array([i >> 2]), 77, args.seed, np.array([i & 3]))[0]) == int(want)

    st = O.OracleState(n)
    O.reset(world, st, seed=args.seed, epoch=0)
    t = 0
    for k in range(args.preroll):
        O.step(world, st, actions=O.gen_actions(n, P, args.seed, 0, 1_000_000 + k), seed=args.seed, t=t)
        t += 1
    for k in range(args.warmup):
        O.step(world, st, actions=O.gen_actions(n, P, args.seed, 0, k), seed=args.seed, t=t)
        t += 1

    # the windows' state per wave
    need_vote = np.ones(nw, bool)
    mode = np.zeros(nw, np.int8)  # 0 none (m == 0), 1 pool, 2 direct
    W = np.zeros(nw, np.int64)
    s = np.zeros(nw, np.int64)
    cuts = np.zeros(nw, np.int64)
    left = np.zeros(nw, np.int64)  # direct steps left
    vote = np.zeros(n, np.int64)  # cargo at the wave's vote
    marks = [m for m in (100, 500, args.steps) if m <= args.steps]
    names = ("pooled", "no_carrier", "direct", "hot", "hot_fire", "hot_no_fire", "cold", "fire_after_fall_wave_steps", "refills",
             "loss_lowers_cargo", "take_block", "take_cargo_passed", "near", "arrival", "hot_past_offset_7", "take_block_inside_window")
    c = dict.fromkeys(names, 0)
    rows = []
    inner = args.steps - 1  # the launch's last step is the full one
    for k in range(args.steps):
        a = np.asarray(O.gen_actions(n, P, args.seed, 0, args.warmup + k))
        cargo0, org0 = st.cargo.copy(), st.origin.copy()
        before = code[st.x, st.y]
        if k < inner:
            carrier_lane = (cargo0.reshape(nw, LANES, 4) > 0).any(2)
            m = carrier_lane.sum(1)
            v = need_vote
            direct = v & ((m > LIMIT) | ((cuts >= 2) & (m != 0)))
            mode[direct], left[direct] = 2, DIRECT_RUN
            cuts[direct] = np.minimum(cuts[direct], 1)
            pool = v & ~direct
            mode[pool] = np.where(m[pool] != 0, 1, 0)
            W[pool] = np.where(m[pool] <= 8, 8, 4) if args.rule == "parent" else np.minimum(16, 64 // np.maximum(m[pool], 1))
            s[pool] = 0
            c["refills"] += int((pool & (m != 0)).sum())
            ve = np.repeat(v, WAVE)
            vote[ve] = cargo0[ve]
            need_vote[:] = False
        O.step(world, st, actions=a, seed=args.seed, t=t)
        ok = np.asarray(st.err) == OK
        mover = ok & (a >= -4) & (a < 4)
        per_wave = lambda x: x.reshape(nw, WAVE).any(1)  # noqa: E731
        took = per_wave((a >= 4 + P) & (before != 0))
        arrived = mover & (st.origin != org0)
        c["loss_lowers_cargo"] += int(per_wave((st.cargo < cargo0) & ~arrived).sum())
        c["take_block"] += int(took.sum())
        rose = per_wave(ok & (a >= 4 + P) & (a < 54 + P) & (st.cargo > cargo0))
        c["take_cargo_passed"] += int(rose.sum())
        cut = took if args.rule == "parent" else rose  # what ends a window
        c["near"] += int(per_wave(code[st.x, st.y] != 0).sum())
        c["arrival"] += int(per_wave(arrived).sum())
        if k < inner:
            # the words of the pooled waves' carrier lanes (carriers at the vote)
            lane_carries = np.repeat((vote.reshape(nw, LANES, 4) > 0).any(2).reshape(-1), 4)
            sel = np.repeat(mode == 1, WAVE) & lane_carries
            idx = ids[sel]
            word = philox_word(idx >> 2, t, args.seed, idx & 3)
            hot_e = np.zeros(n, bool)
            fire_e = np.zeros(n, bool)
            hot_e[idx] = word <= thr[np.clip(vote[idx], 0, 50)]
            fire_e[idx] = mover[idx] & (cargo0[idx] > 0) & (word <= thr[np.clip(cargo0[idx], 0, 50)])
            assert (cargo0[idx] <= vote[idx]).all(), "cargo rose inside a window"
            hot, fire = per_wave(hot_e), per_wave(fire_e)
            assert not (fire & ~hot).any(), f"step {k}: a gate fires on a cold step"
            # nobody outside the vote's carrier lanes loses cargo in a pooled window
            lost = (st.cargo < cargo0) & ~arrived & np.repeat(mode != 2, WAVE)
            assert not (lost & ~fire_e).any(), f"step {k}: a loss the model does not see"
            pooled = mode == 1
            c["pooled"] += int(pooled.sum())
            c["no_carrier"] += int((mode == 0).sum())
            c["direct"] += int((mode == 2).sum())
            c["hot"] += int((pooled & hot).sum())
            c["hot_fire"] += int((pooled & fire).sum())
            c["hot_no_fire"] += int((pooled & hot & ~fire).sum())
            c["cold"] += int((pooled & ~hot).sum() + (mode == 0).sum())
            c["fire_after_fall_wave_steps"] += int(per_wave(fire_e & (cargo0 < vote)).sum())
            c["hot_past_offset_7"] += int((pooled & hot & (s >= 8)).sum())
            c["take_block_inside_window"] += int(((mode != 2) & took & ~cut).sum())
            # the end of a window
            s += 1
            left -= mode == 2
            end_pool = (mode != 2) & (cut | ((mode == 1) & (s == W)))
            early = (mode == 1) & cut & (s <= EARLY_CUT)
            cuts = np.where(end_pool, np.where(early, cuts + 1, 0), cuts)
            need_vote = end_pool | ((mode == 2) & (left == 0))
        t += 1
        if k + 1 in marks:
            ws = nw * (k + 1)
            wi = nw * min(k + 1, inner)
            row = {"timed_steps": k + 1, "wave_steps": ws}
            row.update({f"share_{x}": round(c[x] / ws, 4) for x in ("loss_lowers_cargo", "take_block", "take_cargo_passed", "near", "arrival")})
            row.update({f"share_{x}": round(c[x] / wi, 4) for x in ("pooled", "no_carrier", "direct", "hot", "hot_fire", "hot_no_fire", "cold",
                                                                    "fire_after_fall_wave_steps", "hot_past_offset_7", "take_block_inside_window")})
            row["steps_per_refill"] = round(c["pooled"] / max(c["refills"], 1), 2)
            rows.append(row)
            print(row, file=sys.stderr, flush=True)
    json.dump({"what": "share of wave-steps (a wave = 256 consecutive envs) of the fused launch's inner steps by the GATE pool's mode, "
                       "and of the pooled and carrier-less ones by the refill's screen (hot: some drawn word of a carrier lane is at or "
                       "below its env's threshold at the vote; cold: the others, which test no gate); C oracle, Philox draws, 5 default "
                       "ports, the bench's action rows, after its pre-roll and warm-up. hot and cold are shares of all inner wave-steps; "
                       "a direct wave-step runs the full gate test.",
               "rule": args.rule, "envs": n, "seed": args.seed, "preroll": args.preroll, "warmup": args.warmup, "by_timed_steps": rows}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
