"""The state-only steps of a fused se_step_seq read their Philox key words from a schedule filled
once per launch (philox.h, KeySched: the FUEL draw, a GATE pool refill and the LOSS_r / ARRIVE
draws), scale the fuel cost with one FMA and one add, test a move by one compare of act - 4 against
a bound, issue their four cell lookups together, and run the loss tail of env j only in a wave where
env j of some lane fired (step_seq.h, step_lean.h).

What can go wrong: a key word of the wrong round in one of the draws, a refill drawn under a
schedule that is not the launch's, a loss tail skipped for an env that fired (or a threshold left
stale by the skip), the rank of a LOSS_r block when several envs of a quad fire in one step, a pool
entry kept or lost when a take makes a carrier, and all of it where the counter wraps 2^32 and the
quad id has a high word.

One run of 19 whole waves, a wave of 20 lanes and a tail of 3 envs (about five workgroups), at quad
ids either side of 2^32 and a counter that wraps inside it, is stepped by the C oracle; one step_seq
call of 2, 17 and 40 steps must end in the oracle's bits (x, y, origin, dest, cargo, fuel and the
last step's reward, done and err), and 2 plain steps follow. The waves start with 0, 1, 2, 5, 8, 9,
16, 17 and 64 carrier lanes, whose quads hold 1, 2, 3 and 4 envs with cargo 55: every one of them
moves in step 0, and a cargo of 50 and above fires with certainty. Actors on port 0 take cargo in
the middle of a window: from a lane that carries nothing (the wave votes again), from a lane whose
other env carries, and from a lane that lost its cargo in an arrival and takes again. K = 2 has one
inner step, fewer than any window; the wave of 20 lanes draws directly.

A wrong GATE word shows only where the gate's outcome differs. The CPU companion counts, on the
oracle alone and per kind of wave (windows of 8 with 1 to 4 and with 5 to 8 carrier lanes, windows
of 4, the direct draw), the moving carriers' gate tests whose outcome under the same quad's word of
one window earlier (one step earlier in a direct wave) differs from the outcome under the right
word: what a stale entry would change. Every kind must show at least 16; the seed is the first from
22 on with which it does."""
import collections

import numpy as np
import pytest

from step_seq_support import OK, TAIL, device_rows, gpu_lib, oracle_trace, run_fused  # noqa: F401
from test_gpu_step_seq_gatepool import (CARRIER_LANES, LANES, POOLW, WAVE, carrier_lanes, gate_thr, gate_word, ids_of, launches_of,
                                        sea_run, windows)
from test_gpu_step_seq_trim import E_, W_

gpu = pytest.mark.gpu

SEED, BASE, T0 = 22, (1 << 34) - 4 * WAVE, (1 << 32) - 9  # e1 steps from 0 to 1 after wave 3; t wraps at step 9
COUNTS = (0, 2, 5, 8, 9, 16, 17, 64, 1, 2, 5, 8, 9, 16, 17, 1, 0, 5, 9)
PART_LANES = 20
N = len(COUNTS) * WAVE + 4 * PART_LANES + 3
KS = (2, 17, 40)
K = max(KS)
HEAVY, TAKE = 55, 25  # fires with certainty; fires on half the words
PORT0, BESIDE = tuple(POOLW.ports[0]), (3, 2)  # W_ from port 0 is (3, 2), then (4, 2): water
ACTOR_LANE = 10  # in no set of CARRIER_LANES up to 16
# (wave, kind, the inner step of the take): a window of 8 or 4 is running at that step
ACTORS = ((1, "new", 1), (2, "carrying", 5), (17, "again", 9), (0, "new", 5), (4, "new", 1), (5, "new", 1), (10, "carrying", 11),
          (3, "again", 5), (16, "new", 20), (8, "new", 10))


def trim_run():
    st, acts = sea_run(N, K + TAIL)
    q = 0
    for w, count in enumerate(COUNTS):
        for lane in CARRIER_LANES[count]:
            for j in range(1 + q % 4):  # 1, 2, 3, 4 envs of the quad
                st["cargo"][w * WAVE + 4 * lane + (lane + j) % 4] = HEAVY
            q += 1
    part = len(COUNTS) * WAVE
    for lane in (0, 4, 19):
        st["cargo"][part + 4 * lane:part + 4 * lane + 1 + lane % 4] = HEAVY
    st["cargo"][N - 2] = HEAVY  # the tail kernel's
    for w, kind, k0 in ACTORS:
        i = w * WAVE + 4 * ACTOR_LANE + 1
        assert st["cargo"][i - 1:i + 3].sum() == 0
        st["x"][i], st["y"][i] = PORT0
        st["origin"][i], st["dest"][i] = 1, 2
        acts[:, i] = [(E_ if (k - k0) % 2 else W_) for k in range(K + TAIL)]
        acts[:k0, i] = [4 + 3 if k % 2 == 0 else 4 + 2 for k in range(k0)]
        acts[k0, i] = POOLW.cargo(TAKE)
        acts[k0 + 1:k0 + 3, i] = W_  # off the port: (3, 2), then (4, 2) and back
        if kind == "carrying":  # the env beside it holds cargo and never moves: the lane carries throughout
            st["cargo"][i + 1] = HEAVY
            acts[:, i + 1] = [4 + 3 if k % 2 == 0 else 4 + 2 for k in range(K + TAIL)]
        if kind == "again":  # arrives at port 0 in step 0 and loses its cargo there
            st["x"][i], st["y"][i] = BESIDE
            st["dest"][i], st["cargo"][i] = 0, 20
            acts[0, i] = E_
    return st, acts


_REF = {}


def reference(O):
    """The oracle's recorded steps (read-only, shared by the cases)."""
    if "run" not in _REF:
        init, acts = trim_run()
        trace = oracle_trace(O, POOLW, init, acts, SEED, BASE, T0)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _REF["run"] = (init, acts, trace)
    return _REF["run"]


def kind_of(mode, W, m):
    return "direct" if mode == "direct" else "pool4" if W == 4 else "pool8_1to4" if m <= 4 else "pool8_5to8"


KINDS = ("pool8_1to4", "pool8_5to8", "pool4", "direct")


def stale_tests(O, init, acts, trace, rec):
    """{kind of wave: gate tests of moving carriers in inner steps whose outcome a stale word (the
    quad's word one window, or one direct step, earlier) would change}."""
    prev = [init] + list(trace)
    out = collections.Counter()
    full = N & ~3
    for k, by_wave in rec.items():
        a, before, after = acts[k], prev[k], trace[k]
        for w, (mode, W, _, m) in by_wave.items():
            if mode == "none":
                continue
            for i in range(w * WAVE, min((w + 1) * WAVE, full)):
                if not (-4 <= a[i] < 4 and after["err"][i] == OK and before["cargo"][i] > 0):
                    continue
                thr = gate_thr(before["cargo"][i])
                right = gate_word(O, i, T0 + k, SEED, BASE) <= thr
                stale = gate_word(O, i, T0 + k - (W if mode == "pool" else 1), SEED, BASE) <= thr
                out[kind_of(mode, W, m)] += right != stale
    return out


def assert_scenario(O, init, acts, trace):
    prev = [init] + list(trace)
    rec = windows(POOLW, init, acts, trace, launches_of(K))
    assert N % 4 == 3 and (N & ~3) % WAVE == 4 * PART_LANES and 4.5 * 1024 < N < 5.5 * 1024
    assert T0 < 1 << 32 <= T0 + min(KS[1:]) - 1 and {(BASE + i) >> 34 for i in (0, N - 1)} == {0, 1}
    # the waves at the launch's start: 0, 1 to 4, 5 to 8, 9 to 16 and more than 16 carrier lanes; the partial wave
    m0 = [carrier_lanes(init["cargo"], w) for w in range(len(COUNTS))]
    for lo, hi in ((0, 0), (1, 4), (5, 8), (9, 16), (17, 64)):
        assert any(lo <= m <= hi for m in m0), (lo, hi, m0)
    assert {rec[0][w][0] for w in range(len(COUNTS))} == {"none", "pool", "direct"} and rec[0][len(COUNTS)][0] == "direct"
    assert {rec[0][w][1] for w in range(len(COUNTS)) if rec[0][w][0] == "pool"} == {4, 8}
    # step 0: every env with cargo moves and fires; quads with 1, 2, 3 and 4 of them, in pooled and in direct waves
    full = N & ~3
    heavy = (init["cargo"][:full] >= 50) & (acts[0][:full] >= -4) & (acts[0][:full] < 4) & (trace[0]["err"][:full] == OK)
    per_quad = heavy.reshape(-1, 4).sum(1)
    for pooled in (True, False):
        waves = [w for w in rec[0] if (rec[0][w][0] == "pool") == pooled and rec[0][w][0] != "none"]
        seen = {int(c) for w in waves for c in per_quad[w * LANES:(w + 1) * LANES]}
        assert seen >= {1, 2, 3, 4}, (pooled, seen)
    assert (trace[0]["cargo"][:full][heavy] < HEAVY).sum() > heavy.sum() // 2, "most of them lose cargo at once"
    # the actors
    fired_early = collections.Counter()
    for w, kind, k0 in ACTORS:
        i = w * WAVE + 4 * ACTOR_LANE + 1
        lane = slice(i - 1, i + 3)
        assert k0 < min(KS[1:]) - 1 or k0 < K - 1
        assert trace[k0]["err"][i] == OK and trace[k0]["cargo"][i] == prev[k0]["cargo"][i] + TAKE == TAKE, (w, kind)
        mode, W, s, m = rec[k0][w]
        carried = bool((prev[k0]["cargo"][lane] > 0).any())
        assert carried == (kind == "carrying"), (w, kind)
        if kind == "again":
            assert init["cargo"][i] == 20 and trace[0]["cargo"][i] == 0 and trace[0]["origin"][i] == 0, "arrives in step 0"
            assert (init["cargo"][lane] > 0).any() and not carried, "the lane was a carrier, and is none at its take"
        if mode == "pool":
            assert 0 < s < W - 1, f"wave {w}: the take at offset {s} of a window of {W}"
        # the model's rule: any take ends the window, and the vote counts the lane
        assert rec[k0 + 1][w][2] == 0 and rec[k0 + 1][w][3] == carrier_lanes(prev[k0 + 1]["cargo"], w)
        # the actor's gate fires, with a loss, before the window it took in would have ended
        end = k0 - s + W if mode == "pool" else K - 1
        lost = [k for k in range(k0 + 1, end) if trace[k]["cargo"][i] < prev[k]["cargo"][i]]
        fired_early[kind] += bool(lost) and mode == "pool"
    print(dict(fired_early))
    assert fired_early["new"] >= 2 and fired_early["again"] >= 1, "a taker's gate fires inside the window it took in"
    assert rec[ACTORS[3][2]][0][0] == "none" and rec[ACTORS[3][2] + 1][0][:2] == ("pool", 8), "the first carrier of wave 0"
    # the window running at the end of each launch is longer than the steps left
    for Kl in KS:
        r = windows(POOLW, init, acts, trace, launches_of(Kl))
        last = r[Kl - 2]
        assert any(mode == "pool" and s < W - 1 for mode, W, s, _ in last.values()), Kl
    out = stale_tests(O, init, acts, trace, rec)
    print(dict(out))
    for kind in KINDS:
        assert out[kind] >= 16, f"{kind} waves: {out[kind]} gate tests that a stale word would change"


def test_scenario_on_the_oracle(oracle_mod):
    init, acts, trace = reference(oracle_mod)
    assert_scenario(oracle_mod, init, acts, trace)


# plain, every wave direct, one workgroup (each hardware wave steps several groups under one schedule)
@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}], ids=ids_of)
def test_fused_run_equals_the_oracle(env, gpu_lib, oracle_mod):
    """Runs of 2, 17 and 40 steps from the same state end in the oracle's bits."""
    init, acts, trace = reference(oracle_mod)
    b = POOLW.env(N, seed=SEED, env_id_base=BASE, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"trim2 {env}", T0)
    b.close()
