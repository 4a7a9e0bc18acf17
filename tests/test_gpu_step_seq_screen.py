"""The GATE pool of a fused se_step_seq screens its words at the refill (step_seq.h, "The screen"):
each carrier lane hands its four gate thresholds over with its seed, the lane that draws a block
compares the block's words with them, and the folded ballot is one bit per window offset. A step
whose bit is clear is cold: it reads no pool entry, tests no gate and has no loss branch. That is
exact because inside a window cargo only falls and the threshold never rises as cargo falls; a take
ends the window. SHIPENV_SEQ_SCREEN=0 makes every step hot (the loop before the screen).

What can go wrong: a threshold row at the wrong rank or from the wrong lane, the fold either side of
W = 8 and W = 4, a bit read at the wrong offset or past a run that ends inside its window, a screen
kept after a take raised a carrier's threshold, a screen that forgets a carrier whose cargo fell but
still fires, and do_move missing where a cold step's arrival test reads it. A missed fire shows as
cargo that is not lost, so the CPU companion counts, per kind of wave, the cold steps, the hot steps
on which a gate fires and on which none does, and the fires that follow a fall of cargo inside the
window; it fails if a count is 0, and it asserts that no fire of the oracle falls on a cold step.

The method is step_seq_support's: a twin env stepped by plain steps, the C oracle's trace, and one
step_seq call of 2, 17 and 40 steps (39 inner steps: four windows of 8 and a run that ends inside
the fifth), all equal bit for bit, with 2 plain steps after, under {}, SHIPENV_SEQ_SCREEN=0,
SHIPENV_SEQ_GATE_POOL=0 and SHIPENV_SEQ_RING=0, from counter 0 and with the counter wrapping 2^32
inside the first window. The envs are whole waves of 0, 1, 8, 9, 16 and 17 carrier lanes, the
scripted ships' wave, a wave of 20 lanes and a tail of 3 envs, at sea in
test_gpu_step_seq_gatepool's world and moving every step. The carriers hold 55 (the gate fires for
certain: hot on every step until a partial loss, after which the same window may fire again), 30
(these move on every other step only: hot steps on which nothing fires) and 1 (cold windows); the
one carrier lane of its wave holds all three. The scripted ships: one carries 30, arrives at port
0 at step 1 (cargo 0 in mid-window) and takes 20 there at step 3 (a take by a lane that lost its
cargo); one sits on port 0 with cargo 5 and takes 20 more at step 5 (a take by a carrier, offset 1
of the second window); one sits there with no cargo in a lane without any and takes 25 at step 10
(offset 4 of the third window). The wave of 17 draws directly, with the full gate test, until
carriers have lost their whole cargo (7 pooled steps at the run's end, 23 with the wrap), so no count is
asked of it. The second scenario is test_gpu_step_seq_ring's hand-built run, whose world has two
ports on one cell and a ship that arrives at the second of them; its CPU companion is in that file.
The third holds a ship loaded with a destination past the last port as its wave's only irregular
env (bad_dest_run); the C oracle indexes its port table with the destination, so that run is
compared with the twin alone.

The counts of the companion (printed with -s), as (cold, hot with a fire, hot without, fires after a
fall of cargo inside the window) over the 39 inner steps, from counter 0: 1 lane (18, 17, 4, 9),
8 lanes (20, 12, 7, 2), 9 lanes (17, 20, 2, 12), 16 lanes (14, 19, 6, 8), the scripted ships' wave
(23, 9, 7, 2); the wave without carriers runs 39 cold steps. With the wrap: (27, 9, 3, 7),
(16, 15, 8, 6), (16, 14, 9, 6), (16, 22, 1, 12), (23, 8, 8, 1)."""
import numpy as np
import pytest

from step_seq_support import OK, TAIL, assert_same, device_rows, gpu_lib, oracle_trace, run_fused, twin_trace  # noqa: F401
from test_gpu_step_seq_gatepool import (CARRIER_LANES, IDS, LANES, POOLW, WAVE, gate_thr, gate_word, launches_of, sea_run,
                                        windows)
from test_gpu_step_seq_ring import HAND
from test_gpu_step_seq_ring import N as N_HAND
from test_gpu_step_seq_ring import hand_run
from test_gpu_step_seq_trim import E_, N_, S_, W_

gpu = pytest.mark.gpu

COUNTS = (0, 1, 8, 9, 16, 17, 0)  # the last: the scripted ships' wave, two carrier lanes with them
PART_LANES = 20
N = len(COUNTS) * WAVE + 4 * PART_LANES + 3
KS = (2, 17, 40)
K = max(KS)
MIX = (55, 1, 30, 55, 1)  # the carriers' cargo, by their rank in the wave
SETTINGS = [{}, {"SHIPENV_SEQ_SCREEN": "0"}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_RING": "0"}]
ACTOR_WAVE = 6
# (lane, env slot) of the scripted ships
ARRIVER, CARRIER_TAKER, NEW_TAKER = (10, 0), (20, 1), (30, 2)
ARRIVE_AT, TAKES = 1, {ARRIVER: (3, 20), CARRIER_TAKER: (5, 20), NEW_TAKER: (10, 25)}


def ids_of(env):
    return "-".join(f"{k[8:].lower()}{v}" for k, v in env.items()) or "plain"


def env_of(actor):
    return ACTOR_WAVE * WAVE + 4 * actor[0] + actor[1]


def screen_run():
    rows = K + TAIL
    st, acts = sea_run(N, rows)
    for w, count in enumerate(COUNTS):
        for r, lane in enumerate(CARRIER_LANES[count]):
            i = w * WAVE + 4 * lane
            if count == 1:  # the one carrier lane holds four carriers
                st["cargo"][i:i + 4] = (55, 1, 30, 55)
            else:
                st["cargo"][i + lane % 4] = MIX[r % len(MIX)]
            if count == 1 or r % len(MIX) == 2:  # the carrier of 30 moves on every other step: hot steps without a fire
                e = i + 2 if count == 1 else i + lane % 4
                acts[:, e] = [(S_, 4 + 0, N_, 4 + 0)[k % 4] for k in range(rows)]
    for lane in (0, 7, 19):  # the wave of 20 lanes (it draws directly) and the tail
        st["cargo"][len(COUNTS) * WAVE + 4 * lane + lane % 4] = 55
    st["cargo"][N - 2] = 55
    port0 = tuple(POOLW.ports[0])
    for actor, (k0, amount) in TAKES.items():
        i = env_of(actor)
        st["x"][i], st["y"][i] = port0
        st["origin"][i], st["dest"][i], st["cargo"][i] = 1, 2, 0
        # selects until the take, then off the port: (3, 2), (4, 2) and back and forth
        acts[:, i] = [(E_ if (k - k0) % 2 else W_) for k in range(rows)]
        acts[:k0, i] = [4 + 3 if k % 2 == 0 else 4 + 2 for k in range(k0)]
        acts[k0, i] = POOLW.cargo(amount)
        acts[k0 + 1, i] = acts[k0 + 2, i] = W_
    a = env_of(ARRIVER)  # two cells south of port 0, bound for it
    st["x"][a], st["y"][a] = port0[0], port0[1] + 2
    st["origin"][a], st["dest"][a], st["cargo"][a] = 1, 0, 30
    acts[:2, a] = [N_, N_]
    acts[2, a] = 4 + 1  # a select of the port it left: passes or not, the ship stays
    st["cargo"][env_of(CARRIER_TAKER)] = 5
    return st, acts


N_BAD = 2 * WAVE + 3
BAD_ENV, BAD_DEST = 4 * 9 + 2, POOLW.P + 1


def bad_dest_run():
    """Two whole waves at sea and a tail; one ship of wave 0 is loaded with a destination past the
    last port, one cell south of port 3, and moves onto it. The step clamps the index of the port it
    compares positions with, so this ship arrives "at port 3"; a wave that took it for regular and
    tested the arrival by the cell code would not see that. The C oracle indexes its port table
    with the destination, so this run has the twin alone for its reference."""
    st, acts = sea_run(N_BAD, K + TAIL)
    for w in (0, 1):
        for r, lane in enumerate(CARRIER_LANES[8]):
            st["cargo"][w * WAVE + 4 * lane + lane % 4] = MIX[r % len(MIX)]
    x, y = POOLW.ports[3]
    st["x"][BAD_ENV], st["y"][BAD_ENV] = x, y + 1
    st["origin"][BAD_ENV], st["dest"][BAD_ENV], st["cargo"][BAD_ENV] = 0, BAD_DEST, 30
    acts[:, BAD_ENV] = 4 + 0  # after the first move: selects of its origin, which fail
    acts[0, BAD_ENV] = N_
    return st, acts


def carriers(cargo, wave):
    return int((cargo[wave * WAVE:(wave + 1) * WAVE].reshape(LANES, 4) > 0).any(1).sum())


def screen_counts(O, init, acts, trace, ids):
    """{wave: [cold, hot with a fire, hot without, fires after a fall]} over the inner steps of the
    run of K steps in pooled windows and windows without a carrier, from the model of the windows
    and the drawn words themselves; asserts that every fire falls on a hot step."""
    seed, base, t0 = IDS[ids]
    rec = windows(POOLW, init, acts, trace, launches_of(K))
    prev = [init] + list(trace)
    out = {w: [0, 0, 0, 0] for w in range(len(COUNTS))}
    for k, by_wave in sorted(rec.items()):
        for w, (mode, _, s, m) in by_wave.items():
            if w >= len(COUNTS) or mode == "direct":
                continue
            vote = prev[k - s]["cargo"]
            hot, fires, after_fall = False, 0, 0
            for lane in range(LANES if m else 0):
                i0 = w * WAVE + 4 * lane
                if not (vote[i0:i0 + 4] > 0).any():
                    continue  # no carrier lane at the vote: nobody drew its blocks
                for i in range(i0, i0 + 4):
                    word = gate_word(O, i, t0 + k, seed, base)
                    hot |= word <= gate_thr(vote[i])
                    before = prev[k]["cargo"][i]
                    if -4 <= acts[k][i] < 4 and trace[k]["err"][i] == OK and before > 0 and word <= gate_thr(before):
                        fires += 1
                        after_fall += before < vote[i]
                    assert before <= vote[i], f"step {k} env {i}: cargo rose inside a window"
            assert hot or not fires, f"step {k} wave {w}: a gate fires on a cold step"
            # no fire from a lane outside the vote's carriers either: cargo falls only where a word fires
            sl = slice(w * WAVE, (w + 1) * WAVE)
            fell = (trace[k]["cargo"][sl] < prev[k]["cargo"][sl]) & (trace[k]["origin"][sl] == prev[k]["origin"][sl])
            assert hot or not fell.any(), f"step {k} wave {w}: cargo lost on a cold step"
            c = out[w]
            c[0] += not hot
            c[1] += hot and fires > 0
            c[2] += hot and fires == 0
            c[3] += after_fall
    return out


def assert_scenario(O, init, acts, trace, ids):
    assert N % 4 == 3 and [carriers(init["cargo"], w) for w in range(len(COUNTS))] == [0, 1, 8, 9, 16, 17, 2]
    a, c, n = env_of(ARRIVER), env_of(CARRIER_TAKER), env_of(NEW_TAKER)
    assert trace[ARRIVE_AT]["cargo"][a] == 0 and trace[ARRIVE_AT]["origin"][a] == 0 and trace[0]["origin"][a] == 1
    assert trace[3]["cargo"][a] == 20 and trace[3]["err"][a] == OK, "the lane that lost its cargo takes"
    assert trace[4]["cargo"][c] == 5 and trace[5]["cargo"][c] == 25 and trace[5]["err"][c] == OK, "a carrier takes"
    assert init["cargo"][n // 4 * 4:n // 4 * 4 + 4].sum() == 0 and trace[10]["cargo"][n] == 25 and trace[10]["err"][n] == OK
    rec = windows(POOLW, init, acts, trace, launches_of(K))
    # the takes fall inside their windows and end them; the last window is cut by the run's end
    assert [rec[k][ACTOR_WAVE][2] for k in (3, 4, 5, 6, 10, 11)] == [3, 0, 1, 0, 4, 0]
    assert all(rec[k][ACTOR_WAVE][0] == "pool" for k in range(12))
    assert rec[K - 2][2][:3] == ("pool", 8, (K - 2) % 8) and (K - 1) % 8 != 0
    assert all(r[0][0] == "none" for r in rec.values()) and all(r[7][0] == "direct" for r in rec.values())
    assert {rec[k][3][1] for k in rec if rec[k][3][0] == "pool"} == {4, 8} and rec[0][4][:2] == ("pool", 4)
    assert rec[0][5][0] == "direct" and rec[K - 2][5][0] == "pool"
    t0 = IDS[ids][2]
    if ids == "wrap":
        assert t0 >> 32 == 0 and (t0 + 7) >> 32 == 1 and rec[0][2][:3] == ("pool", 8, 0)
    counts = screen_counts(O, init, acts, trace, ids)
    print(ids, counts)
    assert counts[0] == [K - 1, 0, 0, 0], "the wave without carriers: every inner step cold"
    # the wave of 17 draws directly (the full gate test) until carriers lose their whole cargo: no count asked of it
    for w in (w for w in range(1, len(COUNTS)) if COUNTS[w] != 17):
        assert all(v > 0 for v in counts[w]), f"wave {w} ({COUNTS[w]} carrier lanes): a count is 0: {counts[w]}"


_REF = {}


def oracle_reference(O, ids):
    if ids not in _REF:
        seed, base, t0 = IDS[ids]
        init, acts = screen_run()
        trace = oracle_trace(O, POOLW, init, acts, seed, base, t0)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _REF[ids] = (init, acts, trace)
    return _REF[ids]


_TWIN = {}


def twin_reference(O, name, ids):
    """The twin's recorded steps, equal to the oracle's step by step (read-only, shared by the cases)."""
    if (name, ids) not in _TWIN:
        seed, base, t0 = IDS[ids]
        if name == "screen":
            world, (init, acts, want) = POOLW, oracle_reference(O, ids)
        elif name == "hand":
            world = HAND
            init, acts = hand_run()
            want = oracle_trace(O, HAND, init, acts, seed, base, t0)
        else:
            world, want = POOLW, None
            init, acts = bad_dest_run()
        trace = twin_trace(world, init, acts, seed, base, t0)
        for k in range(len(acts) if want is not None else 0):
            assert_same(trace[k], want[k], f"{name} {ids}: twin vs oracle, step {k}")
        if name == "bad_dest":  # the ship arrives at the clamped port on its first step
            assert BAD_DEST > POOLW.P - 1 and init["dest"][BAD_ENV] == BAD_DEST and trace[0]["origin"][BAD_ENV] == BAD_DEST
            assert trace[0]["cargo"][BAD_ENV] == 0 and (trace[0]["x"][BAD_ENV], trace[0]["y"][BAD_ENV]) == tuple(POOLW.ports[3])
        _TWIN[name, ids] = (world, init, acts, trace)
    return _TWIN[name, ids]


@pytest.mark.parametrize("ids", list(IDS))
def test_screen_scenario_on_the_oracle(ids, oracle_mod):
    init, acts, trace = oracle_reference(oracle_mod, ids)
    assert_scenario(oracle_mod, init, acts, trace, ids)


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("name", ["screen", "hand", "bad_dest"])
def test_screened_run_equals_the_twin_and_the_oracle(name, ids, env, gpu_lib, oracle_mod):
    """Runs of 2, 17 and 40 steps from the same state end in the twin's bits, which are the oracle's."""
    seed, base, t0 = IDS[ids]
    world, init, acts, trace = twin_reference(oracle_mod, name, ids)
    b = world.env({"screen": N, "hand": N_HAND, "bad_dest": N_BAD}[name], seed=seed, env_id_base=base, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"screen {name} {ids} {env}", t0)
    b.close()
