"""The pooled window loop of a fused se_step_seq (step_seq.h, "The wave's GATE pool") at every way
out of a window: after an even and after an odd number of its steps, by a take of cargo, by the
window's last step and by the run's last inner step. The action row of step k + 1 is loaded ahead of
step k's arithmetic, so every exit hands the loaded row on: to the next window, to the direct run,
to the run's last step. The suite was written for a loop of two steps per turn, the two action
register sets swapping roles, whose halves each have the window's exit; that loop was measured and
not kept ("carried cell address"), and the suite stays for the loop as it is and
for the day the pair is taken up again ("first half" and "second half" below are the even and the
odd steps of a window).

What can go wrong: a step run on the wrong row's actions after an exit (a copy missing, or one too
many), a row loaded twice or skipped when a window ends on an odd step, a window of odd length that
runs one step over, the screen or the pool entry of step s read at s + 1, the direct run entered
and left with the rows out of step.

The method is step_seq_support's, on test_gpu_step_seq_windows' first world (7 x 9, five ports on
distinct cells): a twin env stepped by plain steps, the C oracle's trace, and one step_seq call of
2, 3, 4, 5, 17, 18, 40 and 41 steps (1, 2, 3, 4, 16, 17, 39 and 40 inner steps: a run ends after
the first and after the second half of a turn, at a window's last step and one step into the next),
all equal bit for bit in state, reward, done and err, with 2 plain steps after, under {},
SHIPENV_SEQ_GATE_POOL=0, SHIPENV_SEQ_RING=0 and SHIPENV_STEP_BLOCKS=1, from counter 0 and with the
counter wrapping 2^32.
  wave 0, wave 1: 7 and 9 carrier lanes at sea: windows of 9 and of 7 steps, which end in the first
    half of a turn.
  wave 2: 17 carrier lanes: the direct run; one of the carriers arrives at step 2 and has no cargo
    at the next vote, so the wave comes back to the pool (16 lanes, windows of 4).
  wave 3 (TAKERS): two light carriers at sea and four ships on port 2 that take 49 of cargo at steps
    3, 8, 10 and 17: at offsets 3, 4, 1 and 6 of their windows, so two windows end after the second
    half of a turn and two after the first. Each then leaves the port on every other step, and its
    gate (49 of 50) fires before the window it cut would have ended.
  a wave of 20 lanes and a tail of 3 envs.

The CPU companion asserts all of that on the oracle's trace with test_gpu_step_seq_windows' model of
the windows, and fails if a case does not happen."""
import numpy as np
import pytest

from step_seq_support import OK, TAIL, assert_same, device_rows, gpu_lib, oracle_trace, run_fused, twin_trace  # noqa: F401
from test_gpu_step_seq_gatepool import IDS, WAVE, launches_of
from test_gpu_step_seq_trim import E_, N_, W_
from test_gpu_step_seq_windows import CARRIER_LANES, MIX, PORT2, WIN, env_of, place, sea_run, windows

gpu = pytest.mark.gpu

KS = (2, 3, 4, 5, 17, 18, 40, 41)
K = max(KS)
SETTINGS = [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_RING": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}]
COUNTS = (7, 9, 17)
DIRECT_WAVE, TAKERS_WAVE, WAVES = 2, 3, 4
PART_LANES = 20
N = WAVES * WAVE + 4 * PART_LANES + 3
TAKE = 49  # port 2's stock of cargo: the gate of a ship that holds it fires for 49 words of 50
TAKERS = {(10, 0): 3, (20, 1): 8, (30, 2): 10, (40, 3): 17}  # (lane, env slot): the step of its take
OFFSETS = [3, 4, 1, 6]  # of those steps in their windows
DIRECT_ARRIVER = (8, 0)  # a carrier lane of the wave of 17
ARRIVES_AT = 2


def ids_of(env):
    return "-".join(f"{k[8:].lower()}{v}" for k, v in env.items()) or "plain"


def pair_run():
    rows = K + TAIL
    st, acts = sea_run(N, rows)
    for w, count in enumerate(COUNTS):
        for r, lane in enumerate(CARRIER_LANES[count]):
            st["cargo"][w * WAVE + 4 * lane + lane % 4] = MIX[r % len(MIX)]
    # the carrier of the wave of 17 that arrives: selects port 2 (it stays), then onto it from the south
    place(st, acts, env_of(DIRECT_WAVE, DIRECT_ARRIVER), (PORT2[0], PORT2[1] + 1), 0, 1, 30, [4 + 2] * ARRIVES_AT + [N_], (4 + 0, 4 + 1))
    for lane in (1, 62):  # the wave TAKERS: two light ships at sea
        st["cargo"][TAKERS_WAVE * WAVE + 4 * lane + lane % 4] = 1
    for actor, k0 in TAKERS.items():  # selects until the take, then off the port and back: (4, 4), (3, 4)
        place(st, acts, env_of(TAKERS_WAVE, actor), PORT2, 1, 0, 0, [4 + 3 if k % 2 == 0 else 4 + 4 for k in range(k0)] + [WIN.cargo(TAKE)], (W_, E_))
    for lane in (0, 7, 19):  # the wave of 20 lanes and the tail
        st["cargo"][WAVES * WAVE + 4 * lane + lane % 4] = 55
    st["cargo"][N - 2] = 55
    return st, acts


def assert_scenario(init, acts, trace, ids):
    assert N % 4 == 3 and {(Kl - 1) % 2 for Kl in KS} == {0, 1} and {16, 17} <= {Kl - 1 for Kl in KS}
    assert WIN.cargo_stock[2] == TAKE and tuple(WIN.ports[2]) == PORT2
    rec = windows(WIN, init, acts, trace, launches_of(K))
    prev = [init] + list(trace)
    # windows of odd length, each ending in the first half of a turn; the wave of 17 draws directly
    assert rec[0][0][:2] == ("pool", 9) and rec[0][1][:2] == ("pool", 7) and rec[0][DIRECT_WAVE][0] == "direct"
    # ... and comes back: its arriver has no cargo at the second vote
    a = env_of(DIRECT_WAVE, DIRECT_ARRIVER)
    assert prev[ARRIVES_AT]["cargo"][a] > 0 and trace[ARRIVES_AT]["cargo"][a] == 0 and trace[ARRIVES_AT]["origin"][a] == 2
    back = [k for k in range(1, K - 1) if rec[k][DIRECT_WAVE][0] == "pool"]
    assert back and back[0] == 16 and rec[16][DIRECT_WAVE][3] <= 16, "the wave of 17 never pools"
    # the takes: each passes in a pooled window, at its offset, and the next step starts a new window
    offsets = []
    for actor, k0 in TAKERS.items():
        i = env_of(TAKERS_WAVE, actor)
        assert prev[k0]["cargo"][i] == 0 and trace[k0]["cargo"][i] == TAKE and trace[k0]["err"][i] == OK
        mode, W, s, m = rec[k0][TAKERS_WAVE]
        assert mode == "pool" and m >= 1 and rec[k0 + 1][TAKERS_WAVE][0] == "pool" and rec[k0 + 1][TAKERS_WAVE][2] == 0
        offsets.append(s)
        end = k0 - s + W  # where the window it cut would have ended
        lost = [k for k in range(k0 + 1, min(end, K - 1)) if trace[k]["cargo"][i] < prev[k]["cargo"][i]]
        assert lost, f"env {i}: no cargo lost in steps {k0 + 1} .. {end - 1}"
    print(ids, "take offsets", offsets, "the wave of 17 pools from step", back[0], "with", rec[back[0]][DIRECT_WAVE][3], "carrier lanes")
    assert offsets == OFFSETS and {s % 2 for s in offsets} == {0, 1}
    assert all(rec[k][TAKERS_WAVE][0] == "pool" for k in range(K - 1)), "the takers' wave never leaves the pool"


_REF = {}


def oracle_reference(O, ids):
    if ids not in _REF:
        seed, base, t0 = IDS[ids]
        init, acts = pair_run()
        trace = oracle_trace(O, WIN, init, acts, seed, base, t0)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _REF[ids] = (init, acts, trace)
    return _REF[ids]


_TWIN = {}


def twin_reference(O, ids):
    """The twin's recorded steps, equal to the oracle's step by step (read-only, shared by the cases)."""
    if ids not in _TWIN:
        seed, base, t0 = IDS[ids]
        init, acts, want = oracle_reference(O, ids)
        trace = twin_trace(WIN, init, acts, seed, base, t0)
        for k in range(len(acts)):
            assert_same(trace[k], want[k], f"pair {ids}: twin vs oracle, step {k}")
        _TWIN[ids] = trace
    return _TWIN[ids]


@pytest.mark.parametrize("ids", list(IDS))
def test_pair_scenario_on_the_oracle(ids, oracle_mod):
    init, acts, trace = oracle_reference(oracle_mod, ids)
    assert_scenario(init, acts, trace, ids)


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
def test_paired_run_equals_the_twin_and_the_oracle(ids, env, gpu_lib, oracle_mod):
    """Runs of every length in KS from the same state end in the twin's bits, which are the oracle's."""
    seed, base, t0 = IDS[ids]
    init, acts, _ = oracle_reference(oracle_mod, ids)
    trace = twin_reference(oracle_mod, ids)
    b = WIN.env(N, seed=seed, env_id_base=base, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"pair {ids} {env}", t0)
    b.close()
