"""The state-only steps of a fused se_step_seq skip the take work and the arrival test for a
wave that needs neither. Two wave-uniform votes, once per step and group:

* the take guard: does any env of the wave have a take action (act >= 4 + P) and stand on a
  non-water cell (the carried cell code, before the move, is not 0)?
* the arrival guard: does any env of the wave make a valid move and stand on a non-water cell
  after it?

The suites before this one keep a ship on a port in every wave, so every wave votes yes and only
the general path runs. A guard can be computed from the wrong action row or from stale codes, miss
an env slot or a lane, be evaluated per workgroup instead of per wave, or once per launch instead
of per step. So here every env but one actor is a ship at sea that shuttles between two water
cells (some with cargo, so losses fire): its wave votes no. The actor runs a scenario at one of
the env indices ACTORS: lane 0 slot 0, slot 3, lane 63 slot 3, the next wave's first lane, the
last full wave, workgroup 1's only group, the tail.

Both votes are recomputed here from actions, positions and the cell map, per wave (256
consecutive envs of the full groups) and step, on the recorded steps. Each scenario states at
which inner steps its actor's wave votes yes; every other wave votes no at every inner step, and
the actor's wave votes no at another inner step of the same run. The tests without the gpu mark
assert this on the C oracle, which is what makes the GPU tests prove that both paths ran and that
a wave changed path inside one launch.

The method is test_gpu_step_seq_trim's: a twin env stepped by K VecEnv.step calls (equal to the
oracle step by step) is the reference, one step_seq call must end in the same bits, and 2 plain
steps follow. A sparse random run on the 100 x 100 map (about one env in 64 on a port) follows,
whole and split, with and without non-temporal loads, and with several groups per thread."""
import numpy as np
import pytest

from step_seq_support import (AMOUNT, NOT_AT_PORT, OK, TAIL, assert_same, device_rows, empty_state, gpu_lib, load,  # noqa: F401
                              oracle_trace, run_fused, snapshot, twin_trace)
from test_gpu_step_seq_lean import world_of
from test_gpu_step_seq_trim import E_, K_SCN, N_, N_GENERIC, S_, SHARED, SMALL, assert_generic_coverage, ship

gpu = pytest.mark.gpu

WAVE = 256  # envs of one wave: 64 lanes, a group of 4 envs each
ACTORS = (0, 3, 255, 256, 1023, 1024, 1028)
INNER = range(K_SCN - 1)


def cell_codes(world):
    """The world image's cell codes: 0 water, 255 ground, i + 1 on port i's cell (the first port
    of a shared cell; a port is never ground)."""
    code = np.where(np.asarray(world.water) != 0, 0, 255).astype(np.int32)
    for i in reversed(range(world.P)):
        code[world.ports[i][0], world.ports[i][1]] = i + 1
    return code


def votes(world, init, acts, trace, K):
    """(take, arrive)[k][wave] of the inner steps k < K - 1 over the full groups' envs."""
    code = cell_codes(world)
    n = len(init["x"])
    full = n & ~3
    waves = [slice(s, min(s + WAVE, full)) for s in range(0, full, WAVE)]
    prev = [init] + list(trace)
    take, arrive = [], []
    for k in range(K - 1):
        a, s0, s1 = acts[k], prev[k], trace[k]
        t = (a >= 4 + world.P) & (code[s0["x"], s0["y"]] != 0)
        m = (a >= -4) & (a < 4) & (s1["err"] == OK) & (code[s1["x"], s1["y"]] != 0)
        take.append([bool(t[w].any()) for w in waves])
        arrive.append([bool(m[w].any()) for w in waves])
    return np.array(take), np.array(arrive)


# ----------------------------------------------------------------- the single actor
def scenarios():
    """[(label, world, the actor's ship, rows 0 .. K_SCN - 1, claims, the inner steps at which the
    actor's wave votes yes for a take, those for an arrival)]; a claim (k, field, value) holds
    after step k <= K_SCN - 2."""
    tc, tf = SMALL.cargo, SMALL.fuel
    sc, sf = SHARED.cargo, SHARED.fuel
    return [
        # onto port 0 (a mover on a port cell, no arrival: dest is 2), cargo == stock, stock + 1
        ("onto_port_take_cargo", SMALL, ship((2, 3), 1, 2), [N_, tc(3), tc(4), 4 + 0],
         [(0, "pos", (2, 2)), (1, "err", OK), (1, "cargo", 3), (2, "err", AMOUNT), (2, "cargo", 3)], {1, 2}, {0}),
        ("onto_port_take_fuel", SMALL, ship((2, 3), 1, 2), [N_, tf(7), tf(8), S_],
         [(0, "pos", (2, 2)), (1, "err", OK), (2, "err", AMOUNT)], {1, 2}, {0}),
        # off port 0 (onto water: no vote) and back, then a take
        ("off_and_back_take", SMALL, ship((2, 2), 1, 2), [S_, N_, tf(2), tc(1)],
         [(0, "pos", (2, 3)), (1, "pos", (2, 2)), (2, "err", OK)], {2}, {1}),
        # a move blocked by ground at (2, 1): the ship keeps port 0's code
        ("blocked_then_take", SMALL, ship((2, 2), 1, 2), [N_, tc(2), tf(7), S_],
         [(0, "pos", (2, 2)), (0, "err", OK), (1, "err", OK), (1, "cargo", 2), (2, "err", OK)], {1, 2}, {0}),
        # an arrival at port 2, then cargo == its stock
        ("arrive_then_take", SMALL, ship((6, 9), 0, 2, cargo=10), [N_, tc(9), tf(4), tf(1)],
         [(0, "pos", (6, 8)), (0, "origin", 2), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 9), (2, "err", OK)], {1, 2}, {0}),
        # a select of the port the ship stands on, then a move blocked by ground: an arrival
        # without moving; then a take there
        ("select_here_blocked_arrival", SMALL, ship((2, 2), 1, 2, cargo=0), [4 + 0, N_, tc(3), S_],
         [(0, "dest", 0), (0, "origin", 1), (1, "pos", (2, 2)), (1, "err", OK), (1, "origin", 0), (2, "err", OK), (2, "cargo", 3)],
         {2}, {1}),
        # a ship loaded onto a ground cell (code 255): the wave takes the general path, no take passes
        ("on_ground_code", SMALL, ship((4, 6), 0, 2), [4 + 1, tc(1), tf(1), tc(1)],
         [(0, "dest", 1), (1, "err", NOT_AT_PORT), (2, "err", NOT_AT_PORT)], {1, 2}, set()),
        # an arrival at port 1 on port 0's cell (its code is port 0's), then takes against port 0's stocks
        ("shared_arrive_take", SHARED, ship((4, 3), 2, 1, cargo=7), [E_, sc(2), sf(6), sc(1)],
         [(0, "pos", (3, 3)), (0, "origin", 1), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 2), (2, "err", AMOUNT)], {1, 2}, {0}),
    ]


SCN = {s[0]: s for s in scenarios()}
# rows 5 and 8 hold neither a port nor ground in SMALL and SHARED, and neither do their neighbours
SEA_ROWS = (5, 8)


def actor_run(label, actor):
    """The background and the actor's scenario at env `actor`: a ship at (row, y) moves S to
    (row, y + 1) and N back, with a destination; every fourth carries cargo 1 .. 59."""
    _, world, sh, rows, _, _, _ = SCN[label]
    n = N_GENERIC
    st = empty_state(n)
    acts = np.zeros((K_SCN + TAIL, n), np.int32)
    for i in range(n):
        st["x"][i], st["y"][i] = SEA_ROWS[i % 2], (i // 2) % (world.W - 1)
        st["origin"][i], st["dest"][i] = i % world.P, (i + 1) % world.P
        st["cargo"][i] = 1 + i % 59 if i % 4 == 0 else 0
        st["fuel"][i] = 100.0 + 0.125 * i
        acts[:, i] = [S_ if k % 2 == 0 else N_ for k in range(K_SCN + TAIL)]
    st["x"][actor], st["y"][actor] = sh["cell"]
    st["origin"][actor], st["dest"][actor], st["cargo"][actor] = sh["origin"], sh["dest"], sh["cargo"]
    acts[:K_SCN, actor] = rows
    return world, st, acts


def assert_actor_claims(label, actor, init, acts, trace):
    _, world, _, _, claims, take_at, arrive_at = SCN[label]
    for k, field, want in claims:
        assert k <= K_SCN - 2, f"{label}: a claim about the last step proves nothing about an inner one"
        got = (int(trace[k]["x"][actor]), int(trace[k]["y"][actor])) if field == "pos" else int(trace[k][field][actor])
        assert got == want, f"{label} at env {actor}: step {k} {field} {got} != {want}"
    # the background never touches a non-water cell, and some of it loses cargo in an inner step
    code = cell_codes(world)
    others = np.arange(len(init["x"])) != actor
    for s in [init] + list(trace):
        assert (code[s["x"], s["y"]][others] == 0).all(), label
    assert any((trace[k]["cargo"][others] < (init if k == 0 else trace[k - 1])["cargo"][others]).any() for k in INNER)
    take, arrive = votes(world, init, acts, trace, K_SCN)
    in_wave = actor < (len(init["x"]) & ~3)  # the tail's envs are the tail kernel's: no wave, no vote
    mine = actor // WAVE
    for name, vote, at in (("take", take, take_at), ("arrival", arrive, arrive_at)):
        want = np.zeros_like(vote)
        if in_wave:
            for k in at:
                want[k, mine] = True
        assert (vote == want).all(), f"{label} at env {actor}: the {name} votes {vote.tolist()} != {want.tolist()}"
        assert not at or len(at) < len(INNER), f"{label}: the {name} vote never changes inside the run"


def test_the_background_rows_are_open_water():
    for world in (SMALL, SHARED):
        code = cell_codes(world)
        assert all((code[r] == 0).all() for r in SEA_ROWS)
        assert world.P >= 2
    assert N_GENERIC // WAVE == 4 and N_GENERIC % WAVE == 7 and N_GENERIC % 4 == 3
    assert {a // WAVE for a in ACTORS} == {0, 1, 3, 4} and 1028 >= (N_GENERIC & ~3)
    assert cell_codes(SHARED)[3, 3] == 1 and cell_codes(SMALL)[4, 6] == 255


@pytest.mark.parametrize("label", list(SCN))
def test_actor_scenarios_hold_what_they_claim_on_the_oracle(label, oracle_mod):
    for actor in ACTORS:
        world, init, acts = actor_run(label, actor)
        assert_actor_claims(label, actor, init, acts, oracle_trace(oracle_mod, world, init, acts))


@gpu
@pytest.mark.parametrize("label", list(SCN))
def test_single_actor_fused_equals_step_calls(label, gpu_lib, oracle_mod):
    """For every actor index: the twin's recorded steps hold the claims and the votes, equal the
    oracle's step by step, and the fused run ends where the twin does."""
    world = SCN[label][1]
    a, b = world.env(N_GENERIC), world.env(N_GENERIC)
    for actor in ACTORS:
        _, init, acts = actor_run(label, actor)
        load(a, init)
        dev = device_rows(a, acts)
        trace = []
        for k in range(len(acts)):
            a.step(dev[k].contiguous())
            trace.append(snapshot(a))
        assert_actor_claims(label, actor, init, acts, trace)
        for k, want in enumerate(oracle_trace(oracle_mod, world, init, acts)):
            assert_same(trace[k], want, f"{label} at env {actor}: twin vs oracle, step {k}")
        run_fused(b, init, device_rows(b, acts), trace, K_SCN, None, f"{label} at env {actor}")
    a.close()
    b.close()


# ----------------------------------------------------------------- a sparse random run
K_SPARSE = 33
SPARSE_SEED = 7


def sparse_run(seed=SPARSE_SEED):
    """The 100 x 100 map with its 5 ports. About one env in 64 starts on a port and one in 64 on
    the cell before its destination; the rest are in open sea. Actions are drawn as
    test_gpu_step_seq_trim.generic_run draws them."""
    world = world_of(5)
    n, rows = N_GENERIC, K_SPARSE + TAIL
    rng = np.random.default_rng(seed)
    st = empty_state(n)
    for i in range(n):
        o = int(rng.integers(world.P))
        d = (o + 1 + i % (world.P - 1)) % world.P
        if i % 64 == 5:
            cell = world.ports[o]
        elif i % 64 == 37 and d in world.approach:
            cell = world.approach[d][0][1]
        else:
            cell = world.open_sea[int(rng.integers(len(world.open_sea)))]
        st["x"][i], st["y"][i] = cell
        st["origin"][i], st["dest"][i] = o, d
        st["fuel"][i] = 0.5 + 0.75 * (i % 64)
        st["cargo"][i] = i % 60
    acts = rng.integers(-6, world.A + 3, (rows, n)).astype(np.int32)
    moves = rng.integers(-4, 4, (rows, n)).astype(np.int32)
    return world, st, np.where(rng.random((rows, n)) < 0.5, moves, acts)


def assert_sparse_coverage(world, init, acts, trace):
    """Passed takes of both kinds, a loss, an arrival, out of fuel and refusals (the generic
    run's coverage: the 100 x 100 world has 5 ports as GENERIC has), and each vote both ways among
    the inner steps of the 33-step run."""
    assert world.P == 5
    assert_generic_coverage(init, acts, trace)
    take, arrive = votes(world, init, acts, trace, K_SPARSE)
    for name, vote in (("take", take), ("arrival", arrive)):
        assert vote.any() and not vote.all(), f"the {name} vote is {bool(vote.any())} at every wave-step"
        # ... and inside one wave of one launch
        assert any(vote[:, w].any() and not vote[:, w].all() for w in range(vote.shape[1])), name


def test_sparse_run_on_the_oracle(oracle_mod):
    world, init, acts = sparse_run()
    on_port = np.array([[int(init["x"][i]), int(init["y"][i])] in world.ports for i in range(N_GENERIC)])
    assert 1 / 128 < on_port.mean() < 1 / 32
    assert_sparse_coverage(world, init, acts, oracle_trace(oracle_mod, world, init, acts))


_SPARSE = []


def sparse_reference():
    """The twin's 33 + TAIL recorded steps (read-only, shared by the cases)."""
    if not _SPARSE:
        world, init, acts = sparse_run()
        _SPARSE.append((world, init, acts, twin_trace(world, init, acts)))
    return _SPARSE[0]


@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_SEQ_MAX_STEPS": "3"}, {"SHIPENV_NT_LOADS": "1"}, {"SHIPENV_NT_LOADS": "0"},
                                 {"SHIPENV_STEP_BLOCKS": "1"}], ids=lambda e: "-".join(f"{k[8:]}{v}" for k, v in e.items()) or "plain")
def test_sparse_run_fused_equals_step_calls(env, gpu_lib, oracle_mod):
    """Runs of 2 and 33 steps: whole, cut into launches of at most three steps, with and without
    non-temporal loads, and with one workgroup (several groups per thread, a vote per group)."""
    world, init, acts, trace = sparse_reference()
    assert_sparse_coverage(world, init, acts, trace)
    want = oracle_trace(oracle_mod, world, init, acts)
    for k in (0, 1, K_SPARSE - 1, K_SPARSE + TAIL - 1):
        assert_same(trace[k], want[k], f"sparse: twin vs oracle, step {k}")
    b = world.env(N_GENERIC, **env)
    dev = device_rows(b, acts)
    for K in (2, K_SPARSE):
        run_fused(b, init, dev, trace, K, None, f"sparse {env}")
    b.close()
