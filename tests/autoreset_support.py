"""Dense auto-reset steps: hand-built cases in which a chosen set of envs finishes in one step,
and what the C oracle says that step must leave behind. Shared by test_autoreset_dense_cpu.py
(the cases are what they claim to be) and test_gpu_autoreset_dense.py (the kernels against them).

A ship dies exactly when it moves with less fuel than the move costs (environment.py:288-290),
and the cost of a unit move is 1 + uniform(-0.1, 0.1) (:103-104): fuel 0.5 always dies, fuel
150 never does. So a case chooses its dying envs: they get fuel 0.5 and a move, the others fuel
150 and the synthetic agent's mix (whose TAKE_* at sea and SELECT of the origin raise).

World: 9 x 13, all water, four ports, every ship at (4, 6) with origin 1 and dest 0, so any move
stays on the map and reaches no port; a reset ship stands on a port, from which any move stays on
the map too. Cargo 0 / 30 / 60 by env index, so the loss gate and the LOSS ranks run beside the
resets, on dying envs as well.

Dying masks over env index i (lane = (i // 4) % 64, j = i % 4, wave = i // 256): see mask().

numpy and the oracle only: nothing here needs a GPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

H, W = 9, 13
PORTS = [(1, 2), (2, 10), (7, 1), (7, 11)]
PORT_FUEL = [5, 20, 11, 16]
PORT_CARGO = [20, 7, 13, 5]
START = (4, 6)
ORIGIN, DEST = 1, 0
CARGO = (0, 30, 60)
SEED = 60221
DEAD_FUEL, LIVE_FUEL = 0.5, 150.0

N_TAIL_APPENDS = 1350  # 4 * (64 * 5 + 17) + 2: five full waves, a wave of 17 lanes, a 2-env tail group
N_TAIL_FRESH = 1283    # 4 * 64 * 5 + 3: the tail group opens segment 5
N_RECORD = 1024        # no tail: se_step_record's one-launch shape
SIZES = (N_TAIL_APPENDS, N_TAIL_FRESH, N_RECORD)
PATTERNS = ("all", "none", "counts", "totals", "random50", "random5")
SEG = 256              # envs (and records) of one done-list segment: 64 lanes of 4
FILLER_RUN = 8         # SHIPENV_DONE_PAD: a wave's records padded to runs of 8 (one 128-byte line)
SENTINEL = -7
WAVE_TOTALS = (1, 7, 8, 9, 255)  # `totals`, waves 0..4; every env after wave 4 dies


def water():
    return np.ones((H, W), np.uint8)


def mask(pattern, n):
    """The envs that finish, as a bool array."""
    i = np.arange(n)
    lane, j, wave, k = (i // 4) % 64, i % 4, i // SEG, i % SEG
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "counts":  # the quad's mask is lane % 16: all 16 masks, every count 0..4
        return ((lane % 16) >> j & 1).astype(bool)
    if pattern == "totals":
        per_wave = [k == 255, k < 7, k < 8, (100 <= k) & (k < 109), k != 128]
        m = wave > 4
        for w, sel in enumerate(per_wave):
            m = m | ((wave == w) & sel)
        return m
    if pattern == "random50":
        return np.random.default_rng(5001).random(n) < 0.5
    if pattern == "random5":
        return np.random.default_rng(5002).random(n) < 0.05
    raise ValueError(pattern)


def second_pattern(pattern):
    """The pattern of a case's second step: every pattern follows one and precedes one."""
    return PATTERNS[(PATTERNS.index(pattern) + 2) % len(PATTERNS)]


def actions_for(O, m, t, salt):
    """A move for the dying envs, the synthetic agent's mix (invalid actions included) for the rest."""
    n = len(m)
    rng = np.random.default_rng(7000 + salt)
    moves = rng.integers(0, 4, n).astype(np.int32)
    return np.where(m, moves, O.gen_actions(n, len(PORTS), SEED, 0, t & 0xFFFFFFFF)).astype(np.int32)


def fuel_for(m):
    return np.where(m, DEAD_FUEL, LIVE_FUEL).astype(np.float64)


def oracle_world(O):
    return O.OracleWorld(water(), [p[0] for p in PORTS], [p[1] for p in PORTS], PORT_FUEL, PORT_CARGO)


def initial(n, salt):
    """State and running episodes before the first step: a return in [-30, 10) and a length in
    [0, 50) for every env."""
    rng = np.random.default_rng(9000 + salt)
    i = np.arange(n)
    return SimpleNamespace(
        x=np.full(n, START[0], np.int32), y=np.full(n, START[1], np.int32),
        cargo=np.array(CARGO, np.int32)[i % 3], origin=np.full(n, ORIGIN, np.int32),
        dest=np.full(n, DEST, np.int32),
        ep_return=(rng.random(n) * 40.0 - 30.0).astype(np.float32),
        ep_len=rng.integers(0, 50, n).astype(np.int32))


def stamps(t, ep_len):
    """Episode-start stamps of running lengths at step counter t: (t - len) mod 2^32, as the
    int32 the device tensor holds."""
    return ((int(t) - ep_len.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


FIELDS = ("x", "y", "fuel", "cargo", "origin", "dest")


def snapshot(st):
    return SimpleNamespace(**{f: getattr(st, f).copy() for f in FIELDS + ("reward", "done", "err", "ep_return", "ep_len")})


def expected(before, after, t, start_before):
    """What one auto-reset step at step counter t (any width; taken mod 2^32) must leave, from the
    oracle's state before and after it. For the finished envs in env order: env, ret (the f32
    return of the finished episode), len, step; counts[s] of segment s = envs [256 s, 256 s + 256);
    start: the stamps after the step, (t + 1) mod 2^32 where done, start_before elsewhere."""
    t32 = int(t) & 0xFFFFFFFF
    done = after.done != 0
    env = np.nonzero(done)[0].astype(np.int32)
    rew = after.reward.astype(np.float32)
    ret = (before.ep_return + rew).astype(np.float32)[env]
    length = (before.ep_len + 1).astype(np.int32)[env]
    step = np.full(len(env), np.array(t32, np.uint32).view(np.int32), np.int32)
    n = len(done)
    nseg = (n + SEG - 1) // SEG
    counts = np.bincount(env // SEG, minlength=nseg).astype(np.int32)
    new_stamp = np.array((t32 + 1) & 0xFFFFFFFF, np.uint32).view(np.int32)
    start = np.where(done, new_stamp, start_before).astype(np.int32)
    return SimpleNamespace(env=env, ret=ret, len=length, step=step, counts=counts, start=start, done=done,
                           recs=np.stack([env, ret.view(np.int32), length, step], axis=1).astype(np.int32))


def raw_half(exp, n, nseg, t, pad):
    """One half of the done list, [nseg * 256, 4] int32, after a step at counter t onto a half
    prefilled with the sentinel record: each segment's records from its start; with pad, filler
    records (env -1, return 0, length 0, the step) from the count of the full groups' records up
    to the next multiple of FILLER_RUN, the partial last group's records written over them
    (wave_compact, step_tail_envs); the sentinel everywhere else. Also the counts."""
    t32 = np.array(int(t) & 0xFFFFFFFF, np.uint32).view(np.int32)
    half = np.full((nseg * SEG, 4), SENTINEL, np.int32)
    counts = np.zeros(nseg, np.int32)
    counts[:len(exp.counts)] = exp.counts
    full_envs = n & ~3
    for s in range(nseg):
        sel = exp.env // SEG == s
        k = int(sel.sum())
        by_wave = int((sel & (exp.env < full_envs)).sum())  # the tail group's records come after
        if pad and by_wave:
            run = by_wave + (-by_wave) % FILLER_RUN
            half[s * SEG + by_wave:s * SEG + run] = (-1, 0, 0, t32)
        half[s * SEG:s * SEG + k] = exp.recs[sel]
    return half, counts


@functools.lru_cache(maxsize=None)
def _case(pattern, n, t0):
    from oracle import oracle as O

    O.build()
    world = oracle_world(O)
    salt = PATTERNS.index(pattern) * 8 + SIZES.index(n)
    ini = initial(n, salt)
    st = O.OracleState(n)
    for f in ("x", "y", "cargo", "origin", "dest"):
        getattr(st, f)[:] = getattr(ini, f)
    st.ep_return[:] = ini.ep_return
    st.ep_len[:] = ini.ep_len
    start = stamps(t0, ini.ep_len)
    steps = []
    stats = np.zeros(3, np.float64)
    for k, pat in enumerate((pattern, second_pattern(pattern))):
        t = t0 + k
        m = mask(pat, n)
        st.fuel[:] = fuel_for(m)  # refuelled by hand before every step
        acts = actions_for(O, m, t, salt + 100 * k)
        before = snapshot(st)
        step_stats = O.step_autoreset(world, st, acts, seed=SEED, t=t & 0xFFFFFFFF)
        after = snapshot(st)
        exp = expected(before, after, t, start)
        start = exp.start
        stats += step_stats
        steps.append(SimpleNamespace(pattern=pat, t=t, mask=m, fuel=fuel_for(m), actions=acts, before=before,
                                     after=after, exp=exp, stats=step_stats))
    case = SimpleNamespace(pattern=pattern, n=n, t0=t0, initial=ini, start0=stamps(t0, ini.ep_len), steps=steps)
    for obj in [ini] + steps + [s.before for s in steps] + [s.after for s in steps] + [s.exp for s in steps]:
        for v in vars(obj).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    case.start0.setflags(write=False)
    return case


def case(pattern, n, t0=7):
    """Two consecutive auto-reset steps from step counter t0 (computed once and shared,
    read-only): steps[0] finishes mask(pattern), steps[1] mask(second_pattern(pattern)) from the
    state the first left, both refuelled by hand. Each step holds its actions, the fuel to load,
    the oracle's snapshots before and after, the oracle's stats of that step and expected()."""
    return _case(pattern, n, int(t0))


def sequential_sum(values):
    """f64 additions in order, as the oracle accumulates its statistics."""
    s = 0.0
    for v in values:
        s += float(v)
    return s
