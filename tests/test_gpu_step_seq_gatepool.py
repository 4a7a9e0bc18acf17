"""The state-only steps of a fused se_step_seq take their GATE words from a wave-private pool
(step_seq.h, "The wave's GATE pool"). When its pool is empty a wave counts its carrier lanes (a
lane one of whose four envs has cargo > 0), m. With m == 0 it draws no GATE block; with m <= 16
the carriers hand their quads' four words over through LDS, every lane draws one carrier's block
for one of the next W steps (W = 8 for m <= 8, else 4), and for W steps each lane reads its words
from pool entry rank * W + offset; above 16, or in a wave with a lane past the last full group,
it draws directly for 16 steps. A step whose take block ran ends the window, and after two
refilled windows in a row that a take ended within 2 steps the wave draws directly for 16 steps
(one more such window sends it there again): a wave of ships in port must not refill every step.

What can go wrong: the rank or the offset of an entry, the window size either side of 8 and 16,
a counter or quad id word lost on the way through LDS, a window kept after a take made a new
carrier, a pool left over from the launch, the group or the path before, and a refill in a wave
with lanes missing. A wrong GATE word shows only when the gate's outcome differs, so each CPU
companion counts, on the C oracle alone, the moving carriers' gate tests per window size and
offset, and bounds the chance that a wrong word at that offset would pass them all.

The model of the kernel's windows (`windows`) is computed from states and actions alone: which
wave votes when, what it counts, and at which offset of which window every inner step runs. The
tests without the gpu mark assert on the C oracle that each scenario holds what it claims.

The method is test_gpu_step_seq_guards': a twin env stepped by K VecEnv.step calls (equal to the
oracle step by step) is the reference, one step_seq call must end in the same bits, and 2 plain
steps follow. The background is ships at sea that shuttle between two water cells."""
import numpy as np
import pytest

from step_seq_support import (OK, TAIL, assert_same, device_rows, empty_state, gpu_lib, oracle_trace, run_fused,  # noqa: F401
                              twin_trace)
from test_gpu_step_seq_guards import cell_codes
from test_gpu_step_seq_trim import E_, N_, S_, W_, World, generic_reference

gpu = pytest.mark.gpu

WAVE, LANES = 256, 64  # envs and lanes of one wave
LIMIT, DIRECT_RUN = 16, 16  # the kernel's: carrier lanes up to which a wave pools; steps between two votes above it
EARLY_CUT = 2  # a refilled window that a take ends within this many steps was cut early
SLOT_GATE = 7
SEED = 22

# SMALL's geometry (test_gpu_step_seq_trim) with 49 cargo at port 0: the amounts a take can ask for
# end at 49, the cargo with the highest gate probability below 1 (gate_thr[49] / 2^32 = 0.98)
POOLW = World(ports=[(2, 2), (2, 5), (6, 8), (0, 9)], fuel=[7, 0, 4, 5], cargo=[49, 0, 9, 6], ground=[(2, 1), (4, 6)])
SEA_ROWS = (5, 8)  # neither a port nor ground there, nor beside them


def gate_thr(cargo):
    """The world image's gate table: floor(fl(c / 50) * 2^32), 2^32 - 1 from 50 on."""
    c = min(max(int(cargo), 0), 50)
    return 0xffffffff if c == 50 else int(np.floor(np.ldexp(c / 50.0, 32)))


def gate_word(O, env, t, seed=SEED, env_id_base=0):
    """Word env % 4 of the quad's GATE block at counter t (the contract: key = seed, counter =
    (quad id, t, slot))."""
    quad = (env_id_base + env) >> 2
    blk = O.philox([quad & 0xffffffff, quad >> 32, t & 0xffffffff, SLOT_GATE], [seed & 0xffffffff, seed >> 32])
    return int(blk[env & 3])


# ----------------------------------------------------------------- the model of the windows
def launches_of(K, mark_after=None, max_steps=None):
    """[(first step, one past the last)] of the fused launches of a K-step run."""
    cuts = [0] + ([mark_after] if mark_after else []) + [K]
    out = []
    for a, b in zip(cuts, cuts[1:]):
        while b - a > (max_steps or K):
            out.append((a, a + max_steps))
            a += max_steps
        out.append((a, b))
    return out


def windows(world, init, acts, trace, launches):
    """rec[k][wave] = (mode, W, offset, m) of every inner step k of the launches, for the waves of
    the full groups; mode "pool", "none" (m == 0: no draw) or "direct". A launch's last step is the
    full step and has no record. A wave with a lane past the last full group is direct throughout."""
    code = cell_codes(world)
    n = len(init["x"])
    full = n & ~3
    prev = [init] + list(trace)
    nw = (full + WAVE - 1) // WAVE
    rec = {}
    for w in range(nw):
        sl = slice(w * WAVE, min((w + 1) * WAVE, full))
        whole = sl.stop - sl.start == WAVE
        for a, b in launches:
            k, cuts = a, 0  # cuts: refilled windows in a row that a take cut early
            while k < b - 1:
                cargo = prev[k]["cargo"][sl]
                m = int((np.pad(cargo, (0, WAVE - len(cargo))).reshape(LANES, 4) > 0).any(1).sum())
                if not whole or m > LIMIT or (cuts >= 2 and m):
                    for _ in range(min(DIRECT_RUN, b - 1 - k)):
                        rec.setdefault(k, {})[w] = ("direct", 0, 0, m)
                        k += 1
                    cuts = min(cuts, 1)
                    continue
                W = 8 if m <= 8 else 4
                took = False
                for s in range(min(W, b - 1 - k) if m else b - 1 - k):
                    rec.setdefault(k, {})[w] = ("pool" if m else "none", W, s, m)
                    took = bool(((acts[k][sl] >= 4 + world.P) & (code[prev[k]["x"][sl], prev[k]["y"][sl]] != 0)).any())
                    k += 1
                    if took:
                        break
                cuts = cuts + 1 if took and m and s + 1 <= EARLY_CUT else 0
    return rec


def gate_tests(O, world, init, acts, trace, launches, seed=SEED, env_id_base=0, t0=0):
    """{(W, offset): [(fired, p)]} over the gate tests of moving carriers in pooled windows: p is
    the chance that another, uniform word gives the same outcome. Also checks the model of the gate
    against the oracle: cargo falls only where the word fires."""
    rec = windows(world, init, acts, trace, launches)
    prev = [init] + list(trace)
    out = {}
    for k, by_wave in rec.items():
        a, before, after = acts[k], prev[k], trace[k]
        for w, (mode, W, s, _) in by_wave.items():
            for i in range(w * WAVE, min((w + 1) * WAVE, len(a) & ~3)):
                if not (-4 <= a[i] < 4 and after["err"][i] == OK and before["cargo"][i] > 0):
                    continue
                thr = gate_thr(before["cargo"][i])
                fired = gate_word(O, i, t0 + k, seed, env_id_base) <= thr
                arrived = after["origin"][i] != before["origin"][i]
                assert fired or arrived or after["cargo"][i] == before["cargo"][i], (k, i)
                if mode == "pool":
                    p = (thr + 1) / 2.0 ** 32
                    out.setdefault((W, s), []).append((fired, p if fired else 1 - p))
    return out


def assert_offsets_covered(tests, sizes, least=5):
    """Every offset of every window size sees at least `least` fires and `least` non-fires, and a
    wrong word at that offset passes all its tests with a chance below 1e-9."""
    for W in sizes:
        for s in range(W):
            ev = tests.get((W, s), [])
            fires, chance = sum(f for f, _ in ev), float(np.prod([p for _, p in ev]))
            assert fires >= least and len(ev) - fires >= least, f"W={W} offset {s}: {fires} fires of {len(ev)} tests"
            assert chance < 1e-9, f"W={W} offset {s}: a wrong word passes with chance {chance:.2e}"


# ----------------------------------------------------------------- the background and the carriers
def sea_run(n, rows, world=POOLW):
    """Every env a ship at (row, y) that moves S to (row, y + 1) and N back, with a destination and
    no cargo."""
    st = empty_state(n)
    acts = np.zeros((rows, n), np.int32)
    for i in range(n):
        st["x"][i], st["y"][i] = SEA_ROWS[i % 2], (i // 2) % (world.W - 1)
        st["origin"][i], st["dest"][i] = i % world.P, (i + 1) % world.P
        st["fuel"][i] = 100.0 + 0.125 * i
        acts[:, i] = [S_ if k % 2 == 0 else N_ for k in range(rows)]
    return st, acts


# the carrier lanes of a wave by their number: lane 0 and lane 63, both 32-lane halves
CARRIER_LANES = {
    0: [], 1: [63], 2: [1, 40], 5: [1, 2, 34, 35, 62], 8: [0, 63, 5, 17, 30, 33, 47, 58],
    9: [0, 31, 32, 63, 7, 20, 40, 50, 60], 16: list(range(0, 64, 4)), 17: list(range(0, 64, 4)) + [63], 64: list(range(64)),
}


def put_carriers(st, wave, count, cargo=49, whole_lane=False):
    """Lane L's cargo goes to env slot L % 4 (lane 0: slot 0, lane 63: slot 3); lane 5 of the
    8-lane set carries in two slots. whole_lane: in all four, so the lane stays a carrier."""
    for lane in CARRIER_LANES[count]:
        st["cargo"][wave * WAVE + 4 * lane + lane % 4] = cargo
        if whole_lane:
            st["cargo"][wave * WAVE + 4 * lane:wave * WAVE + 4 * lane + 4] = cargo
    if count == 8:
        st["cargo"][wave * WAVE + 4 * 5 + 2] = cargo


def carrier_lanes(cargo, wave):
    return int((cargo[wave * WAVE:(wave + 1) * WAVE].reshape(LANES, 4) > 0).any(1).sum())


# ----------------------------------------------------------------- slots and offsets
# waves i and i + 4 are successive groups of one hardware wave under SHIPENV_STEP_BLOCKS=1
COUNTS = (8, 1, 0, 9, 16, 17, 64, 5)
N_COUNTS = len(COUNTS) * WAVE + 3
K_COUNTS = 40
KS = (2, 9, 10, 17, K_COUNTS)
# (seed, env_id_base, first counter): plain; quad ids with e1 0 and 1 in wave 0 (its lanes below
# and from 32) and the first window of 8 at t = 2^32 - 3 .. 2^32 + 4
IDS = {"plain": (SEED, 0, 0), "wrap": (SEED, (1 << 34) - 128, (1 << 32) - 3)}


def counts_run():
    st, acts = sea_run(N_COUNTS, K_COUNTS + TAIL)
    for w, c in enumerate(COUNTS):
        put_carriers(st, w, c, whole_lane=c == 5)  # 5 lanes, 20 envs: more tests at every offset of W = 8
    st["cargo"][N_COUNTS - 2] = 49  # the tail kernel's
    return st, acts


def assert_counts_scenario(O, init, acts, trace, ids):
    seed, base, t0 = IDS[ids]
    assert [carrier_lanes(init["cargo"], w) for w in range(len(COUNTS))] == list(COUNTS)
    rec = windows(POOLW, init, acts, trace, launches_of(K_COUNTS))
    first = rec[0]
    assert [first[w][0] for w in range(8)] == ["pool", "pool", "none", "pool", "pool", "direct", "direct", "pool"]
    assert [first[w][1] for w in (0, 1, 3, 4, 7)] == [8, 8, 4, 4, 8]
    # no take anywhere: a window ends only at its size, so offsets run 0 .. W - 1 from the launch's start
    assert all(r[0][2] == k % 8 for k, r in rec.items() if r[0][0] == "pool" and r[0][1] == 8)
    # the wave of 9 comes down to a window of 8 and the wave of 17 from the direct draw to the pool
    # inside the launch, as carriers lose their whole cargo
    assert {rec[k][3][1] for k in rec if rec[k][3][0] == "pool"} == {4, 8}
    assert {rec[k][5][0] for k in rec} == {"direct", "pool"}
    assert all(rec[k][2][0] == "none" for k in rec)
    tests = gate_tests(O, POOLW, init, acts, trace, launches_of(K_COUNTS), seed, base, t0)
    # 39 inner steps: every offset of W = 8 sees 97 to 175 gate tests with 7 to 43 fires, every offset of W = 4
    # 103 to 170 with 10 to 41 (printed by -s). A wrong word at one offset passes each test with the chance of
    # the test's own outcome; over an offset's tests that product is below 1e-9 (asserted)
    print({ws: (sum(f for f, _ in ev), len(ev)) for ws, ev in sorted(tests.items())})
    assert_offsets_covered(tests, (8, 4))
    if ids == "wrap":
        quads = (base + np.arange(WAVE)) >> 2
        assert set(quads >> 32) == {0, 1} and (quads[4 * 31] >> 32, quads[4 * 32] >> 32) == (0, 1)
        assert (t0 + 7) >> 32 == 1 and t0 >> 32 == 0 and first[0][:2] == ("pool", 8)


@pytest.mark.parametrize("ids", list(IDS))
def test_counts_scenario_on_the_oracle(ids, oracle_mod):
    seed, base, t0 = IDS[ids]
    init, acts = counts_run()
    assert_counts_scenario(oracle_mod, init, acts, oracle_trace(oracle_mod, POOLW, init, acts, seed, base, t0), ids)


_REF = {}


def reference(name, make, world=POOLW, ids="plain"):
    """The twin's recorded steps of a run (read-only, shared by the cases)."""
    if (name, ids) not in _REF:
        seed, base, t0 = IDS[ids]
        init, acts = make()
        _REF[name, ids] = (init, acts, twin_trace(world, init, acts, seed, base, t0))
    return _REF[name, ids]


def assert_twin_is_oracle(O, world, init, acts, trace, ids, what):
    seed, base, t0 = IDS[ids]
    for k, want in enumerate(oracle_trace(O, world, init, acts, seed, base, t0)):
        assert_same(trace[k], want, f"{what}: twin vs oracle, step {k}")


SETTINGS = [{}, {"SHIPENV_NT_LOADS": "1"}, {"SHIPENV_NT_LOADS": "0"}, {"SHIPENV_SEQ_MAX_STEPS": "7"}, {"SHIPENV_STEP_BLOCKS": "1"},
            {"SHIPENV_SEQ_GATE_POOL": "0"}]
ids_of = lambda e: "-".join(f"{k[8:]}{v}" for k, v in e.items()) or "plain"  # noqa: E731


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
def test_carrier_counts_fused_equals_step_calls(ids, env, gpu_lib, oracle_mod):
    """Waves of 8, 1, 0, 9, 16, 17, 64 and 5 carrier lanes; runs of 2, 9, 10, 17 and 40 steps, and
    17 split at step 5: whole, with both kinds of load, cut into launches of at most 7 steps, with
    one workgroup (each hardware wave steps two groups with different counts) and with the direct
    draw."""
    seed, base, t0 = IDS[ids]
    init, acts, trace = reference("counts", counts_run, ids=ids)
    assert_counts_scenario(oracle_mod, init, acts, trace, ids)
    if not env:
        assert_twin_is_oracle(oracle_mod, POOLW, init, acts, trace, ids, f"counts {ids}")
    b = POOLW.env(N_COUNTS, seed=seed, env_id_base=base, **env)
    dev = device_rows(b, acts)
    for K in KS:
        run_fused(b, init, dev, trace, K, None, f"counts {ids} {env}", t0)
    run_fused(b, init, dev, trace, 17, 5, f"counts {ids} {env}", t0)
    b.close()


# ----------------------------------------------------------------- invalidation
K_TAKE = 24
TAKE = 25  # the amount taken: the gate then fires on half the words, so a stale word shows on half the tests
# (wave, its carrier lanes before the take, the actor's env in the wave, the inner step of its take)
ACTORS = ((0, 5, 4 * 10 + 0, 3),    # a window of 8 running: the take at offset 3
          (1, 16, 4 * 2 + 1, 1),    # 16 -> 17 carrier lanes: from the pool (a window of 4) to the direct draw
          (2, 0, 4 * 63 + 3, 5),    # no carrier: the first one appears inside the run
          (3, 5, 4 * 3 + 2, 11),    # a window of 8, the second of the launch: the take at offset 3
          (4, 5, 4 * 20 + 1, 1))    # takes at steps 1 and 2: two windows in a row cut early, then the direct draw
N_TAKE = 5 * WAVE + 3
TAKE_SEED = 22  # the first seed from 22 on with which assert_take_scenario holds on the oracle


def take_run():
    """The actors stand on port 0's cell with no cargo, select until their take, take TAKE cargo,
    then move between the two water cells below the port."""
    st, acts = sea_run(N_TAKE, K_TAKE + TAIL)
    for w, count, at, k0 in ACTORS:
        put_carriers(st, w, count, whole_lane=count == 16)  # 16 lanes that are still 16 at the take
        i = w * WAVE + at
        assert st["cargo"][i // 4 * 4:i // 4 * 4 + 4].sum() == 0, "the actor's lane carries nothing before the take"
        st["x"][i], st["y"][i] = POOLW.ports[0]
        st["origin"][i], st["dest"][i], st["cargo"][i] = 1, 2, 0
        acts[:, i] = [(E_ if (k - k0) % 2 else W_) for k in range(K_TAKE + TAIL)]
        acts[:k0, i] = [4 + 3 if k % 2 == 0 else 4 + 2 for k in range(k0)]
        acts[k0, i] = POOLW.cargo(TAKE)
        if w == 4:  # one more unit of cargo at the next step: the second window lasts one step
            k0 += 1
            acts[k0, i] = POOLW.cargo(1)
        acts[k0 + 1, i] = W_  # off the port: (3, 2), then (4, 2) and back
        acts[k0 + 2, i] = W_
    return st, acts


def assert_take_scenario(O, init, acts, trace, seed=TAKE_SEED):
    rec = windows(POOLW, init, acts, trace, launches_of(K_TAKE))
    prev = [init] + list(trace)
    for w, count, at, k0 in ACTORS:
        i = w * WAVE + at
        assert k0 % 8 != 0 and k0 % 4 != 0 and k0 + 1 < K_TAKE - 1
        assert carrier_lanes(prev[k0]["cargo"], w) <= count and prev[k0]["cargo"][i] == 0
        assert trace[k0]["cargo"][i] == TAKE and trace[k0]["err"][i] == OK, f"wave {w}: the take passes"
        # the take ends the window: the wave votes again at the next step, offset 0, one lane more
        mode, W, s, m = rec[k0 + 1][w]
        assert s == 0 and m == carrier_lanes(prev[k0]["cargo"], w) + 1, (w, rec[k0 + 1][w])
        # and the actor's gate fires, with a loss, before the window it was taken in would have ended
        mode0, W0, s0, _ = rec[k0][w]
        end = k0 - s0 + W0 if mode0 == "pool" and w != 4 else K_TAKE - 1
        lost = [k for k in range(k0 + 1, end) if trace[k]["cargo"][i] < prev[k]["cargo"][i]]
        assert lost, f"wave {w}: no cargo lost in steps {k0 + 1} .. {end - 1}"
        assert gate_word(O, i, lost[0], seed) <= gate_thr(prev[lost[0]]["cargo"][i])
    k0 = ACTORS[1][3]
    assert rec[k0][1][:2] == ("pool", 4) and rec[k0 + 1][1] == ("direct", 0, 0, 17), "16 -> 17: the wave changes path"
    assert rec[k0 + 1 + DIRECT_RUN][1][0] in ("direct", "pool") and k0 + 1 + DIRECT_RUN < K_TAKE - 1
    assert rec[ACTORS[2][3]][2][0] == "none" and rec[ACTORS[2][3] + 1][2][:2] == ("pool", 8)
    assert rec[3][0][:3] == ("pool", 8, 3) and rec[4][0][:3] == ("pool", 8, 0)
    assert rec[11][3][:3] == ("pool", 8, 3) and rec[12][3][:3] == ("pool", 8, 0)
    # wave 4: windows of 2 steps and of 1 step, each ended by a take; the direct draw for 16 steps with at most 16
    # carrier lanes; then the pool again
    assert [rec[k][4][:3] for k in (0, 1, 2)] == [("pool", 8, 0), ("pool", 8, 1), ("pool", 8, 0)]
    assert all(rec[k][4][0] == "direct" and 0 < rec[k][4][3] <= LIMIT for k in range(3, 3 + DIRECT_RUN))
    assert rec[3 + DIRECT_RUN][4][:3] == ("pool", 8, 0)
    i4 = 4 * WAVE + ACTORS[4][2]
    assert trace[2]["cargo"][i4] == TAKE + 1 and trace[2]["err"][i4] == OK


def test_take_scenario_on_the_oracle(oracle_mod):
    init, acts = take_run()
    assert_take_scenario(oracle_mod, init, acts, oracle_trace(oracle_mod, POOLW, init, acts, TAKE_SEED))


@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_NT_LOADS": "0"}, {"SHIPENV_NT_LOADS": "1"}, {"SHIPENV_SEQ_GATE_POOL": "0"}], ids=ids_of)
def test_a_take_ends_the_window(env, gpu_lib, oracle_mod):
    """A new carrier inside a window of 8, a wave that goes from 16 to 17 carrier lanes, and a wave
    whose first carrier appears mid-run: each take is followed by a fired gate with a loss before
    the old window's end."""
    if "take" not in _REF:
        init, acts = take_run()
        _REF["take"] = (init, acts, twin_trace(POOLW, init, acts, TAKE_SEED))
    init, acts, trace = _REF["take"]
    assert_take_scenario(oracle_mod, init, acts, trace)
    if not env:
        for k, want in enumerate(oracle_trace(oracle_mod, POOLW, init, acts, TAKE_SEED)):
            assert_same(trace[k], want, f"take: twin vs oracle, step {k}")
    b = POOLW.env(N_TAKE, seed=TAKE_SEED, **env)
    dev = device_rows(b, acts)
    for K in (K_TAKE, 10):
        run_fused(b, init, dev, trace, K, None, f"take {env}")
    b.close()


# ----------------------------------------------------------------- a partial last wave
N_PART = 4 * (64 + 5) + 3  # a whole wave, a wave of 5 lanes, a tail of 3 envs
K_PART = 17


def part_run():
    st, acts = sea_run(N_PART, K_PART + TAIL)
    put_carriers(st, 0, 8)
    for i in (WAVE + 0, WAVE + 4 * 4 + 3, N_PART - 3, N_PART - 1):  # lanes 0 and 4 of the partial wave, the tail
        st["cargo"][i] = 49
    return st, acts


def assert_part_scenario(O, init, acts, trace):
    rec = windows(POOLW, init, acts, trace, launches_of(K_PART))
    assert all(r[0][:2] == ("pool", 8) and r[1][0] == "direct" for r in rec.values())
    prev = [init] + list(trace)
    # cargo is lost in the whole wave, the partial wave and the tail inside the run
    for sl in (slice(0, WAVE), slice(WAVE, N_PART & ~3), slice(N_PART & ~3, N_PART)):
        assert any((trace[k]["cargo"][sl] < prev[k]["cargo"][sl]).any() for k in range(K_PART - 1)), sl
    gate_tests(O, POOLW, init, acts, trace, launches_of(K_PART))


def test_partial_wave_scenario_on_the_oracle(oracle_mod):
    init, acts = part_run()
    assert_part_scenario(oracle_mod, init, acts, oracle_trace(oracle_mod, POOLW, init, acts))


@gpu
@pytest.mark.parametrize("env", [{}, {"SHIPENV_NT_LOADS": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}], ids=ids_of)
def test_partial_last_wave_draws_directly(env, gpu_lib, oracle_mod):
    """n = 4 (64 + 5) + 3: the wave with inactive lanes refills nothing and matches, beside a whole
    wave that pools and the tail kernel's envs."""
    init, acts, trace = reference("part", part_run)
    assert_part_scenario(oracle_mod, init, acts, trace)
    if not env:
        assert_twin_is_oracle(oracle_mod, POOLW, init, acts, trace, "plain", "partial wave")
    b = POOLW.env(N_PART, **env)
    dev = device_rows(b, acts)
    for K in (2, 10, K_PART):
        run_fused(b, init, dev, trace, K, None, f"partial wave {env}")
    b.close()


# ----------------------------------------------------------------- the dense random run
@gpu
@pytest.mark.parametrize("nt", ["1", "0"])
def test_pool_and_direct_draw_equal_the_step_calls(nt, gpu_lib):
    """test_gpu_step_seq_trim's random run (ships on ports in every wave, cargo 0 .. 59, takes
    and arrivals throughout: most waves are above the limit, windows end early): the default and
    SHIPENV_SEQ_GATE_POOL=0 both end where the step calls do."""
    init, acts, trace = generic_reference("plain")
    from test_gpu_step_seq_trim import GENERIC, N_GENERIC

    for pool in (None, "0", "1"):
        b = GENERIC.env(N_GENERIC, SHIPENV_NT_LOADS=nt, SHIPENV_SEQ_GATE_POOL=pool)
        dev = device_rows(b, acts)
        for K in (2, 33):
            run_fused(b, init, dev, trace, K, None, f"dense nt={nt} pool={pool}")
        b.close()


# ----------------------------------------------------------------- no room for the pool
class Wide(World):
    """240 x 245 cells: the image takes 60 KiB of LDS, which leaves room for the fused kernel's
    stock table (2 KiB) under the 64 KiB of a launch and none for the pools (6 KiB)."""

    H, W = 240, 245


WIDE = Wide(ports=[(2, 2), (2, 5), (200, 240), (239, 9)], fuel=[7, 0, 4, 5], cargo=[49, 0, 9, 6], ground=[(2, 1), (4, 6)])
N_WIDE, K_WIDE = 2 * WAVE + 3, 12


def image_bytes(world):
    """WorldDims::padded() * 4 (world.h): the cell codes in whole 16-byte units, the port
    positions, the stocks from an even word, the 51 gate words, from an even word the 100 + 20 words
    of the f64 tables, and the 4 moves; in whole 1024-word rows."""
    cw = (world.H * world.W + 15) // 16 * 4
    stk = (cw + world.P + 1) & ~1
    frac = (stk + 2 * world.P + 51 + 1) & ~1
    total = frac + 100 + 20 + 4
    return max((total + 1023) // 1024 * 1024, 3072) * 4


def wide_run():
    st, acts = sea_run(N_WIDE, K_WIDE + TAIL, WIDE)
    put_carriers(st, 0, 8)
    put_carriers(st, 1, 16)
    return st, acts


def test_wide_world_has_room_for_the_stock_table_only(oracle_mod):
    stock_table, pools = 256 * 8, 4 * (64 + 32) * 16
    assert image_bytes(POOLW) + stock_table + pools <= 64 * 1024
    assert image_bytes(WIDE) + stock_table <= 64 * 1024 < image_bytes(WIDE) + stock_table + pools
    code = cell_codes(WIDE)
    assert all((code[r, :13] == 0).all() for r in SEA_ROWS)
    init, acts = wide_run()
    trace = oracle_trace(oracle_mod, WIDE, init, acts)
    prev = [init] + trace
    assert any((trace[k]["cargo"] < prev[k]["cargo"]).any() for k in range(K_WIDE - 1))


@gpu
def test_wide_world_stays_fused_and_correct(gpu_lib, oracle_mod):
    """The launch has no room for the pools: the fused kernel draws directly. The run equals the
    step calls whole, cut into launches of at most 5 steps (only a fused run is cut: each launch
    ends in a full step) and with the settings that choose the direct draw and a launch per step.
    Which kernel ran is not visible from outside; launch_step_seq's rule is the one
    test_wide_world_has_room_for_the_stock_table_only states."""
    init, acts = wide_run()
    trace = twin_trace(WIDE, init, acts)
    for k, want in enumerate(oracle_trace(oracle_mod, WIDE, init, acts)):
        assert_same(trace[k], want, f"wide: twin vs oracle, step {k}")
    for env in ({}, {"SHIPENV_SEQ_MAX_STEPS": "5"}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_FUSE": "0"}):
        b = WIDE.env(N_WIDE, **env)
        run_fused(b, init, device_rows(b, acts), trace, K_WIDE, None, f"wide {env}")
        b.close()
