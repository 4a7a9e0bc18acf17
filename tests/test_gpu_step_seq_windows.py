"""The GATE pool of a fused se_step_seq sizes its windows to the carriers and ends them only where
cargo rose, and a regular wave tests an arrival by the cell code where it may (step_seq.h, "The
wave's GATE pool" and step_group_ring; step_lean.h, gate_window_entry and arrive_by_code).
  * A wave of m <= 16 carrier lanes draws W = min(16, 64 / m) steps ahead, lane L = s m + c drawing
    carrier c's block for offset s, and reads entry s m + rank; the refill's ballot, shifted by m
    per step, is the screen.
  * A window ends after a step in which some env's cargo rose (a passed take of cargo). A take of
    fuel and a refused take leave it standing.
  * In a launch whose ports lie on distinct cells, a regular wave all of whose envs have dest < P
    tests an arrival as do_move & (code == dest + 1); every other wave compares positions.

What can go wrong: the reciprocal multiply or the window length at some m, an entry read at the
wrong rank or offset (W = 16, 12, 9, 8, 7 and 4 all read differently), a screen bit taken from the
neighbouring offset's m bits or past bit 31, a hot step past offset 7 taken for cold, a window kept
after cargo rose (a new carrier has no entry and no screen bit: its gate never fires), a window
ended or a pool entry lost where only fuel was taken, a stale threshold after an arrival, an arrival
seen at another port's cell or for a ship that did not try to move or moved off the map, a wave
with a loaded dest >= P or a world with a shared cell taken for the test by code. A missed fire
shows as cargo that is not lost, a missed arrival as an origin that does not change.

The method is step_seq_support's: a twin env stepped by plain steps, the C oracle's trace, and one
step_seq call of 2, 17 and 40 steps (39 inner steps: two 16-step windows and a run that ends inside
the third), all equal bit for bit in state, reward, done and err, with 2 plain steps after, under
{}, SHIPENV_SEQ_SCREEN=0, SHIPENV_SEQ_GATE_POOL=0, SHIPENV_SEQ_RING=0 and SHIPENV_STEP_BLOCKS=1,
from counter 0 and with the counter wrapping 2^32 inside the first window.

The first run is on a hand-built 7 x 9 map like test_gpu_step_seq_ring's with its five ports on
distinct cells: whole waves of 0, 1, 3, 4, 5, 7, 8, 9, 16 and 17 carrier lanes at sea (W = 16, 16,
16, 12, 9, 8, 7, 4 and the direct run; the carriers hold 55, 1, 30, 55, 1 by rank as in
test_gpu_step_seq_screen, the one carrier lane of its wave 49 four times, so that gates fire at
offsets 8 .. 15), three waves of scripted ships, a wave of 20 lanes and a tail of 3 envs.
  wave TAKES (cargo takes in mid-window, each ending its window): a carrier of 30 arrives at port 2
    at step 1 (cargo 0 in mid-window) and takes 20 there at step 3 (a take by a lane that lost its
    cargo); a carrier of 5 takes 20 more at step 5; six ships in lanes without cargo take 25 at
    step 10. Each then leaves the port and its gate fires before the cut window would have ended.
  wave KEPT (nothing ends its 16-step windows): a carrier of 55 takes fuel at step 3 and moves from
    step 4 on, so its gate fires, for certain, later in the same window; another is refused a take
    at step 5 and moves from step 6 on; a carrier of 30 selects port 4 at step 0 and arrives there
    at step 5 (an arrival that zeroes a carrier in mid-window, at a destination selected earlier).
  wave ARRIVALS (the test by code): an arrival; a ship that crosses another port's cell and does
    not arrive; a mover blocked by ground while standing on its destination, which arrives; an
    arrival at a port selected at step 0; a take right after an arrival.
The second run is test_gpu_step_seq_ring's hand-built run, whose world has two ports on one cell
(no launch there tests by code). The third is test_gpu_step_seq_screen's bad_dest_run: a ship
loaded with dest >= P as its wave's only such env, in a world with distinct ports; the C oracle
indexes its port table with the destination, so that run is compared with the twin alone. The
fourth is a world of one port: an arrival there writes pick_other's 1 = P as the new dest, which the
position compare clamps to port 0, so a ship blocked by ground on the port arrives on every step
and a ship that leaves and comes back arrives again; such a launch must never test by code (a
code never equals dest + 1 = 2). It too is compared with the twin alone.

The CPU companion asserts on the oracle that each scripted case happens, with a model of the new
windows (`windows`) and the drawn words themselves, and fails if a count is 0: hot steps past
offset 7 and fires there, takes of fuel and refused takes inside a window that stays, the three
kinds of cargo take in mid-window, and arrivals by each route. The counts it prints (-s), from
counter 0 and with the wrap: hot steps past offset 7: 51 and 50, fires there: 22 and 18, kept
takes: 2 and 2, arrivals in the waves that test by code (here every whole wave): 18 and 18.

Mutation checks, run once while this was built (not part of the suite): a library that never ends a
window on a take of cargo, and one whose test by code ignores do_move, both fail the default cases
of the first run."""
import numpy as np
import pytest

from step_seq_support import AMOUNT, OK, TAIL, assert_same, device_rows, empty_state, gpu_lib, oracle_trace, run_fused, twin_trace  # noqa: F401
from test_gpu_step_seq_gatepool import IDS, LANES, LIMIT, DIRECT_RUN, EARLY_CUT, POOLW, WAVE, gate_thr, gate_word, launches_of
from test_gpu_step_seq_guards import cell_codes
from test_gpu_step_seq_ring import HAND, Hand, assert_claims
from test_gpu_step_seq_ring import N as N_HAND
from test_gpu_step_seq_ring import hand_run
from test_gpu_step_seq_screen import BAD_DEST, BAD_ENV, N_BAD, bad_dest_run
from test_gpu_step_seq_trim import E_, N_, S_, W_

gpu = pytest.mark.gpu

KS = (2, 17, 40)
K = max(KS)
SETTINGS = [{}, {"SHIPENV_SEQ_SCREEN": "0"}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_RING": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}]

# ports 0 on a corner, 1 and 4 on edges, 2 in the interior with ground north of it, 3 beside the west edge: all on distinct cells
WIN = Hand(ports=[(0, 0), (0, 5), (3, 4), (5, 2), (3, 8)], fuel=[7, 5, 9, 4, 6], cargo=[3, 6, 49, 2, 5], ground=[(3, 3), (1, 7), (5, 6)])
SEA_ROWS = (2, 6)  # neither a port nor ground in these rows
COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 16, 17)
W_OF = {0: 16, 1: 16, 3: 16, 4: 16, 5: 12, 7: 9, 8: 8, 9: 7, 16: 4}
CARRIER_LANES = {0: [], 1: [63], 3: [0, 33, 63], 4: [0, 31, 32, 63], 5: [1, 2, 34, 35, 62], 7: [0, 9, 18, 27, 36, 45, 63],
                 8: [0, 63, 5, 17, 30, 33, 47, 58], 9: [0, 31, 32, 63, 7, 20, 40, 50, 60], 16: list(range(0, 64, 4)),
                 17: list(range(0, 64, 4)) + [63]}
MIX = (55, 1, 30, 55, 1)  # the carriers' cargo, by their rank in the wave
TAKES_WAVE, KEPT_WAVE, ARRIVALS_WAVE = len(COUNTS), len(COUNTS) + 1, len(COUNTS) + 2
WAVES = len(COUNTS) + 3
PART_LANES = 20
N = WAVES * WAVE + 4 * PART_LANES + 3
PORT2, PORT3, PORT4 = (3, 4), (5, 2), (3, 8)
# (lane, env slot) of the scripted ships of the waves TAKES and KEPT
ARRIVER, CARRIER_TAKER, NEW_TAKER = (10, 0), (20, 1), (30, 2)
CARGO_TAKES = {ARRIVER: (3, 20), CARRIER_TAKER: (5, 20), NEW_TAKER: (10, 25)}
# five more like NEW_TAKER, at the same step: a window kept over that take gives each of them another lane's words
MORE_TAKERS = ((34, 0), (38, 1), (42, 3), (46, 2), (50, 0))
FUEL_TAKER, REFUSED, MID_ARRIVER = (5, 1), (12, 2), (40, 3)
FUEL_AT, REFUSED_AT, MID_ARRIVE_AT = 3, 5, 5


# one port, in the interior with ground north of it
ONE_PORT = Hand(ports=[PORT2], fuel=[9], cargo=[49], ground=[(3, 3), (1, 7), (5, 6)])
N_ONE = 2 * WAVE + 3
ONE_BLOCKED, ONE_RETURNS = [4 * lane + lane % 4 for lane in (0, 21, 63)], [WAVE + 4 * lane + lane % 4 for lane in (3, 40)]


def one_port_run():
    """Two whole waves at sea and a tail, every ship with origin 0 and dest 0 (dest < P everywhere). In
    wave 0 three carriers stand on the port and move north into the ground on every step; in wave 1
    two ships go onto the port, off it and onto it again."""
    st, acts = sea_run(N_ONE, K + TAIL)
    st["origin"][:] = 0
    st["dest"][:] = 0
    for i in ONE_BLOCKED:
        place(st, acts, i, PORT2, 0, 0, 20, [], (N_,))
    for i in ONE_RETURNS:
        place(st, acts, i, (3, 5), 0, 0, 10, [], (N_, S_))
    return st, acts


def ids_of(env):
    return "-".join(f"{k[8:].lower()}{v}" for k, v in env.items()) or "plain"


def env_of(wave, actor):
    return wave * WAVE + 4 * actor[0] + actor[1]


def sea_run(n, rows):
    """Every env a ship at (row, y) that moves S to (row, y + 1) and N back, with a destination and no cargo."""
    st = empty_state(n)
    acts = np.zeros((rows, n), np.int32)
    for i in range(n):
        st["x"][i], st["y"][i] = SEA_ROWS[i % 2], (i // 2) % (WIN.W - 1)
        st["origin"][i], st["dest"][i] = i % WIN.P, (i + 1) % WIN.P
        st["fuel"][i] = 100.0 + 0.125 * (i % 512)
        acts[:, i] = [S_ if k % 2 == 0 else N_ for k in range(rows)]
    return st, acts


def place(st, acts, i, cell, origin, dest, cargo, rows_first, then):
    """Ship i at `cell`; its first action rows, then `then` repeated (a pair: alternating)."""
    st["x"][i], st["y"][i] = cell
    st["origin"][i], st["dest"][i], st["cargo"][i] = origin, dest, cargo
    rows = len(acts)
    acts[:, i] = [then[(k - len(rows_first)) % len(then)] for k in range(rows)]
    acts[:len(rows_first), i] = rows_first


def arrival_scripts():
    """[(label, ship (cell, origin, dest, cargo), first rows, claims)] of the wave ARRIVALS; after the
    first rows the ship selects (it stays). Copy j of script s is env j of lane 4 s + j."""
    tc = WIN.cargo
    return [
        ("arrival", ((0, 4), 0, 1, 10), [S_], [(0, "pos", (0, 5)), (0, "origin", 1), (0, "cargo", 0), (0, "err", OK)]),
        # over port 1's cell on the way to port 4: no arrival there (cargo 0: no gate either)
        ("crossing", ((0, 4), 0, 4, 0), [S_, S_], [(0, "pos", (0, 5)), (0, "origin", 0), (0, "dest", 4), (1, "pos", (0, 6)), (1, "origin", 0)]),
        # blocked by the ground north of port 2 while standing on it, its destination: an arrival
        ("blocked_on_dest", (PORT2, 0, 2, 20), [4 + 2, N_], [(0, "cargo", 20), (1, "err", OK), (1, "pos", PORT2), (1, "origin", 2), (1, "cargo", 0)]),
        # a select at step 0, four steps of staying, then onto the selected port
        ("selected_earlier", ((5, 3), 0, 1, 0), [4 + 3, 4 + 3, 4 + 3, 4 + 3, N_],
         [(0, "dest", 3), (3, "origin", 0), (3, "pos", (5, 3)), (4, "pos", PORT3), (4, "origin", 3), (4, "err", OK)]),
        ("arrive_then_take", ((3, 5), 0, 2, 10), [4 + 2, 4 + 2, N_, tc(9)],
         [(2, "pos", PORT2), (2, "origin", 2), (2, "cargo", 0), (3, "err", OK), (3, "cargo", 9)]),
        # a ship that stands on its destination and does not try to move: no arrival
        ("stays_on_dest", (PORT2, 0, 2, 20), [4 + 2, 4 + 2, 4 + 2], [(2, "origin", 0), (2, "cargo", 20), (2, "pos", PORT2)]),
    ]


def script_envs(s):
    return [ARRIVALS_WAVE * WAVE + 4 * (4 * s + j) + j for j in range(4)]


def windows_run():
    rows = K + TAIL
    st, acts = sea_run(N, rows)
    for w, count in enumerate(COUNTS):
        for r, lane in enumerate(CARRIER_LANES[count]):
            i = w * WAVE + 4 * lane
            if count == 1:  # the one carrier lane holds four carriers: fires at every offset of its 16-step windows
                st["cargo"][i:i + 4] = 49
            else:
                st["cargo"][i + lane % 4] = MIX[r % len(MIX)]
                if r % len(MIX) == 2:  # the carrier of 30 moves on every other step only: hot steps without a fire
                    acts[:, i + lane % 4] = [(S_, 4 + 0, N_, 4 + 0)[k % 4] for k in range(rows)]
    for lane in (0, 7, 19):  # the wave of 20 lanes (it draws directly) and the tail
        st["cargo"][WAVES * WAVE + 4 * lane + lane % 4] = 55
    st["cargo"][N - 2] = 55
    # ---- the wave TAKES: two carrier lanes of light ships at sea, and the three ships that take cargo at port 2
    for lane in (1, 62):
        st["cargo"][TAKES_WAVE * WAVE + 4 * lane + lane % 4] = 1
    for actor, (k0, amount) in list(CARGO_TAKES.items()) + [(x, CARGO_TAKES[NEW_TAKER]) for x in MORE_TAKERS]:
        i = env_of(TAKES_WAVE, actor)
        # selects until the take, then off the port and back: (4, 4), (3, 4)
        place(st, acts, i, PORT2, 1, 0, 0, [4 + 3 if k % 2 == 0 else 4 + 4 for k in range(k0)] + [WIN.cargo(amount)], (W_, E_))
    a = env_of(TAKES_WAVE, ARRIVER)  # two cells south of port 2, bound for it
    st["x"][a], st["y"][a] = PORT2[0], PORT2[1] + 2
    st["origin"][a], st["dest"][a], st["cargo"][a] = 1, 2, 30
    acts[:3, a] = [N_, N_, 4 + 1]  # the select of the port it left: passes or not, the ship stays
    st["cargo"][env_of(TAKES_WAVE, CARRIER_TAKER)] = 5
    # ---- the wave KEPT: one carrier lane of a light ship at sea, and three carriers whose windows nothing ends
    st["cargo"][KEPT_WAVE * WAVE + 4 * 63 + 3] = 1
    place(st, acts, env_of(KEPT_WAVE, FUEL_TAKER), PORT2, 1, 0, 55, [4 + 3, 4 + 4, 4 + 3, WIN.fuel(3)], (W_, E_))
    place(st, acts, env_of(KEPT_WAVE, REFUSED), PORT3, 1, 0, 55, [4 + 2, 4 + 4, 4 + 2, 4 + 4, 4 + 2, WIN.cargo(3)], (W_, E_))
    place(st, acts, env_of(KEPT_WAVE, MID_ARRIVER), (3, 7), 1, 0, 30, [4 + 4] * MID_ARRIVE_AT + [S_], (4 + 0, 4 + 2))
    # ---- the wave ARRIVALS
    for s, (_, (cell, origin, dest, cargo), first, _) in enumerate(arrival_scripts()):
        for i in script_envs(s):
            place(st, acts, i, cell, origin, dest, cargo, first, (4 + 2, 4 + 3))
            st["fuel"][i] = 100.0 + 0.125 * (i % 64)
    return st, acts


# ----------------------------------------------------------------- the model of the new windows
def windows(world, init, acts, trace, launches):
    """rec[k][wave] = (mode, W, offset, m) of every inner step k, as test_gpu_step_seq_gatepool's model,
    with W = min(16, 64 / m) and a window ended only by a step in which some env's cargo rose."""
    n = len(init["x"])
    full = n & ~3
    prev = [init] + list(trace)
    rec = {}
    for w in range((full + WAVE - 1) // WAVE):
        sl = slice(w * WAVE, min((w + 1) * WAVE, full))
        whole = sl.stop - sl.start == WAVE
        for a, b in launches:
            k, cuts = a, 0
            while k < b - 1:
                cargo = prev[k]["cargo"][sl]
                m = int((np.pad(cargo, (0, WAVE - len(cargo))).reshape(LANES, 4) > 0).any(1).sum())
                if not whole or m > LIMIT or (cuts >= 2 and m):
                    for _ in range(min(DIRECT_RUN, b - 1 - k)):
                        rec.setdefault(k, {})[w] = ("direct", 0, 0, m)
                        k += 1
                    cuts = min(cuts, 1)
                    continue
                W = min(16, 64 // m) if m else 16
                rose = False
                for s in range(min(W, b - 1 - k) if m else b - 1 - k):
                    rec.setdefault(k, {})[w] = ("pool" if m else "none", W, s, m)
                    rose = bool((trace[k]["cargo"][sl] > prev[k]["cargo"][sl]).any())
                    k += 1
                    if rose:
                        break
                cuts = cuts + 1 if rose and m and s + 1 <= EARLY_CUT else 0
    return rec


def window_counts(O, init, acts, trace, ids):
    """Over the pooled windows of the run of K steps, from the model and the drawn words themselves:
    the window lengths seen, the hot steps past offset 7, the fires there, and the take blocks that
    leave their window standing. Asserts that cargo never rises inside a window and that every fire
    falls on a hot step."""
    seed, base, t0 = IDS[ids]
    code = cell_codes(WIN)
    rec = windows(WIN, init, acts, trace, launches_of(K))
    prev = [init] + list(trace)
    out = {"lengths": set(), "direct": 0, "hot_past_7": 0, "fires_past_7": 0, "kept_takes": 0}
    for k, by_wave in sorted(rec.items()):
        for w, (mode, W, s, m) in by_wave.items():
            if mode == "direct":
                out["direct"] += 1
                continue
            sl = slice(w * WAVE, (w + 1) * WAVE)
            took = bool(((acts[k][sl] >= 4 + WIN.P) & (code[prev[k]["x"][sl], prev[k]["y"][sl]] != 0)).any())
            nxt = rec.get(k + 1, {}).get(w)
            out["kept_takes"] += bool(took and m and nxt is not None and nxt[0] == "pool" and nxt[2] == s + 1)
            if not m:
                continue
            out["lengths"].add(W)
            vote = prev[k - s]["cargo"]
            hot, fires = False, 0
            for lane in range(LANES):
                i0 = w * WAVE + 4 * lane
                if not (vote[i0:i0 + 4] > 0).any():
                    assert (prev[k]["cargo"][i0:i0 + 4] <= 0).all(), f"step {k} lane {lane} of wave {w}: a carrier the vote did not see"
                    continue
                for i in range(i0, i0 + 4):
                    word = gate_word(O, i, t0 + k, seed, base)
                    hot |= word <= gate_thr(vote[i])
                    before = prev[k]["cargo"][i]
                    assert before <= vote[i], f"step {k} env {i}: cargo rose inside a window"
                    fires += bool(-4 <= acts[k][i] < 4 and trace[k]["err"][i] == OK and before > 0 and word <= gate_thr(before))
            assert hot or not fires, f"step {k} wave {w}: a gate fires on a cold step"
            out["hot_past_7"] += hot and s >= 8
            out["fires_past_7"] += fires if s >= 8 else 0
    return out


def assert_scenario(O, init, acts, trace, ids):
    carriers = lambda cargo, w: int((cargo[w * WAVE:(w + 1) * WAVE].reshape(LANES, 4) > 0).any(1).sum())  # noqa: E731
    assert N % 4 == 3 and [carriers(init["cargo"], w) for w in range(WAVES)] == list(COUNTS) + [4, 4, 16]
    assert len({tuple(p) for p in WIN.ports}) == WIN.P and (init["dest"][:N & ~3] < WIN.P).all()
    rec = windows(WIN, init, acts, trace, launches_of(K))
    # every wave starts with the window of its count; the wave of 17 draws directly
    assert [rec[0][w][:2] for w in range(len(COUNTS))] == [("none", 16)] + [("pool", W_OF[c]) for c in COUNTS[1:-1]] + [("direct", 0)]
    assert rec[0][WAVES][0] == "direct", "the wave of 20 lanes"
    t0 = IDS[ids][2]
    if ids == "wrap":
        assert t0 >> 32 == 0 and (t0 + 7) >> 32 == 1 and rec[7][1][:3] == ("pool", 16, 7)
    prev = [init] + list(trace)
    # ---- the wave TAKES: the three takes pass, each in mid-window, and each ends its window
    a, c, n = (env_of(TAKES_WAVE, x) for x in (ARRIVER, CARRIER_TAKER, NEW_TAKER))
    assert trace[0]["origin"][a] == 1 and trace[1]["origin"][a] == 2 and trace[1]["cargo"][a] == 0, "the carrier arrives at step 1"
    assert prev[1]["cargo"][a] > 0 and rec[1][TAKES_WAVE][:3] == ("pool", 16, 1) and rec[2][TAKES_WAVE][2] == 2, "in mid-window, which stays"
    assert trace[3]["cargo"][a] == 20 and trace[3]["err"][a] == OK, "the lane that lost its cargo takes"
    assert trace[4]["cargo"][c] == 5 and trace[5]["cargo"][c] == 25 and trace[5]["err"][c] == OK, "a carrier takes"
    assert init["cargo"][n // 4 * 4:n // 4 * 4 + 4].sum() == 0 and trace[10]["cargo"][n] == 25 and trace[10]["err"][n] == OK
    assert [rec[k][TAKES_WAVE][2] for k in (3, 4, 5, 6, 10, 11)] == [3, 0, 1, 0, 4, 0]
    assert all(rec[k][TAKES_WAVE][0] == "pool" for k in range(12))
    more = [env_of(TAKES_WAVE, x) for x in MORE_TAKERS]
    assert (init["cargo"][more] == 0).all() and (trace[10]["cargo"][more] == 25).all() and (trace[10]["err"][more] == OK).all()
    for i, (k0, _) in zip((a, c, n), CARGO_TAKES.values()):  # each taker's gate fires, with a loss, before the cut window would have ended
        end = k0 - rec[k0][TAKES_WAVE][2] + rec[k0][TAKES_WAVE][1]
        lost = [k for k in range(k0 + 1, min(end, K - 1)) if trace[k]["cargo"][i] < prev[k]["cargo"][i]]
        assert lost, f"env {i}: no cargo lost in steps {k0 + 1} .. {end - 1}"
    # ---- the wave KEPT: its first two windows run their 16 steps
    assert [rec[k][KEPT_WAVE][:3] for k in range(32)] == [("pool", 16, k % 16) for k in range(32)]
    f, r, m = (env_of(KEPT_WAVE, x) for x in (FUEL_TAKER, REFUSED, MID_ARRIVER))
    assert trace[FUEL_AT]["err"][f] == OK and trace[FUEL_AT]["fuel"][f] - prev[FUEL_AT]["fuel"][f] == 3.0 and trace[FUEL_AT]["cargo"][f] == 55
    assert trace[FUEL_AT + 1]["err"][f] == OK and trace[FUEL_AT + 1]["x"][f] == PORT2[0] + 1, "it moves right after: the gate fires for certain"
    assert gate_word(O, f, t0 + FUEL_AT + 1, *IDS[ids][:2]) <= gate_thr(55) and trace[15]["cargo"][f] < 55, "and cargo is lost in the same window"
    assert trace[REFUSED_AT]["err"][r] == AMOUNT and trace[REFUSED_AT]["cargo"][r] == 55 and trace[REFUSED_AT + 1]["x"][r] == PORT3[0] + 1
    assert trace[15]["cargo"][r] < 55, "the refused ship's gate fires later in the same window"
    assert trace[0]["dest"][m] == 4 and prev[MID_ARRIVE_AT]["cargo"][m] == 30 and trace[MID_ARRIVE_AT]["origin"][m] == 4
    assert trace[MID_ARRIVE_AT]["cargo"][m] == 0 and (trace[MID_ARRIVE_AT]["x"][m], trace[MID_ARRIVE_AT]["y"][m]) == PORT4
    # ---- the wave ARRIVALS
    scripts = arrival_scripts()
    assert 16 * len(scripts) <= WAVE
    for s, (label, _, _, claims) in enumerate(scripts):
        assert_claims(script_envs(s), claims, init, trace, label)
    # ---- the counts
    counts = window_counts(O, init, acts, trace, ids)
    arrivals = sum(int(((acts[k] >= -4) & (acts[k] < 4) & (trace[k]["err"] == OK) & (trace[k]["origin"] != prev[k]["origin"]))[:WAVES * WAVE].sum())
                   for k in range(K - 1))
    # every whole wave of this run takes the branch by code: distinct ports and dest < P everywhere (asserted above)
    print(ids, counts, "arrivals in the waves that test by code", arrivals)
    assert counts["lengths"] >= {16, 12, 9, 8, 7, 4} and counts["direct"] > 0
    assert counts["hot_past_7"] > 0 and counts["fires_past_7"] > 0 and counts["kept_takes"] >= 2 and arrivals >= 4 * 4 + 2


_REF = {}


def oracle_reference(O, ids):
    if ids not in _REF:
        seed, base, t0 = IDS[ids]
        init, acts = windows_run()
        trace = oracle_trace(O, WIN, init, acts, seed, base, t0)
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
        if name == "windows":
            world, (init, acts, want) = WIN, oracle_reference(O, ids)
        elif name == "hand":
            world = HAND
            init, acts = hand_run()
            want = oracle_trace(O, HAND, init, acts, seed, base, t0)
        elif name == "one_port":
            world, want = ONE_PORT, None
            init, acts = one_port_run()
        else:
            world, want = POOLW, None
            init, acts = bad_dest_run()
        trace = twin_trace(world, init, acts, seed, base, t0)
        for k in range(len(acts) if want is not None else 0):
            assert_same(trace[k], want[k], f"{name} {ids}: twin vs oracle, step {k}")
        if name == "bad_dest":  # the ship arrives at the clamped port on its first step: by the position, in a world with distinct ports
            assert len({tuple(p) for p in POOLW.ports}) == POOLW.P and init["dest"][BAD_ENV] == BAD_DEST >= POOLW.P
            assert trace[0]["origin"][BAD_ENV] == BAD_DEST and trace[0]["cargo"][BAD_ENV] == 0
            assert (np.delete(init["dest"], BAD_ENV) < POOLW.P).all(), "its wave's only such env"
        if name == "one_port":  # an arrival on every step of the blocked ships, on every other step of the returning ones
            assert ONE_PORT.P == 1 and (init["dest"] < ONE_PORT.P).all()
            for i in ONE_BLOCKED:
                assert [int(trace[k]["origin"][i]) for k in range(4)] == [0, 1, 0, 1] and trace[0]["dest"][i] == 1 and trace[0]["cargo"][i] == 0
                assert all(trace[k]["err"][i] == OK and (trace[k]["x"][i], trace[k]["y"][i]) == PORT2 for k in range(K))
            for i in ONE_RETURNS:
                assert trace[0]["origin"][i] == 0 and trace[0]["dest"][i] == 1 and trace[1]["y"][i] == PORT2[1] + 1 and trace[2]["origin"][i] == 1
        _TWIN[name, ids] = (world, init, acts, trace)
    return _TWIN[name, ids]


@pytest.mark.parametrize("ids", list(IDS))
def test_windows_scenario_on_the_oracle(ids, oracle_mod):
    init, acts, trace = oracle_reference(oracle_mod, ids)
    assert_scenario(oracle_mod, init, acts, trace, ids)


def test_shared_cell_scenario_on_the_oracle(oracle_mod):
    """The ring test's run: two ports on one cell, and a ship that arrives at the second of them (by the position)."""
    init, acts = hand_run()
    trace = oracle_trace(oracle_mod, HAND, init, acts)
    assert HAND.ports[3] == HAND.ports[4] and len({tuple(p) for p in HAND.ports}) < HAND.P
    prev = [init] + list(trace)
    at_shared = sum(int(((trace[k]["origin"] != prev[k]["origin"]) & (trace[k]["origin"] == 4))[:N_HAND & ~3].sum()) for k in range(min(KS[1:]) - 1))
    assert at_shared > 0, "no arrival at the second port of the shared cell"


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("name", ["windows", "hand", "bad_dest", "one_port"])
def test_windowed_run_equals_the_twin_and_the_oracle(name, ids, env, gpu_lib, oracle_mod):
    """Runs of 2, 17 and 40 steps from the same state end in the twin's bits, which are the oracle's."""
    seed, base, t0 = IDS[ids]
    world, init, acts, trace = twin_reference(oracle_mod, name, ids)
    b = world.env({"windows": N, "hand": N_HAND, "bad_dest": N_BAD, "one_port": N_ONE}[name], seed=seed, env_id_base=base, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"windows {name} {ids} {env}", t0)
    b.close()
