"""A regular wave of a fused se_step_seq carries each ship's position as the LDS address of its cell
in the bordered table (step_seq.h, step_group_ring<kAddr>; step_lean.h, "The carried cell
address"): a move adds a signed byte delta, dx (W + 2) + dy, read from a four-entry table the
launch derives from the image's packed moves; an arrival in a wave that does not test by the cell
code compares the address with the destination port's; after the inner steps a multiply and a shift
turn the address back into x and y. Maps up to 125 wide take that form; wider maps keep the packed
position (another instantiation of the kernel), and maps whose table does not fit the launch's LDS
(which now counts 16 bytes for the deltas) run the general step.

What can go wrong with a linear address: a stride of H + 2 for W + 2 or a delta built from the
wrong half of a move (a ship one row off on a non-square map, either way round), a row delta that
is truncated or loses its sign (W + 2 = 127 is the last that fits a byte), a move off the map that
changes the address or draws a gate, the way back to x, y at the first and last row and column, a
port's address made with the wrong bias (an arrival missed, or seen on another port's cell), the
table taken at a size where it no longer fits.

The method is step_seq_support's: a twin env stepped by plain steps, the C oracle's trace, and one
step_seq call of 2, 17 and 40 steps, all equal bit for bit in state, reward, done and err, with 2
plain steps after, under {}, SHIPENV_SEQ_GATE_POOL=0, SHIPENV_SEQ_RING=0 and SHIPENV_STEP_BLOCKS=1,
from counter 0 and with the counter wrapping 2^32. Every run is three whole waves, a wave of 20 lanes
and a tail of 3 envs.

  * `h7x9` and `h9x7`: the same hand-built layout on a 7 x 9 and on a 9 x 7 map, ports 3 and 4 on one
    cell (so no wave tests by the code: every arrival is the address compare). Wave 0 holds the
    scripts: a carrier on each edge that moves off it and one in each corner that tries both ways
    off, on every step (an error, no gate: cargo 55 stays; these ships never move, which pins the way
    back to x, y at the four extremes); a carrier beside ground in each direction (a move that stays:
    the gate fires, cargo is lost); an arrival; a ship that crosses another port's cell and does not
    arrive; a mover blocked by ground while standing on its destination, which arrives; an arrival at
    the second port of the shared cell. The other waves are random ships (test_gpu_step_seq_trim's
    generic_run).
  * `w125`, `w126`, `widest`: 45 x 125 (the last width with byte deltas), 45 x 126 (the first
    without) and the highest map 256 wide for which the launch still carries the table with the
    default pools, its height computed here from the launch's rule (`table_fits`). Sixteen lanes of
    walkers go up to 20 rows down the map and back, and as many up from the last row, in the first,
    the last and inner columns.
  * `past`: one row more than `widest`: no table, the general step.
  * test_gpu_step_seq_windows' second, third and fourth runs (two ports on one cell; a loaded dest
    >= P; the world of one port, whose blocked ship arrives on every step): its own references, the
    last two compared with the twin alone, as there.

The CPU companion asserts on the oracle's trace that each scripted case happens (claims per script)
and counts, over the inner steps of the 40-step run, the moves off the map per direction, the moves
blocked by ground, the arrivals (all by the address compare in these worlds) and the row moves of the
walkers; a count of 0 fails."""
import numpy as np
import pytest

from step_seq_support import OK, OOB, TAIL, assert_same, device_rows, gpu_lib, oracle_trace, run_fused, twin_trace  # noqa: F401
from test_gpu_step_seq_gatepool import IDS, image_bytes
from test_gpu_step_seq_ring import assert_claims
from test_gpu_step_seq_trim import E_, N_, S_, W_, World, generic_run
from test_gpu_step_seq_windows import twin_reference as windows_reference

gpu = pytest.mark.gpu

WAVE, PART_LANES = 256, 20
N = 3 * WAVE + 4 * PART_LANES + 3
KS = (2, 17, 40)
K = max(KS)
HEAVY = 55  # cargo >= 50: the gate, where it is drawn, fires with certainty
SETTINGS = [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_RING": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}]
DXY = {N_: (0, -1), E_: (-1, 0), S_: (0, 1), W_: (1, 0)}

# the launch's LDS besides the world image: the stocks by cell code, the waves' GATE pools, the move deltas
STOCK_TABLE, POOLS, DELTAS, LDS_PER_BLOCK, MAX_PORTS = 256 * 8, 4 * (64 + 32) * 16, 16, 160 * 1024 // 4, 253


def ids_of(env):
    return "-".join(f"{k[8:].lower()}{v}" for k, v in env.items()) or "plain"


def sized(H, W):
    return type(f"Map{H}x{W}", (World,), {"H": H, "W": W})


def table_fits(world):
    """launch_step_seq's rule with the default pools (step_lean.h, ring_table_fits): the bordered table
    in whole 16-byte units, and the move deltas behind it, beside the launch's other LDS."""
    table = ((world.H + 2) * (world.W + 2) + 15) & ~15
    return world.P <= MAX_PORTS and image_bytes(world) + STOCK_TABLE + POOLS + DELTAS + table <= LDS_PER_BLOCK


def hand(H, W):
    """Ports 0 in a corner, 1 on an edge, 2 in the interior with ground north of it, 3 and 4 on one
    cell, 5 in the last column; a second ground cell in open water."""
    return sized(H, W)(ports=[(0, 0), (0, 5), (3, 4), (5, 2), (5, 2), (6, 6)], fuel=[7, 5, 9, 4, 8, 6], cargo=[3, 6, 9, 2, 8, 5],
                       ground=[(3, 3), (5, 5)])


def wide(H, W):
    """Ports in a corner, in the last column and in the last row (a random ship at a port has a way
    off the map in every direction), ground north of the last port and in column 2."""
    return sized(H, W)(ports=[(0, 0), (1, W - 1), (H - 1, W // 2)], fuel=[7, 5, 9], cargo=[3, 6, 9],
                       ground=[(H - 1, W // 2 - 1), (2, 2), (H - 2, 2), (H // 2, 2)])


WIDE_W = 256
H_WIDEST = max(h for h in range(8, 257) if table_fits(wide(h, WIDE_W)))
WORLDS = {"h7x9": hand(7, 9), "h9x7": hand(9, 7), "w125": wide(45, 125), "w126": wide(45, 126),
          "widest": wide(H_WIDEST, WIDE_W), "past": wide(H_WIDEST + 1, WIDE_W)}
BORROWED = ("hand", "bad_dest", "one_port")  # test_gpu_step_seq_windows' runs


def hand_scripts(world):
    """[(label, ship (cell, origin, dest, cargo), first rows, rows repeated after them (None: selects, the
    ship stays), claims)]; a claim (k, field, value) holds after step k, "all": after every inner step
    of the run of 17."""
    H, W = world.H, world.W
    stay = [("all", "err", OOB), ("all", "cargo", HEAVY)]
    blocked = [("all", "err", OK), (KS[1] - 2, "lost", HEAVY)]
    out = []
    for label, cell, rows in (("off_north", (2, 0), (N_,)), ("off_south", (2, W - 1), (S_,)), ("off_east", (0, 3), (E_,)),
                              ("off_west", (H - 1, 3), (W_,)), ("corner_ne", (0, 0), (N_, E_)), ("corner_se", (0, W - 1), (S_, E_)),
                              ("corner_nw", (H - 1, 0), (N_, W_)), ("corner_sw", (H - 1, W - 1), (S_, W_))):
        out.append((label, (cell, 0, 2, HEAVY), [], rows, stay + [("all", "pos", cell)]))
    # beside the ground cell (5, 5) in each direction: a move that stays, the gate fires (cargo 55), cargo is lost
    for label, cell, row in (("ground_north", (5, 6), N_), ("ground_south", (5, 4), S_), ("ground_east", (6, 5), E_), ("ground_west", (4, 5), W_)):
        out.append((label, (cell, 0, 2, HEAVY), [], (row,), blocked + [("all", "pos", cell)]))
    out += [
        ("arrival", ((3, 5), 0, 2, 10), [N_], None, [(0, "pos", (3, 4)), (0, "origin", 2), (0, "cargo", 0), (0, "err", OK)]),
        # onto port 2's cell on the way to port 5, then blocked there by the ground north of it: no arrival
        ("crossing", ((3, 5), 0, 5, 0), [N_, N_], None, [(0, "pos", (3, 4)), (0, "origin", 0), (1, "pos", (3, 4)), (1, "err", OK), (1, "origin", 0), (1, "dest", 5)]),
        # blocked by the ground north of port 2 while standing on it, its destination: an arrival
        ("blocked_on_dest", ((3, 4), 0, 2, 20), [4 + 2, N_], None, [(0, "cargo", 20), (1, "err", OK), (1, "pos", (3, 4)), (1, "origin", 2), (1, "cargo", 0)]),
        # the shared cell carries port 3's code; the arrival at port 4 happens there
        ("shared_cell", ((5, 3), 0, 4, 10), [N_], None, [(0, "pos", (5, 2)), (0, "origin", 4), (0, "cargo", 0)]),
    ]
    return out


def script_envs(s):
    """Copy j of script s is env j of lane 4 s + j of wave 0."""
    return [4 * (4 * s + j) + j for j in range(4)]


WALK = 20  # rows a walker goes before it turns (fewer on a lower map)
WALK_LANES = 16
ARRIVERS = [4 * lane + lane % 4 for lane in (20, 41, 63)]  # wave 0, behind the walkers


def walk_columns(world):
    W = world.W
    return [0, 1, 3, W // 3, W // 2 + 1, W - 3, W - 2, W - 1]


def walkers(world):
    """[(env, first cell, the move it starts with, rows before it turns)]: lane l of wave 0, env l % 4."""
    H, cols = world.H, walk_columns(world)
    reach = min(WALK, H - 1)
    out = []
    for lane in range(WALK_LANES):
        down = lane % 2 == 0
        out.append((4 * lane + lane % 4, (0 if down else H - 1, cols[lane // 2]), W_ if down else E_, reach))
    return out


def run_of(name):
    world = WORLDS[name]
    rows = K + TAIL
    st, acts = generic_run(world, N, rows)
    if name.startswith("h"):
        scripts = hand_scripts(world)
        assert 16 * len(scripts) <= WAVE
        for s, (_, (cell, origin, dest, cargo), first, then, _) in enumerate(scripts):
            for i in script_envs(s):
                st["x"][i], st["y"][i] = cell
                st["origin"][i], st["dest"][i], st["cargo"][i] = origin, dest, cargo
                st["fuel"][i] = 100.0 + 0.125 * (i % 64)
                acts[:, i] = [then[k % len(then)] if then is not None else 4 + 2 + k % 2 for k in range(rows)]
                acts[:len(first), i] = first
    else:
        for i, cell, move, reach in walkers(world):
            st["x"][i], st["y"][i] = cell
            st["origin"][i], st["dest"][i], st["cargo"][i], st["fuel"][i] = 1, 2, 0, 200.0
            back = {W_: E_, E_: W_}[move]
            acts[:, i] = [move if (k // reach) % 2 == 0 else back for k in range(rows)]
        for i in ARRIVERS:  # beside the last port, bound for it: an arrival at step 0, then selects
            st["x"][i], st["y"][i] = world.H - 1, world.W // 2 + 1
            st["origin"][i], st["dest"][i], st["cargo"][i], st["fuel"][i] = 1, 2, 10, 200.0
            acts[:, i] = [N_] + [4 + k % 2 for k in range(1, rows)]
    return st, acts


def inner_counts(world, init, acts, trace):
    """Over the inner steps of the 40-step run and the envs of full groups: moves off the map by
    direction, moves blocked by ground, arrivals, and moves that changed the row."""
    prev = [init] + list(trace)
    full = len(init["x"]) & ~3
    off, blocked, arrived, row_moves = [0, 0, 0, 0], 0, 0, 0
    for k in range(K - 1):
        a, s0, s1 = acts[k][:full], prev[k], trace[k]
        mv = (a >= -4) & (a < 4)
        for d in range(4):
            tx, ty = s0["x"][:full] + DXY[d][0], s0["y"][:full] + DXY[d][1]
            out = (tx < 0) | (tx >= world.H) | (ty < 0) | (ty >= world.W)
            sel = mv & ((a & 3) == d)
            assert (s1["err"][:full][sel & out] == OOB).all()
            off[d] += int((sel & out).sum())
            inside = sel & ~out
            ground = np.zeros(full, bool)
            ground[inside] = world.water[tx[inside], ty[inside]] == 0
            stayed = (s1["x"][:full] == s0["x"][:full]) & (s1["y"][:full] == s0["y"][:full])
            assert stayed[ground].all() and (s1["err"][:full][ground] == OK).all()
            blocked += int(ground.sum())
        arrived += int((mv & (s1["err"][:full] == OK) & (s1["origin"][:full] != s0["origin"][:full])).sum())
        row_moves += int((s1["x"][:full] != s0["x"][:full]).sum())
    return off, blocked, arrived, row_moves


def assert_scenario(name, init, acts, trace):
    world = WORLDS[name]
    assert N % 4 == 3 and (N & ~3) % WAVE == 4 * PART_LANES
    regular = (init["dest"] < world.P) & (init["x"] < world.H) & (init["y"] < world.W)
    assert regular.all(), "every wave is regular"
    off, blocked, arrived, row_moves = inner_counts(world, init, acts, trace)
    print(name, f"{world.H} x {world.W}", "off the map by direction", off, "blocked", blocked, "arrivals", arrived, "row moves", row_moves)
    assert min(off) > 0 and blocked > 0 and arrived > 0 and row_moves > 0
    if name.startswith("h"):
        assert world.H != world.W and world.ports[3] == world.ports[4], "non-square, and no launch here tests by the code"
        claims_until = KS[1] - 2
        for s, (label, _, _, _, claims) in enumerate(hand_scripts(world)):
            flat = [(kk, f, v) for k, f, v in claims for kk in (range(claims_until + 1) if k == "all" else [k])]
            assert_claims(script_envs(s), flat, init, trace, f"{name} {label}")
        # the ships on the edges and in the corners never move in the whole run
        for s in range(8):
            e = script_envs(s)
            assert all((trace[k]["x"][e] == init["x"][e]).all() and (trace[k]["y"][e] == init["y"][e]).all() for k in range(K + TAIL))
        corners = {(int(init["x"][script_envs(s)[0]]), int(init["y"][script_envs(s)[0]])) for s in range(4, 8)}
        assert corners == {(0, 0), (0, world.W - 1), (world.H - 1, 0), (world.H - 1, world.W - 1)}
        return
    assert len({tuple(p) for p in world.ports}) == world.P
    cols = walk_columns(world)
    assert 0 in cols and world.W - 1 in cols and len(set(cols)) == len(cols)
    for i, (x0, y0), move, reach in walkers(world):  # row by row down (or up) the map, and back
        assert reach >= 16
        for k in range(2 * reach):
            step = k + 1 if k < reach else 2 * reach - k - 1
            want = x0 + DXY[move][0] * step
            assert (trace[k]["x"][i], trace[k]["y"][i], trace[k]["err"][i]) == (want, y0, OK), f"{name}: walker {i} after step {k}"
    for i in ARRIVERS:
        assert (trace[0]["x"][i], trace[0]["y"][i]) == tuple(world.ports[2]) and trace[0]["origin"][i] == 2 and trace[0]["cargo"][i] == 0


def test_the_sizes_stand_where_the_launch_rule_puts_them():
    """Byte deltas end at W = 125; the widest map with the table, and the first without."""
    assert WORLDS["w125"].W + 2 == 127 and WORLDS["w126"].W + 2 == 128
    assert all(table_fits(WORLDS[n]) for n in ("h7x9", "h9x7", "w125", "w126", "widest")) and not table_fits(WORLDS["past"])
    w = WORLDS["widest"]
    assert w.W == 256 and w.H != w.W and w.H >= 18 and WORLDS["past"].H == w.H + 1


_REF = {}


def oracle_reference(O, name, ids):
    if (name, ids) not in _REF:
        seed, base, t0 = IDS[ids]
        init, acts = run_of(name)
        trace = oracle_trace(O, WORLDS[name], init, acts, seed, base, t0)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _REF[name, ids] = (init, acts, trace)
    return _REF[name, ids]


_TWIN = {}


def twin_reference(O, name, ids):
    """(world, init, acts, the twin's recorded steps), the steps equal to the oracle's one by one
    (read-only, shared by the cases); the borrowed runs are test_gpu_step_seq_windows'."""
    if name in BORROWED:
        return windows_reference(O, name, ids)
    if (name, ids) not in _TWIN:
        seed, base, t0 = IDS[ids]
        init, acts, want = oracle_reference(O, name, ids)
        trace = twin_trace(WORLDS[name], init, acts, seed, base, t0)
        for k in range(len(acts)):
            assert_same(trace[k], want[k], f"{name} {ids}: twin vs oracle, step {k}")
        _TWIN[name, ids] = (WORLDS[name], init, acts, trace)
    return _TWIN[name, ids]


@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("name", list(WORLDS))
def test_scenario_on_the_oracle(name, ids, oracle_mod):
    init, acts, trace = oracle_reference(oracle_mod, name, ids)
    assert_scenario(name, init, acts, trace)


@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("name", list(WORLDS) + list(BORROWED))
def test_addressed_run_equals_the_twin_and_the_oracle(name, ids, env, gpu_lib, oracle_mod):
    """Runs of 2, 17 and 40 steps from the same state end in the twin's bits, which are the oracle's."""
    seed, base, t0 = IDS[ids]
    world, init, acts, trace = twin_reference(oracle_mod, name, ids)
    b = world.env(len(init["x"]), seed=seed, env_id_base=base, **env)
    dev = device_rows(b, acts)
    for Kl in KS:
        run_fused(b, init, dev, trace, Kl, None, f"celladdr {name} {ids} {env}", t0)
    b.close()
