"""What tests/test_gpu_step_seq_world_edits.py steps: worlds that follow one another on one handle
(se_set_ports), the launch rule of the fused se_step_seq restated, the runs and what they cover.

A fused se_step_seq launch takes its form from the world on the handle (launch_step_seq in
csrc/shipenv.hip, step_lean.h, step_seq.h): the GATE pools only where image, stock table and pools
fit 64 KiB; the bordered cell table only with P <= 253 and the launch's LDS under 40 KiB; the
carried cell address only up to W = 125; the arrival by cell code only with two or more ports on
distinct cells; and one launch for the run only while image and stock table fit 64 KiB. Every input
of that choice is rewritten by se_set_ports. A chain here is a map (the water is fixed at se_create)
and the worlds an env of that map is taken through, each on the far side of one of those thresholds
from its neighbour, and back.

  A  the 9 x 13 map of test_gpu_step_seq_trim's World: no port, one port (ONE), two ports on distinct
     cells, three ports with two on one cell, three distinct ports with every stock changed (one port
     emptied, one above every amount a take can ask for), the three ports moved to other water cells,
     64 ports (MANY), and two ports again.
  B  a 16 x 17 map: 253 ports (the most with the table), 254, 253, 254 with two on one cell, 2.
  C  four wide maps, each 2 -> 253 -> 2 ports, whose heights are computed from the restated rule
     (`tallest`): the 3 words per port carry the image over one of its 1024-word rows, and with it
     the launch loses the table (one map at W = 125, the address form, one at W = 256, the packed
     form), the GATE pools, or the fused launch altogether.

This module imports neither torch nor the library; what it borrows from the other step-sequence
files (World, generic_run, scenarios, image_bytes, sized, table_fits, inner_counts) it imports where
it is used."""
import types

import numpy as np

WAVE, PART_LANES = 256, 20
N = 3 * WAVE + 4 * PART_LANES + 3  # test_gpu_step_seq_celladdr's batch
KS = (2, 17, 40)
K = max(KS)
TAIL = 2
N_, E_, S_, W_ = 0, 1, 2, 3  # moves by (dx, dy): (0, -1), (-1, 0), (0, 1), (1, 0); x is the map row
OK, AMOUNT = 0, 5
LAST_CLAIM = KS[1] - 2  # a claim is about an inner step of the runs of 17 and of 40
K_CARRIED = KS[1]  # chain D: steps before and after the edit

# the launch's LDS besides the world image (step_seq.h): the stocks by cell code, the waves' GATE pools
STOCK_TABLE, POOLS, LDS_LAUNCH = 256 * 8, 4 * (64 + 32) * 16, 64 * 1024
BYTE_DELTA_W = 125  # the widest map whose row delta, W + 2, fits a signed byte
MAX_TABLE_PORTS = 253

# ground of map A: off the cells of ONE, MANY and the scripts below, on the edges and in open water
GROUND_A = [(8, 12), (7, 5), (0, 6), (4, 0), (4, 12), (7, 9), (6, 11), (0, 12)]
# ground of map B (16 x 17): 268 water cells
GROUND_B = [(5, 5), (10, 11), (3, 14), (12, 2)]
HB, WB = 16, 17


# ----------------------------------------------------------------- the launch rule, restated
def shape(H, W, P):
    return types.SimpleNamespace(H=H, W=W, P=P)


def fuses(w):
    """se_step_seq_mark: one launch for the run while the image and the stock table fit."""
    from test_gpu_step_seq_gatepool import image_bytes

    return image_bytes(w) + STOCK_TABLE <= LDS_LAUNCH


def pools_fit(w):
    """launch_step_seq: the GATE pools behind the image and the stock table."""
    from test_gpu_step_seq_gatepool import image_bytes

    return image_bytes(w) + STOCK_TABLE + POOLS <= LDS_LAUNCH


def table_carried(w):
    """ring_table_fits with the default pools, as test_gpu_step_seq_celladdr states it."""
    from test_gpu_step_seq_celladdr import table_fits

    return fuses(w) and pools_fit(w) and table_fits(w)


def launch_form(world):
    """What a default launch on this world is: fused, pools, table, addr (the carried cell address),
    by_code (arrivals tested by the cell code where a wave is regular)."""
    table = table_carried(world)
    distinct = len({tuple(p) for p in world.ports}) == world.P
    return dict(fused=fuses(world), pools=pools_fit(world), table=table, addr=table and world.W <= BYTE_DELTA_W,
                by_code=distinct and world.P >= 2)


def tallest(W, rule, few=2, many=MAX_TABLE_PORTS):
    """The tallest map W wide (H != W) on which `rule` holds with `few` ports and no longer with `many`."""
    return max(h for h in range(8, 257) if h != W and rule(shape(h, W, few)) and not rule(shape(h, W, many)))


# ----------------------------------------------------------------- the worlds
def _world(H, W, ground, ports, fuel, cargo):
    from test_gpu_step_seq_celladdr import sized

    return sized(H, W)(ports=ports, fuel=fuel, cargo=cargo, ground=ground)


def lattice(H, W, count):
    """`count` cells on 16 columns from column 0 and up to 16 rows from row 0: distinct, many on the edges."""
    return [((i // 16) * (H // 16), (i % 16) * (W // 16)) for i in range(count)]


def wide_ground(H, W):
    """A handful of ground cells beside ports of both worlds of a wide map (none of them a lattice cell)."""
    cells = lattice(H, W, MAX_TABLE_PORTS)
    return [(0, 1), (2, W - 1)] + [(x, y + 1) for x, y in (cells[i] for i in (5, 40, 100, 200, 252))]


def many_stocks(count):
    """Stocks that differ from port to port, some 0, some above every amount a take can ask for."""
    return [(37 * i + 11) % 230 for i in range(count)], [(5 * i + 3) % 60 for i in range(count)]


_CHAINS = {}


def chains():
    """{chain: [(label, world, reference)]}: reference "oracle", or "twin" where the C oracle is not
    the reference (a world of one port). Worlds that come twice are one object."""
    if _CHAINS:
        return _CHAINS
    from test_gpu_step_seq_trim import MANY, NO_PORT, ONE

    def a(ports, fuel, cargo):
        return _world(9, 13, GROUND_A, ports, fuel, cargo)

    two = a([(2, 2), (6, 8)], [150, 60], [40, 25])
    _CHAINS["A"] = [
        ("none", a(NO_PORT.ports, [], []), "oracle"),
        ("one", a(ONE.ports, ONE.fuel_stock, ONE.cargo_stock), "twin"),
        ("two", two, "oracle"),
        ("shared", a([(2, 2), (6, 8), (6, 8)], [150, 60, 199], [40, 10, 49]), "oracle"),
        ("restocked", a([(2, 2), (6, 8), (4, 10)], [0, 250, 90], [0, 60, 25]), "oracle"),
        ("moved", a([(3, 3), (7, 7), (1, 10)], [0, 250, 90], [0, 60, 25]), "oracle"),
        ("many", a(MANY.ports, MANY.fuel_stock, MANY.cargo_stock), "oracle"),
        ("two_again", two, "oracle"),
    ]

    water_b = [(x, y) for x in range(HB) for y in range(WB) if (x, y) not in GROUND_B]
    fuel, cargo = many_stocks(254)

    def b(ports):
        return _world(HB, WB, GROUND_B, ports, fuel[:len(ports)], cargo[:len(ports)])

    most = b(water_b[:253])
    _CHAINS["B"] = [
        ("p253", most, "oracle"),
        ("p254", b(water_b[:254]), "oracle"),
        ("p253_again", most, "oracle"),
        ("p254_shared", b(water_b[:253] + [water_b[7]]), "oracle"),
        ("p2", b([water_b[0], water_b[-1]]), "oracle"),
    ]

    fuel, cargo = many_stocks(MAX_TABLE_PORTS)
    for name, (H, W) in wide_maps().items():
        few = _world(H, W, wide_ground(H, W), [(0, 0), (1, W - 1)], [150, 60], [40, 25])
        many = _world(H, W, wide_ground(H, W), lattice(H, W, MAX_TABLE_PORTS), fuel, cargo)
        _CHAINS[name] = [("p2", few, "oracle"), ("p253", many, "oracle"), ("p2_again", few, "oracle")]
    return _CHAINS


def wide_maps():
    """Chain C's maps, each the tallest on which the port count alone decides."""
    return {"C_table_addr": (tallest(BYTE_DELTA_W, table_carried), BYTE_DELTA_W),
            "C_table_packed": (tallest(256, table_carried), 256),
            "C_pools": (tallest(256, pools_fit), 256),
            "C_fused": (tallest(256, fuses), 256)}


CHAIN_NAMES = ("A", "B", "C_table_addr", "C_table_packed", "C_pools", "C_fused")
# what the launch rule must say of every world of chains B and C, in order (None: not what the chain is about)
EXPECTED = {
    "B": [dict(table=True, addr=True, by_code=True), dict(table=False, by_code=True), dict(table=True, addr=True, by_code=True),
          dict(table=False, by_code=False), dict(table=True, addr=True, by_code=True)],
    "C_table_addr": [dict(fused=True, pools=True, table=True, addr=True), dict(fused=True, pools=True, table=False, addr=False),
                     dict(fused=True, pools=True, table=True, addr=True)],
    "C_table_packed": [dict(fused=True, pools=True, table=True, addr=False), dict(fused=True, pools=True, table=False),
                       dict(fused=True, pools=True, table=True, addr=False)],
    "C_pools": [dict(fused=True, pools=True, table=False), dict(fused=True, pools=False, table=False), dict(fused=True, pools=True, table=False)],
    "C_fused": [dict(fused=True, pools=False), dict(fused=False, pools=False), dict(fused=True, pools=False)],
    "A": [dict(by_code=False, table=True, addr=True)] * 2 + [dict(by_code=True, table=True), dict(by_code=False, table=True)]
         + [dict(by_code=True, table=True, addr=True)] * 4,
}
# the one entry of launch_form in which neighbouring worlds of the chain differ
CROSSES = {"B": "table", "C_table_addr": "table", "C_table_packed": "table", "C_pools": "pools", "C_fused": "fused"}


def cases():
    """(chain, index) of every world of every chain."""
    return [(c, i) for c in CHAIN_NAMES for i in range(len(chains()[c]))]


# ----------------------------------------------------------------- the runs
def scripts(chain, label):
    """[(label, (cell, origin, dest, cargo), first rows, claims)] laid over the random run of a world
    of chains A and C; after its first rows a ship selects (it stays). A claim (k, field, value) holds after
    step k <= LAST_CLAIM. Cargo is 0 wherever a claim reads it after a move (no gate)."""
    w = dict((name, world) for name, world, _ in chains()[chain])[label]
    if chain.startswith("C"):
        # on a wide map the random ships are far from every port: two ships one and three cells beside a port, bound for it
        d, (x, y) = (1, w.ports[1]) if w.P == 2 else (17, w.ports[17])
        return [(f"arrives_after_{n}", ((x, y - n), 0, d, 10), [S_] * n, [(n - 1, "pos", (x, y)), (n - 1, "origin", d), (n - 1, "cargo", 0), (n - 1, "err", OK)])
                for n in (1, 3)]
    if chain != "A":
        return []
    if label == "shared":
        # the shared cell carries port 1's code and answers with port 1's stocks (10 cargo), not port 2's (49)
        return [("second_of_shared", ((6, 9), 0, 2, 0), [N_], [(0, "pos", (6, 8)), (0, "origin", 2), (0, "err", OK)]),
                ("shared_stocks", ((6, 8), 0, 1, 0), [w.cargo(11), w.cargo(10)], [(0, "err", AMOUNT), (0, "cargo", 0), (1, "err", OK), (1, "cargo", 10)])]
    if label == "restocked":
        # port 0 had 150 fuel and 40 cargo, port 1 60 fuel and 10 cargo in the world before
        return [("refused_at_emptied", ((2, 2), 1, 2, 0), [w.cargo(1), w.fuel(1)], [(0, "err", AMOUNT), (1, "err", AMOUNT), (1, "cargo", 0)]),
                ("past_the_old_stock", ((6, 8), 0, 2, 0), [w.cargo(45), w.fuel(150)], [(0, "err", OK), (0, "cargo", 45), (1, "err", OK), (1, "fuel_gain", True)])]
    if label == "moved":
        # port 0 went from (2, 2) to (3, 3): over the old cell without arriving, then onto the new one
        return [("crosses_old_cell", ((2, 1), 1, 0, 0), [S_, W_, S_],
                 [(0, "pos", (2, 2)), (0, "origin", 1), (0, "dest", 0), (0, "err", OK), (1, "pos", (3, 2)), (1, "origin", 1),
                  (2, "pos", (3, 3)), (2, "origin", 0), (2, "err", OK)]),
                ("back_onto_old_cell", ((2, 2), 1, 0, 0), [E_, W_], [(0, "pos", (1, 2)), (1, "pos", (2, 2)), (1, "origin", 1), (1, "dest", 0), (1, "err", OK)])]
    return []


def script_envs(s):
    """Copy j of script s is env j of lane 4 s + j of wave 0."""
    return [4 * (4 * s + j) + j for j in range(4)]


def scripted_run(name, world, n, rows):
    """A world of fewer than two ports: test_gpu_step_seq_trim's scenarios of that world, lane j of
    group g running scenario (g + j) % S, and after their rows actions drawn as generic_run draws them."""
    from step_seq_support import empty_state
    from test_gpu_step_seq_trim import K_SCN, WORLDS, scenarios

    theirs = WORLDS[name]
    assert (world.ports, world.fuel_stock, world.cargo_stock) == (theirs.ports, theirs.fuel_stock, theirs.cargo_stock)
    scn = scenarios(name)
    rng = np.random.default_rng(n + world.P)
    st = empty_state(n)
    acts = rng.integers(-6, world.A + 3, (rows, n)).astype(np.int32)
    moves = rng.integers(-4, 4, (rows, n)).astype(np.int32)
    acts = np.where(rng.random((rows, n)) < 0.5, moves, acts)
    for i in range(n):
        _, sh, first, _ = scn[(i // 4 + i % 4) % len(scn)]
        st["x"][i], st["y"][i] = sh["cell"]
        st["origin"][i], st["dest"][i], st["cargo"][i] = sh["origin"], sh["dest"], sh["cargo"]
        st["fuel"][i] = sh["fuel"] + 0.125 * (i % 64)
        acts[:K_SCN, i] = first
    return st, acts


_RUNS = {}


def run_of(chain, i):
    """(init, acts) of world i of the chain, K + TAIL rows: generic_run's ships and actions with the
    world's scripts in the first lanes of wave 0. Shared and read-only."""
    label, world, _ = chains()[chain][i]
    if id(world) not in _RUNS:
        from test_gpu_step_seq_trim import generic_run

        rows = K + TAIL
        if world.P < 2:
            st, acts = scripted_run(label, world, N, rows)
        else:
            st, acts = generic_run(world, N, rows)
            for s, (_, (cell, origin, dest, cargo), first, _) in enumerate(scripts(chain, label)):
                for e in script_envs(s):
                    st["x"][e], st["y"][e] = cell
                    st["origin"][e], st["dest"][e], st["cargo"][e] = origin, dest, cargo
                    st["fuel"][e] = 100.0 + 0.125 * (e % 64)
                    acts[:, e] = [4 + k % 2 for k in range(rows)]
                    acts[:len(first), e] = first
        for v in st.values():  # the actions stay writable: torch.from_numpy takes them as they are
            v.setflags(write=False)
        _RUNS[id(world)] = (st, acts, world)  # the world is kept: its id stays its own
    return _RUNS[id(world)][:2]


_ORACLE = {}


def oracle_reference(O, chain, i, ids):
    """(world, init, acts, the C oracle's K + TAIL recorded steps), shared and read-only."""
    from step_seq_support import oracle_trace
    from test_gpu_step_seq_gatepool import IDS

    _, world, _ = chains()[chain][i]
    if (id(world), ids) not in _ORACLE:
        seed, base, t0 = IDS[ids]
        init, acts = run_of(chain, i)
        trace = oracle_trace(O, world, init, acts, seed, base, t0)
        for s in trace:
            for v in s.values():
                v.setflags(write=False)
        _ORACLE[id(world), ids] = (world, init, acts, trace)
    return _ORACLE[id(world), ids]


# ----------------------------------------------------------------- what a run covers
def coverage(world, init, acts, trace):
    """Counts over the inner steps of the 40-step run and the envs of full groups."""
    from test_gpu_step_seq_celladdr import inner_counts

    off, blocked, arrived, _ = inner_counts(world, init, acts, trace)
    P, full = world.P, len(init["x"]) & ~3
    prev = [init] + list(trace)
    took_cargo = took_fuel = lost = 0
    for k in range(K - 1):
        a, s0, s1 = acts[k][:full], prev[k], trace[k]
        ok = s1["err"][:full] == OK
        took_cargo += int((ok & (a >= 4 + P) & (a < 54 + P) & (s1["cargo"][:full] > s0["cargo"][:full])).sum())
        took_fuel += int((ok & (a >= 54 + P) & (s1["fuel"][:full] > s0["fuel"][:full])).sum())
        mv = ok & (a >= -4) & (a < 4)
        lost += int((mv & (s1["origin"][:full] == s0["origin"][:full]) & (s1["cargo"][:full] < s0["cargo"][:full])).sum())
    return dict(arrivals=arrived, took_cargo=took_cargo, took_fuel=took_fuel, lost_at_gate=lost, off_the_map=sum(off), blocked_by_ground=blocked)


def assert_claims(chain, label, init, trace):
    prev = [init] + list(trace)
    for s, (what, _, _, claims) in enumerate(scripts(chain, label)):
        envs = script_envs(s)
        assert max(envs) < WAVE
        for k, field, want in claims:
            assert k <= LAST_CLAIM, f"{what}: a claim about step {k} is about no inner step of the run of {KS[1]}"
            if field == "pos":
                got = np.stack([trace[k]["x"][envs], trace[k]["y"][envs]], 1)
                assert (got == np.array(want)).all(), f"{label} {what}: step {k} position {got[0]} != {want}"
            elif field == "fuel_gain":
                assert (trace[k]["fuel"][envs] > prev[k]["fuel"][envs]).all(), f"{label} {what}: step {k} fuel did not rise"
            else:
                assert (trace[k][field][envs] == want).all(), f"{label} {what}: step {k} {field} {trace[k][field][envs]} != {want}"


def assert_regular(world, init, trace):
    """Every wave is regular from the first step to the last: inside the map, dest < P."""
    for s in [init] + list(trace):
        assert ((s["dest"] < world.P) & (s["x"] < world.H) & (s["y"] < world.W) & (s["x"] >= 0) & (s["y"] >= 0)).all()
