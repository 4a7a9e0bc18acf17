"""se_set_ports rewrites everything a fused se_step_seq launch chooses its form from: the image and
the bordered table behind it, dims, ports_distinct, and a device block that moves when it grows
(upload_world, csrc/shipenv.hip). The other test_gpu_step_seq_*.py files make a fresh env for every
world; here one env per map is taken through a chain of worlds (world_edit_support: A the port-count
and distinct-cell edges on the 9 x 13 map, B the table's port limit on a 16 x 17 map, C four wide
maps on which the port count alone takes the table, the GATE pools or the fused launch away) and is
never closed between them. A launch decision cached at se_create, a ports_distinct left over from the
ports before, a table that is not uploaded again or goes to the old block, a stock table of the old
stocks: each would show here and nowhere else in the suite.

For every world of a chain, in order: set_ports (the first world is the one the env was made
with); the world's run loaded at counter t0 (test_gpu_step_seq_trim's generic_run: ships at ports
and at sea, cargo 0 .. 59, actions over and a little beyond the action space, half of them moves;
for the worlds of no port and of one port that file's scenarios); step_seq of 2, 17 and 40 rows, each
from the same loaded state, and 2 plain steps after. Each run must end in the bits (state, reward,
done, err, counter) of the C oracle's trace for that world and of a twin, a fresh env of that world
stepped by plain step calls. The world of one port is compared with the twin alone, as
test_gpu_step_seq_windows does. The batch is test_gpu_step_seq_celladdr's (three whole waves, a wave
of 20 lanes, a tail of 3 envs), the ids and the settings are the project's: plain and a key and
counter that wrap 2^32; {}, SHIPENV_SEQ_GATE_POOL=0, SHIPENV_SEQ_RING=0 and SHIPENV_STEP_BLOCKS=1,
each applied at se_create of the edited handle. Nothing here has a tolerance.

Chain D carries the state over an edit: after a fused run on the 64-port world the env goes to three
ports without a reload, so ships hold origins and destinations >= P and cargo taken at the old
stocks. The edit must change no byte of the state, the outputs or the counters, and 17 fused steps
on the edited handle must end where 17 plain steps of a fresh env loaded with that snapshot end.

The other kernels that stage the world from the handle at launch and had no test after a set_ports
(se_sample_actions, se_rollout, se_rollout_plan, se_mcts_choose) run on one env of map A taken
through two ports, 64 ports and three ports with a shared cell, with an se_mcts handle made before
the first edit, against a fresh env and agent of each world.

The tests without the gpu mark assert, with the restated launch rule and the C oracle alone, that
every world stands on its side of its threshold, that neighbours stand on opposite sides, and that
every run goes through arrivals, passed takes of both kinds, cargo lost at the gate, moves off the
map and moves blocked by ground in its inner steps; a count of 0 fails."""
import numpy as np
import pytest

import world_edit_support as S
from step_seq_support import NONE, TAIL, assert_same, device_rows, gpu_lib, load, run_fused, snapshot, twin_trace  # noqa: F401
from test_gpu_step_seq_celladdr import KS, N, SETTINGS, ids_of
from test_gpu_step_seq_gatepool import IDS
from test_gpu_step_seq_trim import MANY, NO_PORT, ONE, World

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


# ----------------------------------------------------------------- the CPU companions
def test_the_batch_the_runs_and_the_settings_are_the_projects():
    assert (S.N, S.KS, S.TAIL) == (N, KS, TAIL) and N % 4 == 3 and (N & ~3) % S.WAVE == 4 * S.PART_LANES
    assert sorted(IDS) == ["plain", "wrap"] and IDS["wrap"][1] >> 32 and IDS["wrap"][2] + S.K > 1 << 32
    assert SETTINGS == [{}, {"SHIPENV_SEQ_GATE_POOL": "0"}, {"SHIPENV_SEQ_RING": "0"}, {"SHIPENV_STEP_BLOCKS": "1"}]


def test_chain_a_walks_the_port_count_and_distinct_cell_edges():
    a = S.chains()["A"]
    worlds = [w for _, w, _ in a]
    assert all((w.H, w.W) == (World.H, World.W) and w.H != w.W and (w.water == worlds[0].water).all() for w in worlds)
    assert [w.P for w in worlds] == [0, 1, 2, 3, 3, 3, 64, 2] and worlds[7] is worlds[2]
    assert worlds[0].ports == NO_PORT.ports and worlds[1].ports == ONE.ports and worlds[6].ports == MANY.ports
    assert [ref for _, _, ref in a] == ["oracle", "twin"] + ["oracle"] * 6
    assert [S.launch_form(w)["by_code"] for w in worlds] == [False, False, True, False, True, True, True, True]
    shared, restocked, moved = worlds[3], worlds[4], worlds[5]
    # two ports on one cell, and it carries the lower port's code (the oracle's claim on it is in the scripts)
    assert shared.ports[1] == shared.ports[2] != shared.ports[0] and shared.cargo_stock[1] != shared.cargo_stock[2]
    # distinct again, every stock changed, one port emptied, one above every amount a take can ask for
    assert len({tuple(p) for p in restocked.ports}) == 3 and restocked.ports[:2] == shared.ports[:2]
    assert all(f != g and c != d for f, g, c, d in zip(restocked.fuel_stock, shared.fuel_stock, restocked.cargo_stock, shared.cargo_stock))
    assert (restocked.fuel_stock[0], restocked.cargo_stock[0]) == (0, 0) and restocked.fuel_stock[1] > 199 and restocked.cargo_stock[1] > 49
    # every port on another water cell, the old cells plain water
    assert moved.P == restocked.P and not {tuple(p) for p in moved.ports} & {tuple(p) for p in restocked.ports}
    assert all(moved.water[x, y] for x, y in moved.ports + restocked.ports)
    for w in worlds:
        assert all(0 <= x < w.H and 0 <= y < w.W and w.water[x, y] for x, y in w.ports)


def test_the_worlds_stand_where_the_launch_rule_puts_them():
    """Every world of chains B and C on its side of its threshold, its neighbours on the other side."""
    maps = S.wide_maps()
    print(maps)
    for name, (H, W) in maps.items():
        assert H != W and W == (S.BYTE_DELTA_W if name == "C_table_addr" else 256) and 8 < H <= 256
        # one row more and the port count no longer decides: the tallest such map
        rule = {"C_table_addr": S.table_carried, "C_table_packed": S.table_carried, "C_pools": S.pools_fit, "C_fused": S.fuses}[name]
        assert rule(S.shape(H, W, 2)) and not rule(S.shape(H, W, S.MAX_TABLE_PORTS))
    for chain in S.CHAIN_NAMES:
        worlds = S.chains()[chain]
        forms = [S.launch_form(w) for _, w, _ in worlds]
        assert len(forms) == len(S.EXPECTED[chain])
        for (label, w, _), form, want in zip(worlds, forms, S.EXPECTED[chain]):
            assert {k: form[k] for k in want} == want, f"{chain} {label} ({w.H} x {w.W}, {w.P} ports): {form}"
            assert len({tuple(p) for p in w.ports}) == w.P or "shared" in label
            assert all(w.water[x, y] for x, y in w.ports) and w.H != w.W
        if chain in S.CROSSES:
            side = [f[S.CROSSES[chain]] for f in forms]
            assert all(p != q for p, q in zip(side, side[1:])), f"{chain}: {side}"
    b = [w for _, w, _ in S.chains()["B"]]
    assert [w.P for w in b] == [253, 254, 253, 254, 2] and b[3].ports[253] == b[3].ports[7] and int(b[0].water.sum()) >= 254
    # the image grows by 3 words per port over a 1024-word row on every wide map
    from test_gpu_step_seq_gatepool import image_bytes

    for chain in ("C_table_addr", "C_table_packed", "C_pools", "C_fused"):
        few, many, again = (w for _, w, _ in S.chains()[chain])
        assert again is few and (few.P, many.P) == (2, 253) and image_bytes(many) == image_bytes(few) + 4096
        assert (few.water == many.water).all() and 4 <= int((few.water == 0).sum()) <= 8


REFERENCED = [(c, i) for c, i in S.cases() if S.chains()[c][i][1].P >= 2]


@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("chain,i", REFERENCED, ids=[f"{c}-{S.chains()[c][i][0]}" for c, i in REFERENCED])
def test_world_run_on_the_oracle(chain, i, ids, oracle_mod):
    """The run of every world of two or more ports goes through every kind of step in its inner steps,
    holds what its scripts claim, and keeps every wave regular."""
    label, world, _ = S.chains()[chain][i]
    _, init, acts, trace = S.oracle_reference(oracle_mod, chain, i, ids)
    counts = S.coverage(world, init, acts, trace)
    print(chain, label, ids, f"{world.H} x {world.W}, {world.P} ports", counts)
    assert all(v > 0 for v in counts.values()), counts
    S.assert_claims(chain, label, init, trace)
    S.assert_regular(world, init, trace)


def test_the_carried_state_holds_indices_of_the_old_world(oracle_mod):
    """Chain D on the oracle: after 17 steps on the 64-port world ships hold origins and destinations
    that no world of three ports has, and cargo."""
    _, init, acts, trace = S.oracle_reference(oracle_mod, "A", 6, "plain")
    end = trace[S.K_CARRIED - 1]
    assert (end["dest"] >= 3).sum() > 100 and (end["origin"] >= 3).sum() > 100 and (end["cargo"] > 0).sum() > 100
    assert (end["origin"] != init["origin"]).any(), "and some arrived there"


# ----------------------------------------------------------------- the references
_TWIN = {}


def twin_reference(O, chain, i, ids):
    """(world, init, acts, the twin's recorded steps, the oracle's or None): the twin a fresh env of
    that world, equal to the oracle step by step where the oracle is the reference. Shared, read-only."""
    label, world, ref = S.chains()[chain][i]
    if (id(world), ids) not in _TWIN:
        seed, base, t0 = IDS[ids]
        init, acts = S.run_of(chain, i)
        trace = twin_trace(world, init, acts, seed, base, t0)
        want = S.oracle_reference(O, chain, i, ids)[3] if ref == "oracle" else None
        for k in range(len(acts) if want is not None else 0):
            assert_same(trace[k], want[k], f"{chain} {label} {ids}: twin vs oracle, step {k}")
        _TWIN[id(world), ids] = (world, init, acts, trace, want)
    return _TWIN[id(world), ids]


def edit(env, world):
    env.set_ports(world.ports, world.fuel_stock, world.cargo_stock)
    assert env.P == world.P


# ----------------------------------------------------------------- chains A, B and C
@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("chain", S.CHAIN_NAMES)
def test_edited_handle_equals_the_oracle_and_the_twin(chain, ids, env, gpu_lib, oracle_mod):
    """One handle through the chain's worlds: after every set_ports, runs of 2, 17 and 40 steps from
    the same state end in the oracle's bits for that world and in a fresh env's."""
    seed, base, t0 = IDS[ids]
    worlds = S.chains()[chain]
    b = worlds[0][1].env(N, seed=seed, env_id_base=base, **env)
    try:
        for i, (label, world, _) in enumerate(worlds):
            if i:
                edit(b, world)
            _, init, acts, twin, oracle = twin_reference(oracle_mod, chain, i, ids)
            dev = device_rows(b, acts)
            for Kl in KS:
                for name, trace in (("oracle", oracle), ("twin", twin)):
                    if trace is not None:
                        run_fused(b, init, dev, trace, Kl, None, f"edits {chain} world {i} ({label}) {ids} {env} vs the {name}", t0)
    finally:
        b.close()


# ----------------------------------------------------------------- chain D
@gpu
@pytest.mark.parametrize("env", SETTINGS, ids=ids_of)
@pytest.mark.parametrize("ids", list(IDS))
@pytest.mark.parametrize("target", ["restocked", "shared"])
def test_state_carried_over_an_edit(target, ids, env, gpu_lib):
    """64 ports -> 3 ports (distinct cells: arrivals by code are allowed again; or a shared cell)
    without a reload: the edit changes no byte, and the fused run on the edited handle equals plain
    steps of a fresh env loaded with the snapshot."""
    seed, base, t0 = IDS[ids]
    a = S.chains()["A"]
    labels = [label for label, _, _ in a]
    many, small = a[labels.index("many")][1], a[labels.index(target)][1]
    b = a[labels.index("two")][1].env(N, seed=seed, env_id_base=base, **env)
    fresh = small.env(N, seed=seed, env_id_base=base)
    try:
        edit(b, many)
        init, acts = S.run_of("A", labels.index("many"))
        load(b, init, t0)
        b.step_seq(device_rows(b, acts)[:S.K_CARRIED])
        before, counters = snapshot(b), b.counters
        edit(b, small)
        after = snapshot(b)
        assert_same(after, before, f"carried {target} {ids} {env}: the edit itself")
        assert b.counters == counters == (t0 + S.K_CARRIED, 0)
        assert (after["dest"] >= small.P).sum() > 100 and (after["origin"] >= small.P).sum() > 100 and (after["cargo"] > 0).sum() > 100
        load(fresh, after, counters[0])
        rows = S.run_of("A", labels.index(target))[1][:S.K_CARRIED]
        b.step_seq(device_rows(b, rows))
        dev = device_rows(fresh, rows)
        for k in range(S.K_CARRIED):
            fresh.step(dev[k].contiguous())
        assert_same(snapshot(b), snapshot(fresh), f"carried {target} {ids} {env}: {S.K_CARRIED} steps after the edit")
        assert b.counters == fresh.counters == (t0 + 2 * S.K_CARRIED, 0)
    finally:
        b.close()
        fresh.close()


# ----------------------------------------------------------------- the other consumers of the world
SIMS, ROLLOUT_STEPS = 4, 6


def padded(env, rows):
    """[len(rows), n] device view at a padded stride (a multiple of 4), as rollout_plan takes its plan."""
    n = rows[0].numel()
    buf = torch.zeros((len(rows), ((n + 3) & ~3) + 8), dtype=torch.int32, device=env.device)
    for k, r in enumerate(rows):
        buf[k, :n].copy_(r)
    return buf[:, :n]


def consumer_state(init):
    """The world's loaded run with the ships sample_action reads the world for: every fourth ship without
    cargo (at a port: a take of up to the port's stock), every fifth without a destination (at a port:
    a select among the other ports)."""
    st = {f: v.copy() for f, v in init.items()}
    st["cargo"][1::4] = 0
    st["dest"][2::5] = NONE
    return st


def consumers(env, agent):
    """Everything se_sample_actions, se_rollout, se_rollout_plan and se_mcts_choose write, by name, as bytes."""
    out = {}
    drawn = [tuple(t.clone() for t in env.sample_actions(t)) for t in range(ROLLOUT_STEPS)]
    for t, row in enumerate(drawn):
        out.update({f"sample_actions({t}).{f}": v for f, v in zip(("type", "a", "b"), row)})
    src = torch.arange(env.n, dtype=torch.int32, device=env.device)
    out.update(zip(("rollout.ret", "rollout.steps", "rollout.status"), env.rollout(src, max_steps=ROLLOUT_STEPS, rollout_base=7 * env.n)))
    plan = [padded(env, [row[j] for row in drawn]) for j in range(3)]
    res = env.rollout_plan(src, *plan, rollout_base=3 * env.n, return_end=True)
    out.update({f"rollout_plan.{f}": v for f, v in res._asdict().items()})
    ty, a, b, status, tree = agent.choose_action(return_tree=True)
    out.update({"choose.type": ty, "choose.a": a, "choose.b": b, "choose.status": status})
    out.update({f"choose.tree.{f}": v for f, v in tree._asdict().items()})
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in out.items()}


@gpu
@pytest.mark.parametrize("ids", list(IDS))
def test_other_consumers_on_the_edited_handle(ids, gpu_lib):
    """Two ports -> 64 ports -> three ports with a shared cell on one env, the se_mcts handle made
    before the first edit: sample_actions, rollout, rollout_plan and the MCTS decision with its tree
    equal a fresh env's and agent's bit for bit, and leave the env's own state alone."""
    from shippingenv_amd.mcts import VecMCTSAgent

    seed, base, t0 = IDS[ids]
    a = S.chains()["A"]
    labels = [label for label, _, _ in a]
    env = a[labels.index("two")][1].env(N, seed=seed, env_id_base=base)
    agent = VecMCTSAgent(env, num_simulations=SIMS, max_rollout_steps=ROLLOUT_STEPS)
    try:
        for stage, label in enumerate(("two", "many", "shared")):
            i = labels.index(label)
            world = a[i][1]
            if stage:
                edit(env, world)
            init = consumer_state(S.run_of("A", i)[0])
            fresh = world.env(N, seed=seed, env_id_base=base)
            fagent = VecMCTSAgent(fresh, num_simulations=SIMS, max_rollout_steps=ROLLOUT_STEPS)
            try:
                for e in (env, fresh):
                    load(e, init, t0)
                fagent.mcts_base = agent.mcts_base  # the kept agent has decided before
                before, counters = snapshot(env), env.counters
                got, want = consumers(env, agent), consumers(fresh, fagent)
                assert sorted(got) == sorted(want) and len(got) == 3 * ROLLOUT_STEPS + 3 + 12 + 4 + 7
                for name in want:
                    assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
                    np.testing.assert_array_equal(got[name].view(np.uint8), want[name].view(np.uint8), err_msg=f"{label} {ids}: {name}")
                # the comparison is about something: actions of several kinds, rollouts that ran, trees that grew
                assert len(np.unique(want["sample_actions(0).type"])) >= 3 and (want["rollout.steps"] > 0).any()
                assert (want["rollout_plan.steps"] > 0).any() and want["choose.tree.count"].max() > 1
                assert_same(snapshot(env), before, f"{label} {ids}: the env's own state")
                assert env.counters == counters
            finally:
                fagent.close()
                fresh.close()
    finally:
        agent.close()
        env.close()
