"""MCTS with navigator playouts on the CPU: the claims of tests/test_gpu_mcts_nav.py's two scenario
tables shown on the restatement (tests/mcts_nav_support.py), every rep of every actor at every S
of SIMS, so that the GPU test cannot pass on tables that never leave the easy path; and the
restatement tied to its two parts, nav_support.nav_rollout and mcts_support.decide."""
import struct

import pytest

import mcts_nav_support as MN
import mcts_support as MS
import nav_support as NS
import plan_support as PS


def bits(v):
    return struct.pack("<d", v)


def runs(O, name, label):
    return [d for _, d in MN.by_actor(O, name, label)]


def playouts(O, name, label):
    return [p for d in runs(O, name, label) for p in d.playouts]


def test_native_surface_names_the_new_call():
    """The binding, the status and the keyword argument (no device is touched)."""
    import inspect

    from shippingenv_amd import _native as N
    from shippingenv_amd import mcts

    assert "se_mcts_choose_nav" in N.SIGNATURES and len(N.SIGNATURES["se_mcts_choose_nav"]) == 15
    assert (mcts.OK, mcts.CUT, mcts.RAISED, mcts.NEVER_RETURNS, mcts.STUCK) == (0, 1, 2, 3, 4) and MN.STUCK == 4
    assert inspect.signature(mcts.VecMCTSAgent.__init__).parameters["navigator"].default is None


# ----------------------------------------------------------------- status
def test_no_decision_on_the_four_mcts_worlds_is_stuck(oracle_mod):
    for name, (_, rows) in MS.SCENARIOS.items():
        for label, _, _ in rows:
            assert all(d.status != MN.STUCK for d in runs(oracle_mod, name, label)), label


def test_decisions_that_raise(oracle_mod):
    """No possible action at the root: the empty argmax raises before any playout."""
    for name, label in (("one", "one_port"), ("one", "one_port_at_sea"), ("dot", "dot_select")):
        mine = runs(oracle_mod, name, label)
        assert all(d.status == MN.RAISED and d.action == (MS.SAMPLE_RAISES, 0, 0) for d in mine), label
        assert not any(d.playouts for d in mine)


def test_lake_actors_that_are_always_stuck(oracle_mod):
    """From inside the pocket, in the walled-in cell and without a destination in the pocket every
    decision is STUCK and no expansion raises. Every playout there is stuck: at its first position,
    or, where the tree steps left the ship on the pocket's port with an empty hold, at its second,
    after the one TAKE_CARGO the policy asks for there before it looks for the way."""
    take = (MS.TAKE_CARGO, min(MN.LOAD, NS.LAKE.cargo_stock[1]), 0)
    for label in ("from_pocket", "walled_in", "pocket_select"):
        mine = runs(oracle_mod, "lake", label)
        assert all(d.status == MN.STUCK for d in mine), label
        assert not any(d.expansion_raised for d in mine), label
        for p in playouts(oracle_mod, "lake", label):
            assert p.res.status == NS.STUCK and p.nav_status == NS.UNREACHABLE, label
            assert p.stuck_at == 0 or (p.stuck_at == 1 and p.actions == [take]), (label, p.stuck_at, p.actions)
    assert all(p.stuck_at == 0 for p in playouts(oracle_mod, "lake", "walled_in"))
    assert any(p.stuck_at == 1 for p in playouts(oracle_mod, "lake", "pocket_select"))


def test_lake_outside_actors(oracle_mod):
    for label in ("to_pocket", "outside_select"):
        seen = {d.status for d in runs(oracle_mod, "lake", label)}
        assert seen == {MN.OK, MN.STUCK}, (label, seen)
    assert all(d.status == MN.OK for d in runs(oracle_mod, "lake", "outside"))


def test_no_playout_step_raises_and_none_is_cut(oracle_mod):
    seen = set()
    for name, (_, rows) in MN.SCENARIOS.items():
        for label, _ in rows:
            assert sum(p.res.raised for p in playouts(oracle_mod, name, label)) == 0, label
            seen |= {d.status for d in runs(oracle_mod, name, label)}
    assert seen == {MN.OK, MN.RAISED, MN.STUCK}  # CUT cannot occur; NEVER_RETURNS: see test_mcts_cpu


# ----------------------------------------------------------------- what the playouts and trees go through
def test_playouts_end_on_done(oracle_mod):
    for name, label in (("open", "low_fuel"), ("wall", "detour_dry")):
        assert any(p.res.status == PS.DONE for p in playouts(oracle_mod, name, label)), label


def test_playouts_arrive(oracle_mod):
    for name, label in (("open", "select"), ("open", "loaded"), ("open", "next_to_dest"), ("shared", "shared_select"),
                        ("shared", "shared_arrive"), ("many", "wide"), ("many", "many_fresh"), ("wall", "detour"),
                        ("col", "col_select")):
        assert any(p.arrivals for p in playouts(oracle_mod, name, label)), label


def test_expansions_raise(oracle_mod):
    for name, label in (("open", "corner"), ("open", "fuel_zero_at_sea"), ("row", "row_port"), ("row", "row_end"),
                        ("col", "col_port"), ("col", "col_select"), ("lake", "to_pocket"), ("lake", "outside"),
                        ("lake", "outside_select")):
        assert any(d.expansion_raised for d in runs(oracle_mod, name, label)), label


def test_fallback_where_every_expansion_raises(oracle_mod):
    for name, label in (("open", "fuel_zero_at_sea"), ("dot", "dot_home")):
        mine = MN.by_actor(oracle_mod, name, label)
        assert all(d.fallback and d.expansion_raised == S and len(d.nodes) == 1 and not d.playouts
                   for S, d in mine), label
        assert all(d.status == MN.OK for _, d in mine), label


def test_some_tree_is_deep(oracle_mod):
    assert any(d.depth >= 4 for d in runs(oracle_mod, "open", "loaded"))


# ----------------------------------------------------------------- the restatement and its parts
def test_restated_playout_is_nav_rollout(oracle_mod):
    O = oracle_mod
    sh = MS.SCENARIOS["open"][1][6][1]  # loaded
    ret, kind = MN.restated_playout(O, MS.OPEN, sh, seed=MN.SEED, ident=(1 << 33) + 7)
    want = NS.nav_rollout(O, MS.OPEN, sh, MN.MAX_STEPS, MN.REFUEL_BELOW, MN.LOAD, MN.SEED, (1 << 33) + 7)
    assert kind == "ok" and want.res.steps > 0 and bits(ret) == bits(want.res.ret)
    ret, kind = MN.restated_playout(O, NS.LAKE, MN.NAV_SCENARIOS["lake"][1][3][1], seed=MN.SEED, ident=3)
    assert (ret, kind) == (0.0, "stuck")


@pytest.mark.parametrize("name", ["open", "many"])
def test_without_positions_it_is_the_random_decision_without_steps(oracle_mod, name):
    """max_rollout_steps = 0: both playouts return 0.0 and draw nothing, so the two restatements
    build the same tree node for node."""
    O = oracle_mod
    nav = MN.decisions(O, name, 17, max_steps=0)
    rnd = MS.decisions(O, name, 17, max_steps=0, max_attempts=1)
    assert len(nav) == len(rnd) > 64
    for i, (d, w) in enumerate(zip(nav, rnd)):
        assert (d.status, d.action, len(d.nodes)) == (w.status, w.action, len(w.nodes)), i
        for j, (x, y) in enumerate(zip(d.nodes, w.nodes)):
            assert (x.parent, x.action, x.visits, bits(x.total)) == (y.parent, y.action, y.visits, bits(y.total)), (i, j)
