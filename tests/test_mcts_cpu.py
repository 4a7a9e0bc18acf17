"""The MCTS decision on the CPU: tests/mcts_support.py's restatement of choose_action against
decisions recorded from the reference itself (tests/golden/mcts_golden.json, made by
tests/golden/make_mcts_golden.py), and the claims of the GPU test's hand-made scenarios shown
on the Philox-driver restatement, so that tests/test_gpu_mcts.py cannot pass on scenarios that
never leave the easy path."""
import json
import os
import struct

import pytest

import mcts_support as MS
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "mcts_golden.json")) as _f:
    DECISIONS = json.load(_f)["decisions"]


def bits(v):
    return struct.pack("<d", v)


@pytest.mark.parametrize("rec", DECISIONS, ids=[r["name"] for r in DECISIONS])
def test_restatement_replays_the_reference(rec):
    """Same choices, steps and rollouts in the same order (GoldenDriver raises otherwise), the
    same tree (visits equal, total_reward equal as f64 bits) and the same result."""
    drv = MS.GoldenDriver(rec["events"])
    got = MS.choose_action(MS.ship_from_json(rec["ship"]), len(rec["ports"]), rec["port_cargo"], rec["S"],
                           rec["c"], drv)
    assert drv.at == len(rec["events"]), "the reference went on after the restatement ended"
    assert len(got.nodes) == len(rec["tree"])
    for j, (nd, (parent, action, visits, total)) in enumerate(zip(got.nodes, rec["tree"])):
        assert nd.parent == parent, f"node {j}: parent"
        assert (nd.action is None and action is None) or tuple(action) == nd.action, f"node {j}: action"
        assert nd.visits == visits, f"node {j}: visits"
        assert bits(nd.total) == bits(float.fromhex(total)), f"node {j}: total_reward {nd.total} != {total}"
    if "raise" in rec["result"]:
        assert got.status == MS.RAISED and got.action[0] == MS.SAMPLE_RAISES
    else:
        assert got.status == MS.OK and got.action == tuple(rec["result"]["action"])


def test_golden_covers_the_named_cases():
    by = {r["name"]: r for r in DECISIONS}
    kids = lambda r: {nd[1][0] for nd in r["tree"] if nd[0] == 0}  # noqa: E731
    assert by["fresh_S50"]["S"] == 50 and by["fresh_S3"]["S"] == 3 and len(by["fresh_S50"]["ports"]) == 5
    assert by["fresh_S50"]["max_rollout_steps"] == 100 and abs(by["fresh_S50"]["c"] - 1.4) < 1e-12
    assert by["select_S12"]["ship"][5] == -1 and kids(by["select_S12"]) == {MS.SELECT}
    for name in ("fuel_zero_S2_steps0", "fuel_zero_S9_steps0"):
        r = by[name]
        stock = r["port_cargo"][r["ship"][4]]
        assert float.fromhex(r["ship"][2]) == 0.0 and stock >= 2 and kids(r) == {MS.TAKE_CARGO}
    assert by["fuel_zero_S2_steps0"]["S"] < by["fuel_zero_S2_steps0"]["port_cargo"][1] < by["fuel_zero_S9_steps0"]["S"]
    assert by["fuel_zero_S9_steps100"]["result"] == {"raise": "TypeError"}
    assert any(e[0] == "step" and "raise" in e[2] for e in by["corner_S12"]["events"])
    assert len(by["corner_S12"]["tree"]) - 1 < by["corner_S12"]["S"], "no simulation was skipped"
    assert any(e[0] == "step" and e[2].get("done") for e in by["low_fuel_S12"]["events"])
    assert len(by["one_port"]["ports"]) == 1 and by["one_port"]["result"] == {"raise": "ValueError"}
    assert by["fuel_zero_at_sea_S3"]["events"][-1][0] == "sample"


def test_golden_selection_broke_on_done():
    """Replaying low_fuel_S12 the restatement's selection really breaks on a done step."""
    rec = next(r for r in DECISIONS if r["name"] == "low_fuel_S12")
    got = MS.choose_action(MS.ship_from_json(rec["ship"]), len(rec["ports"]), rec["port_cargo"], rec["S"],
                           rec["c"], MS.GoldenDriver(rec["events"]))
    assert got.broke_on_done > 0


@pytest.mark.parametrize("name", sorted(MS.SCENARIOS))
def test_scenarios_meet_their_claims(oracle_mod, name):
    MS.assert_claims(oracle_mod, name)


def test_scenarios_cover_the_hard_paths(oracle_mod):
    """Across the scenarios: depth >= 2, a raised expansion, a selection broken on done, a root
    wider than S, and every status that can occur. SE_MCTS_NEVER_RETURNS cannot: the sample
    that never returns needs a one-port world and a ship without destination on the port; a
    root without destination either has no possible action (the empty argmax raises first) or
    its first tree step is a SELECT of another port than its origin, which never raises and
    sets the destination for the rest of the simulation, rollout included; and the root
    fallback runs only where every expansion raised, which a SELECT never does."""
    seen = set()
    for name in MS.SCENARIOS:
        seen |= MS.assert_claims(oracle_mod, name)
    assert seen == {MS.OK, MS.CUT, MS.RAISED}
    runs = [d for name in MS.SCENARIOS for S in MS.SIMS for d in MS.decisions(oracle_mod, name, S)]
    assert any(d.depth >= 2 for d in runs)
    assert any(d.expansion_raised for d in runs)
    assert any(d.broke_on_done for d in runs)
    # a selection step that raises (:267) does not occur: whether a step raises depends on the
    # ship's cell, origin and destination being None, and along a path those are the same in
    # every replay (the draws change fuel, cargo and the destination's value only)
    assert not any(d.broke_on_raise for d in runs)
    assert any(d.fallback for d in runs)


def test_restatement_sample_action_is_the_oracles(oracle_mod):
    """The fallback's sample_action restated in mcts_support agrees with the oracle's on the
    category for every scenario ship (the value depends on the word alone)."""
    import numpy as np

    O = oracle_mod
    for name, (world, rows) in MS.SCENARIOS.items():
        ow = world.oracle(O)
        st = O.OracleState(len(rows))
        for i, (_, sh, _) in enumerate(rows):
            st.x[i], st.y[i], st.fuel[i], st.cargo[i], st.origin[i], st.dest[i] = sh
        ty = O.sample_actions(ow, st, seed=1, t=0)[0]
        for i, (label, sh, _) in enumerate(rows):
            got = MS.sample_action(sh, ow, 0x9E3779B9)
            want = {MS.SAMPLE_RAISES: "raised", MS.SAMPLE_NO_OTHER_PORT: "never"}.get(int(ty[i]))
            assert (got == want) if want else (not isinstance(got, str) and got[0] == ty[i]), label
        assert isinstance(ty, np.ndarray)
