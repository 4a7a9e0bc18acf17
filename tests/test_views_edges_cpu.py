"""The C oracle's observe and valid_mask against what the reference itself gave, without a GPU:
every record of tests/golden/views_edges.npz (tests/golden/make_views_golden.py: P = 1, 2, 3,
several ports on one cell, an empty port, stocks at and past the 49 and 199 amount rows, a
256 x 256 map, an origin of None on a port cell, and fuel at the edges of the f64 -> f32
conversion). orc_observe and orc_valid_mask were written from the same reading of
agents/dqn.py:125-175 and utils/preprocessing.py:25-62 as the kernels of csrc/views.h; this is
what makes them trustworthy as the reference of test_gpu_views_edges.py on this domain."""
import numpy as np
import pytest

import views_edge_support as V


def _cell_mates(name):
    """[n, P] bool: port q stands on the ship's cell, per recorded state."""
    _, px, py, _, _ = V.world(name)
    s = V.states(name)
    return (s["x"][:, None] == px[None, :]) & (s["y"][:, None] == py[None, :])


def test_fixture_reaches_every_class():
    """Read from the fixture's arrays alone; a regeneration that loses one of these fails here."""
    z = V.fixture()
    assert V.worlds() == ("p1", "p2", "p3", "shared", "stocks", "side256")
    for name, P in zip(V.worlds(), (1, 2, 3, 18, 11, 5)):
        assert len(V.world(name)[1]) == P
        assert V.want_bits(name).shape == (len(V.states(name)["x"]), (4 + P + 250 + 7) // 8)
        assert V.meta()["records"][name] == len(V.states(name)["x"])
        on_port = _cell_mates(name).any(axis=1)
        s = V.states(name)
        assert (on_port & (s["origin"] < 0)).any() and (on_port & (s["origin"] >= 0)).any(), name
        assert (~on_port).any() and (s["dest"] < 0).any() and (s["dest"] >= 0).any(), name
    assert sum(V.meta()["records"].values()) > 800

    # a cell of 3 or more ports: origin on that cell, elsewhere, and None
    mates, s = _cell_mates("shared"), V.states("shared")
    crowd = mates.sum(axis=1) >= 3
    assert set(mates.sum(axis=1).tolist()) >= {0, 1, 2, 3, 4}
    rows = np.arange(len(crowd))
    origin_here = (s["origin"] >= 0) & mates[rows, np.maximum(s["origin"], 0)]
    assert (crowd & origin_here).any() and (crowd & (s["origin"] >= 0) & ~origin_here).any()
    assert (crowd & (s["origin"] < 0)).any()
    # on such a cell the origin may be the cell's first port (the one _get_current_port_idx takes) or a later one
    first = mates.argmax(axis=1)
    assert (crowd & origin_here & (s["origin"] == first)).any() and (crowd & origin_here & (s["origin"] != first)).any()

    # both clamps binding, both stocks 0, and each clamp on and one past its row, with a ship on the port
    _, px, py, pf, pc = V.world("stocks")
    mates = _cell_mates("stocks")
    assert (mates.sum(axis=1) <= 1).all()  # distinct cells: the ship's port is unambiguous
    here = np.where(mates.any(axis=1), mates.argmax(axis=1), -1)
    visited = set(here[here >= 0].tolist())
    assert visited == set(range(len(px)))
    assert ((pf > 199) & (pc > 49)).any() and ((pf == 0) & (pc == 0)).any()
    assert set(pc.tolist()) >= {0, 1, 48, 49, 50, 51, 60} and set(pf.tolist()) >= {0, 1, 198, 199, 200, 201, 250}
    # an empty port with a ship on it, in p3 too (not the first port there)
    _, _, _, pf3, pc3 = V.world("p3")
    empty = np.nonzero((pf3 == 0) & (pc3 == 0))[0]
    assert len(empty) == 1 and empty[0] > 0 and _cell_mates("p3")[:, empty[0]].any()

    # bit 255, the last bit of the last byte, set and clear in p2
    b = V.want_bits("p2")
    assert b.shape[1] == 32 and (b[:, 31] & 1).any() and not (b[:, 31] & 1).all()

    # every fuel value of the list, by f64 bit pattern (a NaN by being one), and the int 100
    fuel = np.concatenate([z[f"{w}_fuel"] for w in V.worlds()])
    is_int = np.concatenate([z[f"{w}_fuel_is_int"] for w in V.worlds()])
    for v in V.FUELS:
        want = np.float64(v)
        hit = np.isnan(fuel) if np.isnan(want) else fuel.view(np.int64) == want.view(np.int64)
        assert hit.sum() >= 10, v
    assert (is_int != 0).sum() >= 10 and (fuel[is_int != 0] == 100.0).all()
    assert {int(c) for w in V.worlds() for c in z[f"{w}_cargo"]} == {0, 1, 50}

    # x and y of 255, as ship and as port
    s, (_, px, py, _, _) = V.states("side256"), V.world("side256")
    assert s["x"].max() == 255 == s["y"].max() and px.max() == 255 == py.max()
    assert {(0, 0), (255, 255), (0, 255), (255, 0)} <= set(zip(px.tolist(), py.tolist()))


def test_recorded_rows_put_fuel_in_the_cargo_column():
    """Column 3 is what the reference's own state dict holds there (environment.py:206: "cargo" is
    self.fuel), while the ship's cargo differs from its fuel wherever the fuel is not zero."""
    for name in V.worlds():
        z, s = V.fixture(), V.states(name)
        obs6 = z[f"{name}_obs6"]
        np.testing.assert_array_equal(obs6[:, 3].view(np.int64), s["fuel"].view(np.int64))
        np.testing.assert_array_equal(obs6[:, 2].view(np.int64), s["fuel"].view(np.int64))
        assert ((s["cargo"] != s["fuel"]) | (s["fuel"] == 0)).all() and (s["cargo"] != s["fuel"]).any()
        np.testing.assert_array_equal(obs6[:, [0, 1, 4, 5]], np.stack([s[f] for f in ("x", "y", "origin", "dest")], axis=1))


@pytest.mark.parametrize("name", V.worlds())
def test_oracle_valid_mask_is_the_references(oracle_mod, name):
    O = oracle_mod
    st = V.oracle_state(O, V.states(name))
    got = O.valid_mask(O.OracleWorld(*V.world(name)), st)
    np.testing.assert_array_equal(got, V.want_bits(name), err_msg=name)


@pytest.mark.parametrize("name", V.worlds())
def test_oracle_observe_is_the_references(oracle_mod, name):
    O = oracle_mod
    st = V.oracle_state(O, V.states(name))
    got = O.observe(O.OracleWorld(*V.world(name)), st)
    V.assert_rows_equal(got, V.want_obs(name), name)


def test_reference_bits_follow_the_stock_clamps_and_shared_cells():
    """What the recorded bits say at the classes above, spelled out: amounts 1..min(stock, 49 | 199)
    of the cell's first port; SELECT for every port of the cell but the origin; at sea the moves alone."""
    for name in ("stocks", "shared", "p3", "p1"):
        _, px, py, pf, pc = V.world(name)
        P = len(px)
        bits = np.unpackbits(V.want_bits(name), axis=1)[:, :4 + P + 250]
        mates, s = _cell_mates(name), V.states(name)
        assert bits[:, :4].all()
        for i in range(len(bits)):
            sel = mates[i].copy()
            if s["origin"][i] >= 0:
                sel[s["origin"][i]] = False
            np.testing.assert_array_equal(bits[i, 4:4 + P], sel)
            cur = mates[i].argmax() if mates[i].any() else -1
            nc, nf = (min(pc[cur], 49), min(pf[cur], 199)) if cur >= 0 else (0, 0)
            assert bits[i, 4 + P] == 0 and bits[i, 4 + P + 50] == 0  # amount 0
            assert bits[i, 4 + P:4 + P + 50].sum() == nc == bits[i, 4 + P + 1:4 + P + 1 + nc].sum()
            assert bits[i, 4 + P + 50:].sum() == nf == bits[i, 4 + P + 51:4 + P + 51 + nf].sum()
