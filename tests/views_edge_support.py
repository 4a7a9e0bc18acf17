"""The views fixture (tests/golden/views_edges.npz, recorded from the reference's
preprocess_state and DQNAgent.is_valid_action by tests/golden/make_views_golden.py) as the tests
read it: the worlds, each world's states, the rows and bits the reference gave, and the rule the
rows are compared by. Shared by test_views_edges_cpu.py and test_gpu_views_edges.py. numpy only.
"""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN, golden_water, load_golden

STATE = ("x", "y", "fuel", "cargo", "origin", "dest")
# the fuel values every regeneration must record (make_views_golden.py FUELS), as f64 bit patterns
FUELS = (100.0, 0.1, 99.9999, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 16777217.0, 1e-46, 1e-39,
         3.4028235677973366e38, 1e39, -0.0, -3.5, float("inf"), float("nan"))


@functools.lru_cache(maxsize=None)
def fixture():
    z = load_golden(os.path.join(GOLDEN, "views_edges.npz"))
    for v in z.values():
        v.setflags(write=False)
    return z


def meta():
    with open(os.path.join(GOLDEN, "views_edges_meta.json")) as f:
        return json.load(f)


def worlds():
    return tuple(meta()["worlds"])


def world(name):
    """(water, port_x, port_y, port_fuel, port_cargo) of a world; the golden map unless it has its own."""
    z = fixture()
    water = z[f"{name}_water"] if f"{name}_water" in z else golden_water()
    return (water,) + tuple(z[f"{name}_port_{k}"] for k in ("x", "y", "fuel", "cargo"))


def states(name, sel=None):
    """{field: column} of the world's recorded states (origin / dest -1 for None)."""
    z = fixture()
    sel = slice(None) if sel is None else sel
    return {f: z[f"{name}_{f}"][sel] for f in STATE}


def want_obs(name, sel=None):
    """The reference's rows as the kernels must write them: astype(float32) of the f64 record."""
    z = fixture()
    obs6 = z[f"{name}_obs6"]
    rows = np.concatenate([obs6, np.broadcast_to(z[f"{name}_port_block"], (len(obs6), len(z[f"{name}_port_block"])))],
                          axis=1)
    with np.errstate(over="ignore"):  # 3.4028235677973366e38 and 1e39 round to inf: recorded on purpose
        rows = rows.astype(np.float32)
    return rows if sel is None else rows[sel]


def want_bits(name, sel=None):
    b = fixture()[f"{name}_bits"]
    return b if sel is None else b[sel]


def ragged(n):
    """Record indices for a batch of the world's n records, padded by repeats off a multiple of 256."""
    idx = np.arange(n)
    return idx if n % 256 else np.concatenate([idx, idx[:3]])


def assert_rows_equal(got, want, what):
    """f32 rows equal as uint32 bit patterns (so -0.0 and inf count); a NaN need only be a NaN."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(np.where(nan, 0, got.view(np.uint32)), np.where(nan, 0, want.view(np.uint32)),
                                  err_msg=f"{what}: f32 bit patterns")


def oracle_state(O, cols):
    """An OracleState holding the columns of states() (or any dict of the six fields)."""
    st = O.OracleState(len(cols["x"]))
    for f in STATE:
        getattr(st, f)[:] = cols[f]
    return st


def ntmpl(px, py):
    """se_valid_mask's template count: 1 + P + the sum over cells of (ports on the cell)^2."""
    cells = {}
    for c in zip(np.asarray(px).tolist(), np.asarray(py).tolist()):
        cells[c] = cells.get(c, 0) + 1
    return 1 + len(px) + sum(k * k for k in cells.values())


def mask_tb(S):
    """csrc/views.h mask_tb: a template block's bytes (16 zero bytes, the row, zeros to a 16-byte end)."""
    return (S + 35 + 15) & ~15
