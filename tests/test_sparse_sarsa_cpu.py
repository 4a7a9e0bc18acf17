"""The sparse SARSA table's hash and probe rules without a GPU: se_sarsa_sparse_home (host only)
against the restatement of tests/sparse_sarsa_support.py, the restatement's own laws, and the
host-side table builder of shippingenv_amd.sarsa against both."""
import numpy as np
import pytest

import sparse_sarsa_support as SP

LARGEST_ROW = 256 * 256 * 7 * 255 * 255 - 1  # the last row of the 256 x 256 map with 254 ports
ROWS = [0, 1, 1 << 31, 1 << 40, LARGEST_ROW]
CAPACITIES = [64, 1 << 20]


@pytest.fixture(scope="module")
def lib():
    from shippingenv_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def test_mix_is_the_splitmix64_finaliser():
    """Two published outputs of splitmix64 (seed 0: the state after one and two increments of the
    golden gamma, finalised) and the fixed point 0."""
    assert SP.mix(0) == 0
    assert SP.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert SP.mix((2 * 0x9E3779B97F4A7C15) & SP.M64) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("row", ROWS)
def test_home_equals_the_restatement(lib, row, capacity):
    got = lib.se_sarsa_sparse_home(row, capacity)
    assert got == SP.home(row, capacity) and 0 <= got < capacity


def test_home_refuses_what_is_no_table(lib):
    for capacity in (0, 63, 96, -64, 32):
        assert lib.se_sarsa_sparse_home(5, capacity) == -1, capacity
    assert lib.se_sarsa_sparse_home(-1, 64) == -1


def test_the_agents_host_builder_uses_the_same_hash():
    from shippingenv_amd.sarsa import sparse_home, sparse_image

    for capacity in CAPACITIES:
        assert sparse_home(np.array(ROWS), capacity).tolist() == [SP.home(r, capacity) for r in ROWS]
    rng = np.random.default_rng(1)
    rows = rng.choice(10**6, 64, replace=False)
    pages = rng.normal(size=(64, 5))
    keys, out = sparse_image(rows, pages, 64)  # a full table
    assert SP.check_valid(keys, out, 10**6, used=64) == 64
    want = {int(r) * 5 + k: int(pages[i, k].view(np.uint64)) for i, r in enumerate(rows) for k in range(5)}
    assert SP.as_map(keys, out) == want
    with pytest.raises(ValueError):
        sparse_image(np.arange(65), np.zeros((65, 5)), 64)


def rows_with_home(h, capacity, count, start=0):
    out, row = [], start
    while len(out) < count:
        if SP.home(row, capacity) == h:
            out.append(row)
        row += 1
    return out


def test_insert_then_lookup():
    t = SP.Table(64, 3)
    rows = [7, 1 << 40, LARGEST_ROW, 0]
    for k, row in enumerate(rows):
        assert t.find(row) == -1 and t.get(row, 1) == 0.0  # absent: a row of zeros
        assert t.set(row, 1, 1.5 + k)
    assert t.used == 4
    for k, row in enumerate(rows):
        s = t.find(row)
        assert s >= 0 and t.keys[s] == row and t.get(row, 1) == 1.5 + k and t.get(row, 0) == 0.0
        assert t.find_or_insert(row) == s  # found, not inserted again
    assert t.used == 4 and t.find(8) == -1
    assert SP.check_valid(t.keys, t.pages, 1 << 41, used=4) == 4
    assert SP.as_map(t.keys, t.pages) == {row * 3 + 1: int(np.float64(1.5 + k).view(np.uint64)) for k, row in enumerate(rows)}


def test_a_chain_wraps_from_the_last_bucket():
    cap = 64
    last, before = rows_with_home(cap - 1, cap, 3), rows_with_home(cap - 2, cap, 2)
    t = SP.Table(cap, 2)
    slots = [t.find_or_insert(r) for r in before + last]
    assert slots == [cap - 2, cap - 1, 0, 1, 2]  # the second of `before` took the last bucket, the rest wrapped
    assert [t.find(r) for r in before + last] == slots
    SP.check_valid(t.keys, t.pages, 1 << 40, used=5)
    # a row whose home is slot 0 lies behind the wrapped chain
    zero = rows_with_home(0, cap, 1)[0]
    assert t.find(zero) == -1 and t.find_or_insert(zero) == 3
    # the validity check sees a key cut off from its home by an empty slot
    t.keys[0] = SP.EMPTY
    with pytest.raises(AssertionError, match="behind the empty slot"):
        SP.check_valid(t.keys, t.pages, 1 << 40)


def test_a_full_table_ends_the_probe():
    t = SP.Table(64, 2)
    for row in range(64):
        assert t.set(row, 0, 1.0 + row)
    assert t.used == 64 and (t.keys != SP.EMPTY).all()
    assert t.find(1000) == -1 and t.find_or_insert(1000) == -1 and not t.set(1000, 0, 9.0)  # bounded, no room
    assert t.get(1000, 0) == 0.0 and t.used == 64
    assert all(t.get(row, 0) == 1.0 + row for row in range(64))  # every held row is still found
    SP.check_valid(t.keys, t.pages, 64, used=64)
    with pytest.raises(AssertionError):  # 1000 is no row of a 64-row layout
        t.keys[t.find(5)] = 1000
        SP.check_valid(t.keys, t.pages, 64)


def test_the_validity_check_names_each_damage():
    t = SP.from_dense(np.arange(40.0), 4, 64)  # rows 0..9, row 0 holds 0.0 in slot 0 only
    assert SP.check_valid(t.keys, t.pages, 10, used=10) == 10
    assert SP.as_map(t.keys, t.pages) == SP.dense_map(np.arange(40.0))
    twice = t.keys.copy()
    twice[np.flatnonzero(twice == SP.EMPTY)[0]] = 3
    with pytest.raises(AssertionError):
        SP.check_valid(twice, t.pages, 10)
    stray = t.pages.copy()
    stray[np.flatnonzero(t.keys == SP.EMPTY)[0], 1] = -0.0  # a non-zero word on a page without a key
    with pytest.raises(AssertionError, match="without a key"):
        SP.check_valid(t.keys, stray, 10)
    with pytest.raises(AssertionError, match="used"):
        SP.check_valid(t.keys, t.pages, 10, used=9)
