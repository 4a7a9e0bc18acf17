"""tests/replay_support.py holds what it claims, on the C oracle alone: the scripted roles raise
and finish exactly where they say, the rotation reaches every flag byte at every position of a
group of 4, the fuel tags are distinct in f32, the oracle's sampler handles the whole size x batch
x key table, and the flag patterns peel as test_gpu_replay_edges.py needs them to."""
import numpy as np
import pytest

import replay_support as R

O = pytest.importorskip("oracle.oracle")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    O.build()


def _geometries():
    seen = []
    for g in R.SCALAR + R.WIDE + [R.ODD_CUT, R.ITERS_8, R.ITERS_9] + R.RECORD_FALLBACK:
        if g not in seen:
            seen.append(g)
    return seen


def _variants(n, cap):
    """(auto_reset, max_steps, reset_cut) of every scenario the GPU tests step at (n, cap)."""
    out = [(False, 0, True), (True, 0, True), (True, 2, True)]
    if (n, cap) == R.ODD_CUT:
        out.append((False, 0, False))
    return out


@pytest.mark.parametrize("n,cap", _geometries())
def test_scripted_roles_hold(n, cap):
    steps = R.steps_for(n, cap)
    assert steps * n >= 2 * cap + n  # the ring wraps at least twice
    for auto, max_steps, reset_cut in _variants(n, cap):
        sc = R.scenario(5, n, steps, auto_reset=auto, max_steps=max_steps, reset_cut=reset_cut)
        assert len(sc) == steps
        seen = set()
        for s in sc:
            what = (n, cap, auto, max_steps, s.t)
            np.testing.assert_array_equal(s.err != 0, s.role == R.RAISE, err_msg=f"raise {what}")
            np.testing.assert_array_equal(s.done != 0, s.role == R.FINISH, err_msg=f"finish {what}")
            np.testing.assert_array_equal(s.fuel[s.role == R.FINISH], R.FINISH_FUEL)
            np.testing.assert_array_equal(s.fuel[s.role != R.FINISH], s.tags[s.role != R.FINISH])
            past = s.actions[s.role == R.RAISE]
            assert np.isin(past, [4 + 5 + 250, R.BIG_ACTION]).all()
            seen |= set(s.role.tolist())
            if max_steps == 0:
                np.testing.assert_array_equal(s.cut, s.err != 0)
            else:
                assert (s.cut >= (s.err != 0)).all()
        if n >= 3:
            assert seen == {R.PLAIN, R.FINISH, R.RAISE}, (n, cap, auto, max_steps)
        if max_steps == 2:  # the length cut fires for envs that did not raise, too
            assert any((s.cut & (s.err == 0)).any() for s in sc)
    both = np.concatenate([s.actions[s.role == R.RAISE] for s in sc])
    if len(both) >= 2:
        assert set(both.tolist()) == {4 + 5 + 250, R.BIG_ACTION}


@pytest.mark.parametrize("P", [5, 64])
@pytest.mark.parametrize("n,cap", R.POLICY)
def test_policy_geometries_step_in_both_worlds(P, n, cap):
    """The policy tests take only the fuel from the script (the actions are the policy's); the
    scripted actions still hold their claims in the P = 64 world."""
    for s in R.scenario(P, n, R.steps_for(n, cap), auto_reset=True, max_steps=2):
        np.testing.assert_array_equal(s.err != 0, s.role == R.RAISE)
        np.testing.assert_array_equal(s.done != 0, s.role == R.FINISH)


@pytest.mark.parametrize("P,size", [(5, s) for s in R.SIZES if s] + [(64, s) for s in R.SIZES_P64] + [(254, R.P254_SIZE)])
def test_sampler_rings_hold_their_roles(P, size):
    """The one scripted step that fills a sampler ring, with the script's own roles."""
    (s,) = R.scenario(P, size, 1, auto_reset=False)
    np.testing.assert_array_equal(s.err != 0, s.role == R.RAISE)
    np.testing.assert_array_equal(s.done != 0, s.role == R.FINISH)
    live = s.tags[s.role != R.FINISH].astype(np.float32)
    assert len(np.unique(live)) == len(live)


@pytest.mark.parametrize("n,cap", [g for g in _geometries() if g[0] <= 8])
def test_rotation_reaches_every_flag_byte_at_every_position(n, cap):
    """Up to 8 envs: over the scenario's steps every position j of a group of 4 stores each of
    the flag bytes 0, kRecDone and kRecInvalid."""
    for auto, max_steps, reset_cut in _variants(n, cap):
        sc = R.scenario(5, n, R.steps_for(n, cap), auto_reset=auto, max_steps=max_steps, reset_cut=reset_cut)
        got = {j: set() for j in range(min(n, 4))}
        for s in sc:
            flag = (s.done != 0) * R.REC_DONE + (s.err != 0) * R.REC_INVALID
            np.testing.assert_array_equal(flag, R.FLAG_OF_ROLE[s.role])
            for i in range(n):
                got[i % 4].add(int(flag[i]))
        assert all(v == {0, R.REC_DONE, R.REC_INVALID} for v in got.values()), (n, cap, got)


def test_fuel_tags_are_distinct_in_f32():
    """Any TAG_IDS consecutive transitions (more than the largest ring holds) carry distinct tags
    after the f32 rounding of the stored fuel, none of them the finishing fuel."""
    ids = np.arange(R.TAG_IDS, dtype=np.int64)
    f64 = 10.0 + ids / 256.0
    f32 = f64.astype(np.float32)
    np.testing.assert_array_equal(f32.astype(np.float64), f64)
    assert len(np.unique(f32)) == R.TAG_IDS and (f32 != np.float32(R.FINISH_FUEL)).all()
    for n, cap in _geometries() + R.POLICY:
        assert cap < R.TAG_IDS
        steps = R.steps_for(n, cap)
        all_tags = np.concatenate([R.tags(n, t) for t in range(steps)]).astype(np.float32)
        for hi in range(n, len(all_tags) + 1, n):  # what a ring of cap slots holds after each step
            held = all_tags[max(0, hi - cap):hi]
            assert len(np.unique(held)) == len(held)
    assert max(R.SIZES) < R.TAG_IDS


def test_worlds_are_open_water_with_interior_ports():
    for P in (5, 64, 254):
        w = R.world(P)
        assert len(w.ports) == P == len(set(map(tuple, w.ports)))
        assert w.water().all() and w.water().shape == (w.H, w.W) and max(w.H, w.W) <= 256
        for x, y in w.ports:
            assert 2 <= x <= w.H - 3 and 2 <= y <= w.W - 3
        for a in range(P):
            for b in range(a + 1, min(P, a + 40)):
                assert abs(w.ports[a][0] - w.ports[b][0]) + abs(w.ports[a][1] - w.ports[b][1]) >= 3
        assert min(w.port_fuel) >= 5 and min(w.port_cargo) >= 5
    assert (R.world(254).H, R.world(254).W) == (256, 256)


@pytest.mark.parametrize("size", R.SIZES)
def test_oracle_sampler_handles_the_whole_table(size):
    """No flags: distinct picks, min(size, B) live rows, all -1 from an empty ring."""
    inv = np.zeros(max(size, 1), np.uint8)
    for B in R.batches(size):
        for t in R.KEYS:
            slot = O.replay_pick(size, B, inv, seed=R.SEED, t=t)
            live = slot[slot >= 0]
            assert len(live) == min(size, B), (size, B, t)
            assert len(np.unique(live)) == len(live) and (live < max(size, 1)).all()
            if size == 0:
                assert (slot == -1).all()
            if B >= size:
                np.testing.assert_array_equal(np.sort(live), np.arange(size))
    assert R.batches(0) == [1, 63, 64, 65]
    assert all(b >= 1 for b in R.batches(size))


def _peel_cases():
    out = [(size, size // 4, t) for size in R.SIZES if size >= 4 for t in R.KEYS]
    for size, batch, pattern, _ in R.UPDATE_CASES.values():
        if size and pattern != "none":
            out += [(size, batch, t) for t in R.UPDATE_KEYS]
    return out


@pytest.mark.parametrize("size,B,t", _peel_cases())
def test_flag_patterns_peel(size, B, t):
    """The four peels are disjoint, every row has all four candidates, a fifth pick is all -1,
    and each pattern leaves every row at the try it names."""
    assert 1 <= B and 4 * B <= size
    cand, fifth = R.candidates(O, size, B, t)
    assert cand.shape == (4, B) and (cand >= 0).all() and (cand < size).all()
    assert len(np.unique(cand)) == 4 * B
    assert (fifth == -1).all()
    for pattern in R.PATTERNS:
        flags = R.pattern_flags(O, pattern, size, B, t)
        slot = O.replay_pick(size, B, flags.astype(np.uint8), seed=R.SEED, t=t)
        if pattern == "everything":
            assert flags.all() and (slot == -1).all()
            continue
        depth = R.pattern_depth(pattern, B)
        assert flags.sum() == depth.sum()
        want = np.where(depth < 4, cand[np.minimum(depth, 3), np.arange(B)], -1)
        np.testing.assert_array_equal(slot, want, err_msg=pattern)
        assert not flags[slot[slot >= 0]].any()
    assert set(R.pattern_depth("mixed", B).tolist()) <= {0, 1, 2, 3, 4}


def test_mixed_pattern_reaches_every_depth():
    for size, B in [(1025, 256), (1025, 200), (4096, 1024)]:
        assert set(R.pattern_depth("mixed", B).tolist()) == {0, 1, 2, 3, 4}


def test_update_cases_are_what_they_claim():
    for name, (size, batch, pattern, all_zero) in R.UPDATE_CASES.items():
        flags = R.update_flags(O, name)
        assert len(flags) == size
        tries = set()
        for t in R.UPDATE_KEYS:
            slot = O.replay_pick(size, batch, np.concatenate([flags, [False]]).astype(np.uint8), seed=R.SEED, t=t)
            assert bool((slot == -1).all()) == all_zero, (name, t)
            if size:
                first = O.replay_pick(size, batch, np.zeros(size, np.uint8), seed=R.SEED, t=t)
                tries.add(bool(((first >= 0) & (slot != first)).any()))
            if name == "short_ring":  # every transition once, the rows beyond at weight 0
                assert (slot >= 0).sum() == size < batch and not flags.any()
        if name == "first_tile_of_1":
            assert tries == {True} and batch % 32 == 1  # later tries at every update; a tile of 1 row
        if name == "all4":
            assert flags.all()  # 4 B = size: the four peels are the whole ring
    # the roles that build these rings flag exactly those slots
    for name, (size, _, _, _) in R.UPDATE_CASES.items():
        if size == 0:
            continue
        flags = R.update_flags(O, name)
        (s,) = R.scenario(5, size, 1, auto_reset=True, fixed_roles=R.ring_roles(size, flags))
        np.testing.assert_array_equal(s.err != 0, flags)
        np.testing.assert_array_equal(s.done != 0, ~flags & (np.arange(size) % 2 == 1))


@pytest.mark.parametrize("size", [s for s in R.SIZES if s >= 4])
def test_ring_roles_flag_exactly_the_pattern(size):
    for pattern in ("mixed", "everything", "none"):
        flags = R.pattern_flags(O, pattern, size, size // 4, R.T_LAST)
        (s,) = R.scenario(5, size, 1, auto_reset=False, fixed_roles=R.ring_roles(size, flags))
        np.testing.assert_array_equal(s.err != 0, flags)
        np.testing.assert_array_equal(s.done != 0, ~flags & (np.arange(size) % 2 == 1))
