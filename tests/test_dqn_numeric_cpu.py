"""The yardsticks of tests/test_gpu_dqn_numeric.py, on the references alone (no GPU).

Every family of tests/dqn_numeric_support.py has the property that defines it, on the oracle's
observation rows of the worlds and ships the GPU file plays; every cap the GPU file holds the
kernels to is met, with room, by the references themselves (so a family that cannot meet a cap is
found here); _Ref64 gives exactly zero gradient on a silent unit's rows and columns; the float64
Adam direction is finite at every step count of the Adam cases; and the error that an f32
evaluation of Adam's bias corrections may carry is recorded per step count (the GPU bound uses it).
"""
import numpy as np
import pytest

import dqn_numeric_support as S

torch = pytest.importorskip("torch")

WORLD_NAMES = ("default", "clamp")


def _hidden64(model, obs):
    sd = {k: v.double() for k, v in model.state_dict().items()}
    z1 = obs.double() @ sd["fc1.weight"].T + sd["fc1.bias"]
    z2 = torch.relu(z1) @ sd["fc2.weight"].T + sd["fc2.bias"]
    return z1, z2


def test_fuel_edges_are_edges():
    f32, hi, lo = S.fuel_facts()
    F = S.FUELS
    assert np.signbit(f32[1]) and f32[1] == 0 and f32[2] < 0
    assert F[6] < 256 and hi[6] == 256.0 and lo[6] < 0  # hi rounds up across the binade, lo is negative
    assert hi[7] == 256.0 and lo[7] == -(2.0 ** -9) and hi[7] + lo[7] == f32[7]
    # past 2^16 the two parts are 17 binary places apart: 65536.5 has one bit in each and still
    # splits exactly; 1e6 + 0.3 does not (hi + lo no longer holds the f32)
    assert float(hi[8]) + float(lo[8]) == float(f32[8]) and lo[8] == 0.5
    assert float(hi[9]) + float(lo[9]) != float(f32[9])
    assert np.isfinite(hi[10]) and np.isfinite(lo[10]) and f32[10] > 2.0 ** 127
    assert 0 < f32[11] < 2.0 ** -126  # an f32 subnormal
    assert f32[12] == np.float32(100.0) and np.float32(S._TIE100 + 2.0 ** -30) > np.float32(100.0)
    assert f32[3] == 2.0 ** -30 and hi[3] == f32[3] and lo[3] == 0
    for world in WORLD_NAMES:
        r = S.refs(world)
        assert len(set(r.fuel_idx.tolist())) == len(F)
        # the oracle's observation holds the fuel as torch's .float() does, in columns 2 and 3
        np.testing.assert_array_equal(r.obs_edges[:, 2].numpy().view(np.int32), f32[r.fuel_idx].view(np.int32))
        np.testing.assert_array_equal(r.obs_edges[:, 3].numpy().view(np.int32), f32[r.fuel_idx].view(np.int32))


def test_worlds_are_the_tile_classes_of_the_issue():
    from test_gpu_dqn_shapes import compact_class, full_class

    d, c = S.refs("default"), S.refs("clamp")
    assert compact_class(d.P, d.port_fuel, d.port_cargo)[1] == 2 and full_class(d.P)[1] == 9
    assert c.P == 34 and compact_class(c.P, c.port_fuel, c.port_cargo)[1] == 9


@pytest.mark.parametrize("world", WORLD_NAMES)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_family_has_its_property(family, world):
    r = S.refs(world)
    for spread in (1.0, S.SPREAD):
        m = S.make_family(family, r.obs_size, r.A, spread=spread)
        z1, z2 = _hidden64(m, r.obs_typical)
        q = S._q64(m, r.obs_typical)
        assert bool(torch.isfinite(q).all())
        if family == "trained_scale":
            firing = z1[z1 > 0]
            print(f"{world} spread {spread}: median firing h1 {float(firing.median()):.4g}, max |Q| {float(q.abs().max()):.4g}")
            assert float(firing.median()) >= 1e2 and 1e3 <= float(q.abs().max()) <= 1e5
        elif family == "mixed_rows":
            d = S.make_family("default", r.obs_size, r.A, spread=spread)
            for a, b in zip(m.parameters(), d.parameters()):
                ratio = (a.detach().reshape(a.shape[0], -1)[:, 0] / b.detach().reshape(b.shape[0], -1)[:, 0]).abs()
                k = torch.log2(ratio)
                assert bool((k == k.round()).all()) and -12 <= float(k.min()) and float(k.max()) <= 6
                assert float(k.max()) - float(k.min()) >= 12  # large and small rows in one layer
            signs = torch.sign(m.fc2.bias.detach() / d.fc2.bias.detach())
            assert 0.25 < float((signs < 0).float().mean()) < 0.75
        elif family == "dead_units":
            dead1, dead2, zero2 = S.dead_sets()
            assert len(dead1) == len(dead2) == 64 and len(zero2) >= 4
            assert bool((z1[:, dead1] < 0).all()) and bool((z2[:, dead2] < 0).all())
            assert bool((z2[:, zero2] == 0).all()) and not bool(torch.signbit(z2[:, zero2]).any())
            live1 = np.setdiff1d(np.arange(128), dead1)
            assert bool((z1[:, live1] > 0).any())
        elif family == "near_tie":
            w, b = m.fc3.weight.detach().numpy(), m.fc3.bias.detach().numpy()
            n2 = r.A // 2 * 2
            np.testing.assert_array_equal(w[1:n2:2].view(np.int32), w[0:n2:2].view(np.int32))
            np.testing.assert_array_equal(b[1:n2:2].view(np.int32), b[0:n2:2].view(np.int32))
            both = r.valid[:, 0:n2:2] & r.valid[:, 1:n2:2]
            one = r.valid[:, 0:n2:2] ^ r.valid[:, 1:n2:2]
            assert both.any(1).all() and one.any()  # ties between two valid rows and half-valid pairs


@pytest.mark.parametrize("world", WORLD_NAMES)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_caps_hold_on_the_references(family, world):
    """What the GPU file asserts of the kernels, asserted of the references: the non-finite rows
    are the 3.0e38 ships' only; per fuel class the two emulations lie within half of each bar of
    each other (the bar is at least twice their distance by construction: shown is that it is not
    vacuous, below 5e-2 of max |Q|); torch fp32 meets the hard cap of the fp32 mode with the
    rule's own factor (2 err_t + 2 ulp <= cap); and at most 10 % of the envs have a top-2 gap
    inside twice the references' disagreement."""
    p = S.policy_refs(world, family)
    r = p.r
    for ok in (p.ok16, p.ok32):
        bad = set(r.fuel_idx[~ok.numpy()].tolist())
        assert bad <= {10}, bad  # only 3.0e38 leaves the range; the subnormal's rows are finite
    print(f"{world} {family}: finite rows bf16 {int(p.ok16.sum())} f32 {int(p.ok32.sum())} of {S.N_ENVS}")
    for cls in S.FUEL_CLASSES:
        rows = S.class_rows(r, cls, p.ok16)
        if bool(rows.any()):
            mean_bar, worst_bar, dist = p.bars16(rows)
            print(f"  bf16 {cls}: emulations' distance mean {dist[0]:.3g} worst {dist[1]:.3g} -> bars {mean_bar:.3g} {worst_bar:.3g}")
            assert worst_bar <= 5e-2 and mean_bar <= 5e-2
        rows = S.class_rows(r, cls, p.ok32)
        if bool(rows.any()):
            err_t, scale, cap = p.cap32(rows)
            print(f"  f32 {cls}: torch fp32 error {err_t:.3g} of max |Q| {scale:.3g} = {err_t / scale:.3g}, cap {cap:.3g}")
            if family in ("default", "trained_scale"):
                assert 2 * err_t + 2 * scale * 2.0 ** -24 <= cap * scale
            assert cap <= 1e-4
    pairs = family == "near_tie"
    for mode, ref, other, ok in (("bf16", p.qe, p.qp, p.ok16), ("f32", p.q64, p.q32, p.ok32)):
        okn = ok.numpy()
        gap = S.top2_gap(ref.numpy(), r.valid, pairs)[okn]
        delta = (ref - other).abs().max(1).values.numpy()[okn]
        under = float((gap <= 2 * 2 * delta).mean())
        print(f"  {mode}: {under:.3f} of the envs have a top-2 gap within twice the references' disagreement")
        assert under <= 0.10


def test_ref64_gives_zero_gradient_on_silent_units():
    """_Ref64 on dead_units: the gradient is exactly zero on a silent unit's own row and bias and
    on the column that reads it (torch's ReLU gradient at 0 is 0), and not zero elsewhere."""
    r = S.refs("default")
    model = S.make_family("dead_units", r.obs_size, r.A)
    target = S.make_family("trained_scale", r.obs_size, r.A, seed=8)
    b = S.HostBatch(r, 33, S.update_actions(r.A))
    ref = S._Ref64(model, target, b.weighted(), 0.95, 1e-3, 0)
    masks = S.dead_masks(model)
    for g, mask, name in zip(ref.g, masks, ("w1", "b1", "w2", "b2", "w3", "b3")):
        assert bool((g[mask] == 0).all()), name
        if name != "b3":
            assert bool(mask.any()) and bool((g[~mask] != 0).any()), name
    for p0, p1, mask in zip(ref.p0, ref.p, masks):  # and Adam leaves them where they are
        assert bool((p0[mask] == p1[mask]).all())


# (steps taken, the relative error an f32 evaluation may carry in 1 / (1 - b1^t), in sqrt(1 - b2^t))
BIAS_CORRECTION_ERRORS = {
    0: (1.44e-6, 6.62e-5), 999: (1.2e-7, 3.91e-6), 10 ** 5: (1.2e-7, 1.2e-7), 2 ** 24 + 1: (1.2e-7, 1.2e-7),
    2 ** 31 - 2: (1.2e-7, 1.2e-7)}


@pytest.mark.parametrize("steps", S.ADAM_STEPS)
def test_adam_direction_is_finite_and_the_f32_bias_correction_error_is_recorded(steps):
    e1, e2 = S.bias_correction_error(steps)
    print(f"steps {steps}: f32 bias-correction error {e1:.3g} (1 - b1^t), {e2:.3g} (sqrt(1 - b2^t))")
    r1, r2 = BIAS_CORRECTION_ERRORS[steps]
    assert r1 / 1.2 <= e1 <= r1 and r2 / 1.2 <= e2 <= r2, (e1, e2)
    r = S.refs("default")
    model = S.make_family("trained_scale", r.obs_size, r.A)
    target = S.make_family("default", r.obs_size, r.A, seed=8)
    b = S.HostBatch(r, 33, S.update_actions(r.A))
    g = S._Ref64(model, target, b.weighted(), 0.95, 1e-3, 0).g
    for kind in S.ADAM_MOMENTS if steps else ("zero",):
        m0, v0 = S.adam_moments(kind, g)
        ref = S.RefAdam(model, target, b.weighted(), 0.95, 1e-3, steps, m0, v0)
        for i in range(6):
            d = ref._direction(i, ref.g[i])
            assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(ref.p[i]).all()), (kind, i)
            assert bool(torch.isfinite(ref.param_bound(i)).all())
