"""Parity of the HIP path (through the C-ABI) with the reference and the oracle.

* replay: every golden record (the reference's own steps, resets and errors)
  through se_step_replay / se_reset_to -> bit-exact state, reward == f32(ref),
  done, err;
* Philox: the kernel and the oracle on the same seed and actions, bit-exact
  (config 2 move-only, config 3 mix, config 4 auto-reset with 64 ports);
* full size (N = 2^20): invariants plus a sampled exact check per env id.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_files, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "fuel", "cargo", "origin", "dest")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from shippingenv_amd import build

    build.build(verbose=False)


def VecEnv(*a, **k):
    from shippingenv_amd.vec import VecEnv as V

    return V(*a, **k)


def set_state(env, z, sel, prefix="pre_"):
    for f in FIELDS:
        v = z[prefix + f][sel]
        if f in ("origin", "dest"):
            v = np.where(v < 0, 255, v)
        t = getattr(env, f)
        t.copy_(torch.from_numpy(np.ascontiguousarray(v).astype(t.cpu().numpy().dtype)))


def get_state(env):
    torch.cuda.synchronize()
    out = {}
    for f in FIELDS:
        v = getattr(env, f).cpu().numpy()
        if f in ("origin", "dest"):
            v = np.where(v == 255, -1, v.astype(np.int32))
        elif f != "fuel":
            v = v.astype(np.int32)
        out[f] = v
    return out


def assert_state(got, want, what):
    for f in FIELDS:
        if f == "fuel":
            np.testing.assert_array_equal(got[f].view(np.int64), np.asarray(want[f]).view(np.int64),
                                          err_msg=f"{what}: fuel bits")
        else:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")


def tape_of(z, sel):
    from shippingenv_amd.vec import TAPE_DTYPE

    tape = np.zeros(len(sel), TAPE_DTYPE)
    for f in ("u_fuel", "u_gate", "u_type", "beta", "arrive_dest"):
        tape[f] = z[f][sel]
    return tape


def env_for(z, n, water, with_ports=True, **kw):
    sl = slice(None) if with_ports else slice(0, 0)
    ports = [[int(a), int(b)] for a, b in zip(z["port_x"][sl], z["port_y"][sl])]
    return VecEnv(n, water=water, ports=ports, port_fuel=z["port_fuel"][sl],
                  port_cargo=z["port_cargo"][sl], **kw)


# ---------------------------------------------------------------- replay parity
@pytest.mark.parametrize("path", golden_files(), ids=os.path.basename)
def test_replay_matches_reference(path, water):
    z = load_golden(path)
    for kind, with_ports in ((0, True), (2, False)):
        sel = np.nonzero(z["kind"] == kind)[0]
        if not len(sel):
            continue
        env = env_for(z, len(sel), water, with_ports)
        set_state(env, z, sel)
        reward, done, err = env.step_replay(z["act_type"][sel], z["act_a"][sel], z["act_b"][sel],
                                            tape_of(z, sel))
        got = get_state(env)
        want = {f: z["post_" + f][sel] for f in FIELDS}
        assert_state(got, want, os.path.basename(path))
        np.testing.assert_array_equal(reward.cpu().numpy(), z["reward"][sel].astype(np.float32))
        np.testing.assert_array_equal(done.cpu().numpy().astype(np.int32), z["done"][sel])
        np.testing.assert_array_equal(err.cpu().numpy().astype(np.int32), z["err"][sel])
        # the north-star tolerance, stated: reward within 1e-6 (relative) of the f64 value
        np.testing.assert_allclose(reward.cpu().numpy().astype(np.float64), z["reward"][sel],
                                   rtol=1e-6, atol=1e-6)
        env.close()


def _reference_decode(P):
    """index -> (type, a, b) | None from the reference's own map_action_to_env_action
    (tests/golden/decode_golden.json, made by make_decode_golden.py)."""
    import json

    with open(os.path.join(GOLDEN, "decode_golden.json")) as f:
        rows = json.load(f)["P"][str(P)]["rows"]
    return {r[0]: (None if r[1] == "IndexError" else tuple(r[1:])) for r in rows}


@pytest.mark.parametrize("path", golden_files(), ids=os.path.basename)
def test_agent_path_replays_reference_records(path, water):
    """The bench-timed agent-path kernel (step_group_agent, in its replay-tape
    instantiation: se_step_agent_replay) on every golden step record whose typed action
    the reference's decode produces: the record's action becomes the agent index the
    reference maps to it (decode_golden.json), the variates come from the tape, and the
    post-state, reward, done and error class must equal the reference's, bit for bit."""
    z = load_golden(path)
    P = len(z["port_x"])
    inv = {}
    for i, v in sorted(_reference_decode(P).items(), key=lambda kv: (kv[0] < 0, kv[0])):
        if v is not None:
            inv.setdefault(v, i)
    idx = np.array([inv.get((int(t), int(a), int(b) if int(t) == 1 else 0), -1)
                    for t, a, b in zip(z["act_type"], z["act_a"], z["act_b"])], np.int32)
    sel = np.nonzero((z["kind"] == 0) & (idx >= 0))[0]
    assert len(sel) > 1000
    env = env_for(z, len(sel), water)
    set_state(env, z, sel)
    reward, done, err, tape = env.step_agent_replay(idx[sel], tape_of(z, sel))
    got = get_state(env)
    want = {f: z["post_" + f][sel] for f in FIELDS}
    assert_state(got, want, os.path.basename(path) + " (agent path)")
    np.testing.assert_array_equal(reward.cpu().numpy(), z["reward"][sel].astype(np.float32))
    np.testing.assert_array_equal(done.cpu().numpy().astype(np.int32), z["done"][sel])
    np.testing.assert_array_equal(err.cpu().numpy().astype(np.int32), z["err"][sel])
    env.close()
    # the draws the kernel reports consumed are the typed replay's (the drop-in's protocol;
    # the host build of that replay is pinned to the kernel in test_compat_gpu.py)
    from shippingenv_amd.shipping._host import host_step_replay

    st = {f: (np.where(z["pre_" + f][sel] < 0, 255, z["pre_" + f][sel]) if f in ("origin", "dest")
              else z["pre_" + f][sel]) for f in FIELDS}
    h = host_step_replay(water, z["port_x"], z["port_y"], z["port_fuel"], z["port_cargo"], st,
                         z["act_type"][sel], z["act_a"][sel], z["act_b"][sel], tape_of(z, sel))
    np.testing.assert_array_equal(tape["used"], h["tape"]["used"])


@pytest.mark.parametrize("P", [5, 64])
def test_agent_path_decodes_every_index_as_the_reference(P, water):
    """Every agent index the reference decoded (decode_golden.json, -6 .. A + 2) stepped
    through the agent-path kernel equals the reference's typed action stepped through the
    typed replay kernel, from the same states and draws; indices below -4 raise in the
    reference (SE_ERR_BAD_INDEX, state untouched)."""
    table = _reference_decode(P)
    idx = np.array(sorted(table), np.int32)
    reps = 8
    acts = np.tile(idx, reps)
    n = len(acts) // 4 * 4 + 4
    acts = np.concatenate([acts, np.zeros(n - len(acts), np.int32)])
    rng = np.random.default_rng(P)
    if P == 5:
        ports = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]]
    else:
        from shippingenv_amd.vec import random_water_ports

        ports = random_water_ports(water, 64, seed=3)
    mk = lambda: VecEnv(n, water=water, ports=ports, seed=5)  # noqa: E731
    a, b = mk(), mk()
    for e in (a, b):
        e.reset()
    # states: half the envs at their origin port (TAKE / SELECT valid), half moved away
    moves = torch.from_numpy(rng.integers(0, 4, n).astype(np.int32)).cuda()
    keep = torch.from_numpy((np.arange(n) % 2 == 0).astype(np.uint8)).cuda()
    cargo = torch.from_numpy(rng.integers(0, 60, n).astype(np.int32)).cuda()
    for e in (a, b):
        e.step(torch.where(keep.bool(), torch.full_like(moves, 4 + 0), moves))
        e.cargo.copy_(cargo)
    typ = np.zeros(n, np.int32)
    va = np.zeros(n, np.int32)
    vb = np.zeros(n, np.int32)
    for k, i in enumerate(acts):
        v = table.get(int(i))
        if v is None:
            typ[k] = 99  # an unknown category: raises with no draw, like the index error
        else:
            typ[k], va[k], vb[k] = v
    from shippingenv_amd.vec import TAPE_DTYPE

    tape = np.zeros(n, TAPE_DTYPE)
    tape["u_fuel"], tape["u_gate"] = rng.random(n), rng.random(n)
    tape["u_type"], tape["beta"] = rng.random(n), rng.random(n)
    tape["arrive_dest"] = rng.integers(0, P, n)
    ra, da, ea, _ = a.step_agent_replay(acts, tape)
    rb, db, eb = b.step_replay(typ, va, vb, tape)
    torch.cuda.synchronize()
    ea, eb = ea.cpu().numpy(), eb.cpu().numpy()
    bad = np.array([table.get(int(i)) is None for i in acts])
    assert (ea[bad] == 9).all() and (eb[bad] == 7).all()
    np.testing.assert_array_equal(ea[~bad], eb[~bad])
    sa, sb = get_state(a), get_state(b)
    for f in FIELDS:
        np.testing.assert_array_equal(np.asarray(sa[f]).view(np.uint8), np.asarray(sb[f]).view(np.uint8), err_msg=f)
    np.testing.assert_array_equal(ra.cpu().numpy(), rb.cpu().numpy())
    np.testing.assert_array_equal(da.cpu().numpy(), db.cpu().numpy())
    assert (eb[~bad] == 0).sum() > 100  # moves, selects and in-stock takes step
    a.close()
    b.close()


@pytest.mark.parametrize("path", golden_files("tape"), ids=os.path.basename)
def test_replay_resets_match_reference(path, water):
    z = load_golden(path)
    sel = np.nonzero(z["kind"] == 1)[0]
    env = env_for(z, len(sel), water)
    env.reset_to(z["reset_origin"][sel], z["reset_dest"][sel])
    assert_state(get_state(env), {f: z["post_" + f][sel] for f in FIELDS}, "reset")
    env.close()


@pytest.mark.parametrize("path", golden_files("tape")[:3], ids=os.path.basename)
def test_replay_episode_chain_n1(path, water):
    """One env walks the whole recorded trajectory from its own outputs (N = 1:
    the scalar tail path of the kernel)."""
    z = load_golden(path)
    env = env_for(z, 1, water)
    tapes = tape_of(z, np.arange(len(z["kind"])))
    for i in range(len(z["kind"])):
        if z["kind"][i] == 1:
            env.reset_to(z["reset_origin"][i:i + 1], z["reset_dest"][i:i + 1])
        else:
            r, d, e = env.step_replay(z["act_type"][i:i + 1], z["act_a"][i:i + 1],
                                      z["act_b"][i:i + 1], tapes[i:i + 1])
            assert int(e.item()) == z["err"][i] and int(d.item()) == z["done"][i], i
            assert r.item() == np.float32(z["reward"][i]), i
        if i % 97 == 0 or i == len(z["kind"]) - 1:
            assert_state(get_state(env), {f: z["post_" + f][i:i + 1] for f in FIELDS}, f"rec {i}")
    env.close()


# ---------------------------------------------------------------- Philox parity vs oracle
def _oracle_pair(O, env):
    world = O.OracleWorld(env.water, env.port_x, env.port_y, env.port_fuel, env.port_cargo)
    st = O.OracleState(env.n)
    return world, st


def _assert_vs_oracle(env, st, what):
    got = get_state(env)
    want = {f: getattr(st, f) for f in FIELDS}
    assert_state(got, want, what)


@pytest.mark.parametrize("n", [4096, 4099])
def test_config2_move_only_vs_oracle(oracle_mod, n):
    """Config 2: N=4096, move-only actions, 1000 steps, bit-exact x, y, fuel bits,
    cargo, done (and reward == f32 of the oracle's f64) on every step."""
    O = oracle_mod
    seed = 1234
    env = VecEnv(n, seed=seed)
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    _assert_vs_oracle(env, st, "reset")
    rng = np.random.default_rng(0)
    for t in range(1000):
        acts = rng.integers(0, 4, size=n).astype(np.int32)
        r, d, e = env.step(acts)
        O.step(world, st, actions=acts, seed=seed, t=t)
        if t % 50 == 0 or t == 999:
            _assert_vs_oracle(env, st, f"t={t}")
        np.testing.assert_array_equal(r.cpu().numpy(), st.reward.astype(np.float32))
        np.testing.assert_array_equal(d.cpu().numpy().astype(np.int32), st.done)
        np.testing.assert_array_equal(e.cpu().numpy().astype(np.int32), st.err)
    assert st.done.sum() > 0  # fuel ran out somewhere
    env.close()


@pytest.mark.parametrize("blocks,nt", [(None, None), ("3", None), (None, "0")])
def test_config3_full_mix_vs_oracle(oracle_mod, monkeypatch, blocks, nt):
    if blocks:  # several groups per thread, partial last workgroup
        monkeypatch.setenv("SHIPENV_STEP_BLOCKS", blocks)
    if nt:  # the kernel variant with temporal loads (the default above 2^23 envs)
        monkeypatch.setenv("SHIPENV_NT_LOADS", nt)
    O = oracle_mod
    seed, n = 77, 8192
    env = VecEnv(n, seed=seed)
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    seen_err = set()
    for t in range(400):
        acts = env.gen_actions(t)
        ref = O.gen_actions(n, env.P, seed, 0, t)
        np.testing.assert_array_equal(acts.cpu().numpy(), ref)
        r, d, e = env.step(acts)
        O.step(world, st, actions=ref, seed=seed, t=t)
        np.testing.assert_array_equal(r.cpu().numpy(), st.reward.astype(np.float32))
        np.testing.assert_array_equal(e.cpu().numpy().astype(np.int32), st.err)
        seen_err |= set(np.unique(st.err).tolist())
        if t % 40 == 0:
            _assert_vs_oracle(env, st, f"t={t}")
    _assert_vs_oracle(env, st, "end")
    assert {0, 2, 4, 5}.issubset(seen_err)
    env.close()


@pytest.mark.parametrize("n,blocks,nt,pad", [(8192, None, None, None), (8195, "3", None, None),
                                             (8192, None, "1", None), (8195, "3", None, "1")])
def test_config4_autoreset_64_ports_vs_oracle(oracle_mod, water, monkeypatch, n, blocks, nt, pad):
    """blocks="3": 3 workgroups, several groups per thread (double-buffered loads),
    a partial last workgroup and a tail group appended to its done segment. nt="1": the
    variant with nontemporal loads (off by default with auto-reset). pad="1": the done
    list's records padded to whole lines (the form beyond 2^23 envs, forced)."""
    from shippingenv_amd.vec import random_water_ports

    if pad:
        monkeypatch.setenv("SHIPENV_DONE_PAD", pad)

    if blocks:
        monkeypatch.setenv("SHIPENV_STEP_BLOCKS", blocks)
    if nt:
        monkeypatch.setenv("SHIPENV_NT_LOADS", nt)
    O = oracle_mod
    seed = 4242
    ports = random_water_ports(water, 64, seed=3)
    env = VecEnv(n, seed=seed, ports=ports, auto_reset=True)
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    stats = np.zeros(3)
    total_done = 0
    for t in range(600):
        acts = env.gen_actions(t)
        ref = O.gen_actions(n, env.P, seed, 0, t)
        env.step(acts)
        O.step_autoreset(world, st, ref, seed=seed, t=t, stats=stats)
        np.testing.assert_array_equal(env.reward.cpu().numpy(), st.reward.astype(np.float32))
        np.testing.assert_array_equal(env.done.cpu().numpy().astype(np.int32), st.done)
        ids, ret, length, step = env.done_list()
        want = np.nonzero(st.done)[0]
        # per-workgroup segments in env order: the list is deterministic and sorted
        np.testing.assert_array_equal(ids.cpu().numpy(), want)
        assert (step.cpu().numpy() == t).all()
        total_done += len(want)
        if t % 60 == 0:
            _assert_vs_oracle(env, st, f"t={t}")
            np.testing.assert_array_equal(env.ep_return.cpu().numpy(), st.ep_return)
            np.testing.assert_array_equal(env.ep_len.cpu().numpy(), st.ep_len)
    got = env.episode_stats().cpu().numpy()
    assert total_done > 0 and got[1] == stats[1] == total_done
    assert got[2] == stats[2]
    np.testing.assert_allclose(got[0], stats[0], rtol=1e-12)  # summation order differs
    env.close()


def test_observe_and_valid_mask_vs_oracle(oracle_mod):
    O = oracle_mod
    seed, n = 5, 3001
    env = VecEnv(n, seed=seed)
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    for t in range(30):
        env.step(env.gen_actions(t))
        O.step(world, st, actions=O.gen_actions(n, env.P, seed, 0, t), seed=seed, t=t)
    obs = env.observe().cpu().numpy()
    np.testing.assert_array_equal(obs, O.observe(world, st))
    np.testing.assert_array_equal(env.valid_mask().cpu().numpy(), O.valid_mask(world, st))
    env.close()


@pytest.mark.parametrize("ports64", [False, True])
def test_tiled_and_generic_observe_and_mask_agree(oracle_mod, water, ports64):
    """Dense, 16-byte aligned outputs take the tiled kernels (a 256-row tile built in LDS,
    written with 16-byte stores); any other row stride or alignment the generic ones. Both
    equal the oracle, with ragged last tiles (n = 2 * 256 + 77) and at P = 64."""
    from shippingenv_amd.vec import random_water_ports

    O = oracle_mod
    n, seed = 2 * 256 + 77, 9
    ports = random_water_ports(water, 64, seed=4) if ports64 else None
    env = VecEnv(n, seed=seed, ports=ports)
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    for t in range(12):
        env.step(env.gen_actions(t))
        O.step(world, st, actions=O.gen_actions(n, env.P, seed, 0, t), seed=seed, t=t)
    want_obs, want_bits = O.observe(world, st), O.valid_mask(world, st)
    W, S = env.obs_size, want_bits.shape[1]
    np.testing.assert_array_equal(env.observe().cpu().numpy(), want_obs)  # tiled
    wide = torch.full((n, W + 2), -7.0, dtype=torch.float32, device=env.device)
    env.observe(wide)  # ld = W + 2: the generic kernel
    np.testing.assert_array_equal(wide[:, :W].cpu().numpy(), want_obs)
    assert bool((wide[:, W:] == -7.0).all())
    np.testing.assert_array_equal(env.valid_mask().cpu().numpy(), want_bits)  # tiled
    raw = torch.zeros(n * S + 16, dtype=torch.uint8, device=env.device)
    odd = raw[1:1 + n * S].view(n, S)  # not 16-byte aligned: the generic kernel
    env.valid_mask(odd)
    np.testing.assert_array_equal(odd.cpu().numpy(), want_bits)
    env.close()


def test_observe_and_valid_mask_vs_golden(water):
    z = load_golden(os.path.join(GOLDEN, "tape_seed0.npz"))
    k = len(z["valid_bits"])
    env = env_for(z, k, water)
    set_state(env, z, np.arange(k), prefix="post_")
    np.testing.assert_array_equal(env.valid_mask().cpu().numpy(), z["valid_bits"])
    obs = env.observe().cpu().numpy()
    np.testing.assert_array_equal(obs[:, :6], z["obs6"][:k].astype(np.float32))
    env.close()


@pytest.mark.parametrize("case", ["default", "ports64", "shared_cells", "ports100", "tiled_forced"])
def test_valid_mask_row_templates(oracle_mod, water, monkeypatch, case):
    """se_valid_mask's template kernel (round 5): every row is one of 1 + P + sum_p |ports on
    p's cell| templates (the moves alone; a port's cell; a port's cell without the origin's
    SELECT row). The states put ships on every port cell with every origin, None included,
    and at sea; n is ragged (3 tiles + 77 rows). 18 ports with three shared cells exercise the
    same-cell templates; P = 100 (> 64) and SHIPENV_MASK_TILED=1 take the round-4 tiled kernel.
    All equal the oracle (agents/dqn.py:125-175); after set_ports (new stocks) the templates
    are rebuilt and the rows follow."""
    from shippingenv_amd.vec import draw_port_stocks, random_water_ports

    O = oracle_mod
    if case == "default":
        ports = None
    elif case in ("ports64", "tiled_forced"):
        ports = random_water_ports(water, 64, seed=4)
    elif case == "shared_cells":
        base = random_water_ports(water, 12, seed=6)
        ports = base + [base[0], base[0], base[3], base[7], base[7], base[7]]
    else:
        ports = random_water_ports(water, 100, seed=7)
    if case == "tiled_forced":
        monkeypatch.setenv("SHIPENV_MASK_TILED", "1")
    n = 3 * 256 + 77
    env = VecEnv(n, seed=3, ports=ports)
    P = env.P
    rng = np.random.default_rng(11)
    at_port = rng.random(n) < 0.85
    k = rng.integers(0, P, n)
    cells = np.argwhere(env.water != 0)
    sea = cells[rng.integers(0, len(cells), n)]
    x = np.where(at_port, env.port_x[k], sea[:, 0]).astype(np.int32)
    y = np.where(at_port, env.port_y[k], sea[:, 1]).astype(np.int32)
    # origin: the port itself, another port of the same cell, any port, or None
    same = np.array([[env.port_x[a] == env.port_x[b] and env.port_y[a] == env.port_y[b] for b in range(P)]
                     for a in range(P)])
    alt = np.array([rng.choice(np.nonzero(same[i])[0]) for i in k])
    u = rng.random(n)
    origin = np.where(u < 0.4, k, np.where(u < 0.7, alt, np.where(u < 0.9, rng.integers(0, P, n), -1)))
    for stock_seed in (None, 99):
        if stock_seed is not None:
            f, c = draw_port_stocks(P, stock_seed)
            env.set_ports([[int(a), int(b)] for a, b in zip(env.port_x, env.port_y)], f, c)
        world, st = _oracle_pair(O, env)
        st.x[:], st.y[:], st.origin[:] = x, y, origin
        env.x.copy_(torch.from_numpy(x.astype(np.uint8)))
        env.y.copy_(torch.from_numpy(y.astype(np.uint8)))
        env.origin.copy_(torch.from_numpy(np.where(origin < 0, 255, origin).astype(np.uint8)))
        want = O.valid_mask(world, st)
        got = env.valid_mask().cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"{case} stocks {stock_seed}")
        assert want[:, :1].any() and (want.sum(axis=1) > 1).mean() > 0.5  # moves, and port rows
    env.close()


def test_fuel_cost_sqrt_is_correctly_rounded(oracle_mod):
    """Typed moves (dx, dy) from (0, 0) over the whole grid: fuel bits use
    np.sqrt of every reachable squared distance (shipping/util.py:4)."""
    O = oracle_mod
    dx, dy = np.meshgrid(np.arange(100), np.arange(100), indexing="ij")
    n = dx.size
    env = VecEnv(n, seed=9, water=np.ones((100, 100), np.uint8))
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=9, epoch=0)
    for f in ("x", "y"):
        getattr(env, f).zero_()
        getattr(st, f)[:] = 0
    ty = np.ones(n, np.int32)
    env.step_typed(ty, dx.ravel(), dy.ravel())
    O.step(world, st, act_type=ty, act_a=dx.ravel(), act_b=dy.ravel(), seed=9, t=0)
    _assert_vs_oracle(env, st, "sqrt")
    env.close()


# ---------------------------------------------------------------- full size
@pytest.mark.parametrize("n", [1 << 20, (1 << 26) + 3])
def test_full_size_invariants_and_sampled_exactness(oracle_mod, n):
    """N = 2^20 (BASELINE config 3) and 2^26 + 3 (the largest size tested: two groups per
    thread at the default grid cap, and a tail): every ship on a non-ground cell, indices in
    range, and 512 sampled quads (2048 envs) bit-exact against the oracle run with
    the same global ids (shard invariance of the Philox key: draws are keyed by the
    quad, and a LOSS_r block goes to the r-th firing env of its quad)."""
    O = oracle_mod
    seed, T = 2024, 40
    env = VecEnv(n, seed=seed)
    env.reset()
    rng = np.random.default_rng(1)
    quads = np.sort(rng.choice(n // 4, 512, replace=False))
    ids = (4 * quads[:, None] + np.arange(4)[None, :]).ravel()
    world = O.OracleWorld(env.water, env.port_x, env.port_y, env.port_fuel, env.port_cargo)
    sts = [O.OracleState(4) for _ in quads]
    for st, q in zip(sts, quads):
        O.reset(world, st, seed=seed, env_id_base=int(4 * q), epoch=0)
    ids_dev = torch.as_tensor(ids, device=env.device)
    for t in range(T):
        acts = env.gen_actions(t)
        env.step(acts)
        a_host = acts[ids_dev].cpu().numpy()  # the sampled quads' actions only
        for j, (st, q) in enumerate(zip(sts, quads)):
            O.step(world, st, actions=a_host[4 * j:4 * j + 4], seed=seed, env_id_base=int(4 * q), t=t)
    got = get_state(env)
    nonground = world.nonground.astype(bool)
    assert nonground[got["x"], got["y"]].all()
    assert (got["origin"] >= 0).all() and (got["origin"] < env.P).all()
    assert (got["dest"] >= 0).all() and (got["dest"] < env.P).all() and (got["dest"] != got["origin"]).all()
    for f in FIELDS:
        want = np.concatenate([getattr(st, f) for st in sts])
        if f == "fuel":
            np.testing.assert_array_equal(got[f][ids].view(np.int64), want.view(np.int64))
        else:
            np.testing.assert_array_equal(got[f][ids], want, err_msg=f)
    env.close()


def test_shard_invariance(oracle_mod):
    """Envs [k, k+m) of one big VecEnv == a VecEnv of m envs with env_id_base=k."""
    n, k, m, seed = 20000, 12348, 4000, 31  # shard offsets are multiples of 4 (quad draw blocks)
    big = VecEnv(n, seed=seed)
    part = VecEnv(m, seed=seed, env_id_base=k)
    big.reset()
    # resets are keyed by env id too: the shard's reset equals the slice of the big one
    part.reset()
    for t in range(60):
        big.step(big.gen_actions(t))
        part.step(part.gen_actions(t))
    a, b = get_state(big), get_state(part)
    for f in FIELDS:
        np.testing.assert_array_equal(a[f][k:k + m], b[f], err_msg=f)
    big.close()
    part.close()


@pytest.mark.parametrize("blocks,pad,n", [(None, None, (1 << 20) + 3), ("64", None, (1 << 20) + 3),
                                          (None, "1", (1 << 20) + 3), ("64", "1", (1 << 20) + 3),
                                          (None, None, (1 << 26) + 3)])
def test_done_list_full_size_segments(monkeypatch, blocks, pad, n):
    """N = 2^20 + 3 (tail group) with auto-reset: the compacted done list of every
    step lists exactly the envs that reported done, in env order, with the
    returns / lengths the stats slab accumulates. blocks="64": 17 iterations per
    thread, so 4,352 (iteration, wave) segments go through se_done_compact's scan.
    pad="1": each wave's records padded with filler records to the segment's 128-B line
    (the form beyond 2^23 envs, forced here): the tail group's records overwrite the
    filler past its segment's count. n = 2^26 + 3: the largest size tested, with the default
    padding (on beyond 2^23 envs) and two groups per thread at the default grid cap."""
    from shippingenv_amd.vec import random_water_ports

    from conftest import golden_water

    if blocks:
        monkeypatch.setenv("SHIPENV_STEP_BLOCKS", blocks)
    if pad:
        monkeypatch.setenv("SHIPENV_DONE_PAD", pad)
    env = VecEnv(n, seed=11, ports=random_water_ports(golden_water(), 64, seed=3), auto_reset=True)
    env.reset()
    tot_ret, tot_eps, tot_len = 0.0, 0, 0
    for t in range(320):
        env.step(env.gen_actions(t))
        if t >= 180:
            ids, ret, length, step = env.done_list()
            want = torch.nonzero(env.done).flatten().to(torch.int32)
            assert torch.equal(ids, want)
            assert bool((step == t).all())
            tot_ret += float(ret.double().sum())
            tot_eps += len(ids)
            tot_len += int(length.long().sum())
    assert tot_eps > 1000
    got = env.episode_stats().cpu().numpy()
    assert got[1] == tot_eps and got[2] == tot_len
    np.testing.assert_allclose(got[0], tot_ret, rtol=1e-9)
    env.close()


@pytest.mark.parametrize("auto", [False, True])
def test_max_map_and_ports_vs_oracle(oracle_mod, auto):
    """The largest world the ABI takes: a 256x256 map and 254 ports (SE_MAX_PORTS),
    with repeated port cells (first port wins, environment.py:150-152). Its image
    (~6 K dwords) exceeds the step kernel's unguarded staging rows, so the remainder
    staging path and the byte prefix counts at their limits run; bit-exact against
    the oracle for 300 steps with the synthetic agent (A = 4 + 254 + 250 actions)."""
    O = oracle_mod
    rng = np.random.default_rng(77)
    water = (rng.random((256, 256)) < 0.6).astype(np.uint8)
    cells = np.argwhere(water != 0)
    pick = rng.choice(len(cells), size=240, replace=False)
    ports = [[int(a), int(b)] for a, b in cells[pick]]
    ports += ports[:14]  # 14 cells hold two ports each: 254 in total
    n, seed = 6001, 99
    env = VecEnv(n, seed=seed, water=water, ports=ports, auto_reset=auto)
    assert env.P == 254
    world, st = _oracle_pair(O, env)
    env.reset()
    O.reset(world, st, seed=seed, epoch=0)
    stats = np.zeros(3)
    for t in range(300):
        acts = env.gen_actions(t)
        ref = O.gen_actions(n, env.P, seed, 0, t)
        assert np.array_equal(acts.cpu().numpy(), ref)
        env.step(acts)
        if auto:
            O.step_autoreset(world, st, ref, seed=seed, t=t, stats=stats)
        else:
            O.step(world, st, actions=ref, seed=seed, t=t)
        np.testing.assert_array_equal(env.reward.cpu().numpy(), st.reward.astype(np.float32))
        np.testing.assert_array_equal(env.err.cpu().numpy().astype(np.int32), st.err)
        if t % 50 == 49:
            _assert_vs_oracle(env, st, f"t={t}")
    # the TAKE_* / SELECT actions found ports (the O(1) lookup at 254 ports)
    assert (st.err == 0).any()
    env.close()


@pytest.mark.parametrize("auto", [False, True])
def test_graph_captured_steps_equal_eager(auto):
    """K se_step launches captured in one HIP graph (bench.py's config-3 timing path)
    and replayed once leave every field bit-identical to K eager calls."""
    from shippingenv_amd.vec import random_water_ports

    from conftest import golden_water

    n, K = 50003, 40
    ports = random_water_ports(golden_water(), 64, seed=3) if auto else None
    a = VecEnv(n, seed=21, ports=ports, auto_reset=auto)
    b = VecEnv(n, seed=21, ports=ports, auto_reset=auto)
    acts = torch.stack([a.gen_actions(t) for t in range(K)])
    a.reset()
    b.reset()
    for t in range(K):
        a.step(acts[t])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for t in range(K):
                b.step(acts[t])
    with torch.cuda.stream(side):
        g.replay()
    torch.cuda.synchronize()
    fa, fb = get_state(a), get_state(b)
    for f in FIELDS:
        np.testing.assert_array_equal(fa[f], fb[f], err_msg=f)
    for f in ("reward", "done", "err", "ep_return", "ep_len"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    a.close()
    b.close()


@pytest.mark.parametrize("auto,n", [(False, 50003), (True, 50003), (False, 1 << 16)])
def test_step_seq_equals_step_calls(auto, n):
    """se_step_seq (bench.py's timed issue path: K launches from native code, rows at a
    padded stride) leaves every field bit-identical to K VecEnv.step calls."""
    from shippingenv_amd.vec import random_water_ports

    from conftest import golden_water

    K = 24
    ports = random_water_ports(golden_water(), 64, seed=3) if auto else None
    a = VecEnv(n, seed=22, ports=ports, auto_reset=auto)
    b = VecEnv(n, seed=22, ports=ports, auto_reset=auto)
    ld = (n + 3) & ~3
    buf = torch.zeros((K, ld), dtype=torch.int32, device=a.device)
    for t in range(K):
        a.gen_actions(t, out=buf[t, :n])
    acts = buf[:, :n]
    a.reset()
    b.reset()
    for t in range(K):
        a.step(acts[t].contiguous())
    # timer marks inside the runs (se_step_seq_mark): before launch 1 (bench.py's timed loop)
    # and after launch 3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.step_seq(acts[:7], mark=e1, mark_after=0)
    b.step_seq(acts[7:], mark=e0, mark_after=3)
    e1.record()
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0.0
    with pytest.raises(Exception):
        b.step_seq(acts[:2], mark=e0, mark_after=3)  # mark_after beyond the run: SE_EINVAL
    fa, fb = get_state(a), get_state(b)
    for f in FIELDS:
        np.testing.assert_array_equal(fa[f], fb[f], err_msg=f)
    for f in ("reward", "done", "err", "ep_return", "ep_len"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    if auto:
        assert torch.equal(a.episode_stats(), b.episode_stats())
    with pytest.raises(ValueError):
        b.step_seq(acts[0])  # one row, not [K, n]
    a.close()
    b.close()


@pytest.mark.parametrize("P", [5, 64])
def test_agent_replay_need_draw_restores_state(P, water):
    """tapes that lack a variate the step needs. se_step_agent_replay answers
    SE_ERR_NEED_DRAW (10) and puts back the env's old state (step_agent.h: the group restore
    after its stores, full groups and the n % 4 tail); the typed replay kernel and the host
    build of the same code (se_host_step_replay, the drop-in's stepper) must agree bit for
    bit on state, reward, done, err and the `used` bits, and a NEED_DRAW env must equal its
    pre-state. n = 4k + 3; each tape field is NaN (or arrive_dest -1) for ~30 % of envs;
    a quarter of the envs sit one move from their destination port (arrivals)."""
    from shippingenv_amd.shipping._host import host_step_replay
    from shippingenv_amd.vec import TAPE_DTYPE, random_water_ports

    table = _reference_decode(P)
    ports = [[41, 40], [60, 22], [78, 29], [49, 72], [62, 72]] if P == 5 else random_water_ports(water, 64, seed=3)
    rng = np.random.default_rng(100 + P)
    n = 4 * 1000 + 3
    valid = sorted(i for i, v in table.items() if v is not None and i >= 0)
    acts = np.where(rng.random(n) < 0.7, rng.integers(0, 4, n), rng.choice(valid, n)).astype(np.int32)
    mk = lambda: VecEnv(n, water=water, ports=ports, seed=6)  # noqa: E731
    a, b = mk(), mk()
    for e in (a, b):
        e.reset()
        e.step(torch.ones(n, dtype=torch.int32, device=e.device))  # everyone moves east once
    st0 = get_state(a)
    # arrivals: a quarter of the envs one move from their destination port
    px, py = np.array([p[0] for p in ports]), np.array([p[1] for p in ports])
    dxy = {0: (0, -1), 1: (-1, 0), 2: (0, 1), 3: (1, 0)}  # N, E, S, W (shipping/type.py:8-16)
    for i in np.nonzero(rng.random(n) < 0.25)[0]:
        k = int(rng.integers(0, 4))
        d = st0["dest"][i]
        x, y = px[d] - dxy[k][0], py[d] - dxy[k][1]
        if 0 <= x < 100 and 0 <= y < 100:
            st0["x"][i], st0["y"][i] = x, y
            acts[i] = k
    st0["cargo"] = rng.integers(0, 60, n).astype(np.int32)
    st0["fuel"] = np.where(rng.random(n) < 0.1, rng.random(n) * 1.5, 50 + rng.random(n) * 100)
    for e in (a, b):
        for f in FIELDS:
            v = st0[f]
            if f in ("origin", "dest"):
                v = np.where(v < 0, 255, v)
            t = getattr(e, f)
            t.copy_(torch.from_numpy(np.ascontiguousarray(v).astype(t.cpu().numpy().dtype)))
    tape = np.zeros(n, TAPE_DTYPE)
    for f in ("u_fuel", "u_gate", "u_type", "beta"):
        tape[f] = np.where(rng.random(n) < 0.3, np.nan, rng.random(n))
    tape["u_gate"] = np.where(np.isnan(tape["u_gate"]), np.nan, tape["u_gate"] * 0.5)  # the gate fires often
    tape["arrive_dest"] = np.where(rng.random(n) < 0.3, -1, rng.integers(0, P, n))
    typ, va, vb = (np.zeros(n, np.int32) for _ in range(3))
    for k, i in enumerate(acts):
        typ[k], va[k], vb[k] = table[int(i)]
    ra, da, ea, used_a = a.step_agent_replay(acts, tape)
    rb, db, eb = b.step_replay(typ, va, vb, tape)
    torch.cuda.synchronize()
    used_b = b._keep[3].cpu().numpy().view(TAPE_DTYPE)
    hs = {f: (np.where(st0[f] < 0, 255, st0[f]) if f in ("origin", "dest") else st0[f]) for f in FIELDS}
    h = host_step_replay(water, a.port_x, a.port_y, a.port_fuel, a.port_cargo, hs, typ, va, vb, tape)
    sa, sb = get_state(a), get_state(b)
    hstate = {f: (np.where(h[f] == 255, -1, h[f].astype(np.int32)) if f in ("origin", "dest")
                  else (h[f] if f == "fuel" else h[f].astype(np.int32))) for f in FIELDS}
    for f in FIELDS:
        for other, name in ((sb, "typed"), (hstate, "host")):
            np.testing.assert_array_equal(np.asarray(sa[f]).view(np.uint8), np.asarray(other[f]).view(np.uint8),
                                          err_msg=f"{f}: agent vs {name}")
    ea, eb = ea.cpu().numpy().astype(np.int32), eb.cpu().numpy().astype(np.int32)
    np.testing.assert_array_equal(ea, eb)
    np.testing.assert_array_equal(ea, h["err"].astype(np.int32))
    for x, name in ((rb.cpu().numpy(), "typed"), (h["reward"], "host")):
        np.testing.assert_array_equal(ra.cpu().numpy().view(np.uint32), x.view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(da.cpu().numpy(), db.cpu().numpy())
    np.testing.assert_array_equal(da.cpu().numpy(), h["done"])
    np.testing.assert_array_equal(used_a["used"], used_b["used"])
    np.testing.assert_array_equal(used_a["used"], h["tape"]["used"])
    need = ea == 10
    assert need.sum() > 100 and (ea == 0).sum() > 100, (need.sum(), (ea == 0).sum())
    for f in FIELDS:  # NEED_DRAW: the pre-state, untouched
        np.testing.assert_array_equal(np.asarray(sa[f])[need].view(np.uint8),
                                      np.asarray(st0[f])[need].view(np.uint8), err_msg=f"restore {f}")
    assert (ra.cpu().numpy()[need] == 0).all() and (da.cpu().numpy()[need] == 0).all()
    # quads that mix NEED_DRAW and stepped envs (the restore is per env, not per group)
    q = need[:n - 3].reshape(-1, 4)
    assert ((q.sum(1) > 0) & (q.sum(1) < 4)).sum() > 50
    a.close()
    b.close()
