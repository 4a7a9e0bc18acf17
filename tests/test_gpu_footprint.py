"""Every entry point held to the memory footprint include/shipenv.h documents for it.

The other GPU suites take state, inputs and outputs from torch's caching allocator, which rounds
every tensor up to 512 bytes: a store a few entries past n, before entry 0 or into a buffer a call
"only reads" lands in slack, faults nowhere and changes nothing a test reads. Here every buffer of
a call is a view into one guarded arena (tests/footprint_support.py; test_footprint_support_cpu.py
shows the arena reporting each kind of damage): exactly as long as the header says, its trailing
guard at the very next byte, at least 4 KiB of position-dependent guard on either side, so that an
overrun is read back and nothing can fault. Each call runs once on such a guarded env and once on
an ordinary twin with the same arguments and the same pre-state, and is held, in this order, to:

1. every guard intact;
2. every input byte-identical (actions, typed type / a / b, src, plans, len, ids, masks, tapes
   except `used`);
3. every state field the header calls read-only or not written for the call byte-identical;
4. every output entry the header says is not written still holding the prefill;
5. every written output and state field equal to the twin's, byte for byte;
6. for se_reset, se_step, se_step_typed, se_observe and se_valid_mask, equal to the C oracle too.

Sizes: the edges of a group of 4, a wave of 64, a workgroup row of 256 groups and, with
SHIPENV_STEP_BLOCKS=1 at 2052 envs, more than one group per thread. Pre-states: a reset and three
steps of the synthetic agent; the auto-reset cases put a third of the envs at fuel 0.5, so every
wave finishes some and the done lists, stamps and statistics are written.
"""
import ctypes as C

import numpy as np
import pytest

import footprint_support as F
from rollout_support import OPEN

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

SEED = 2027
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1028]
CASES = [pytest.param(n, None, id=str(n)) for n in SIZES] + [pytest.param(2052, "1", id="2052-one-block")]
sizes = pytest.mark.parametrize("n,blocks", CASES)
SHIP = ("x", "y", "fuel", "cargo", "origin", "dest")
EPISODE = ("ep_return", "ep_start")
LISTS = ("done_recs", "done_count")
TAPE_BYTES = 40  # sizeof(se_tape); `used` is its last 4 bytes
i32, u8, f64, f32, i64 = np.int32, np.uint8, np.float64, np.float32, np.int64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


_OPEN = []


@pytest.fixture(autouse=True)
def _close_after():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error is sticky: end the session instead of launching more
        _OPEN.clear()
        pytest.exit(f"the device reported an error, nothing more is run: {e}", returncode=3)
    while _OPEN:  # handles before their env, also when the test failed
        _OPEN.pop().close()


def keep(obj):
    _OPEN.append(obj)
    return obj


def lib():
    from shippingenv_amd import _native as N

    return N.lib()


def ok(rc):
    from shippingenv_amd import _native as N

    N.check(rc)


def dev(env, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def raw(t):
    """A device tensor's bytes on the host."""
    return t.contiguous().cpu().numpy().reshape(-1).view(np.uint8)


def same(got, want, what):
    """got (numpy, from the arena) and want (a twin's tensor, or numpy) hold the same bytes."""
    want = raw(want) if isinstance(want, torch.Tensor) else np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    np.testing.assert_array_equal(np.ascontiguousarray(got).reshape(-1).view(np.uint8), want, err_msg=what)


class Pair:
    """A guarded env g (state and the call's buffers `extra` in one arena) and its ordinary twin t,
    made by the same constructor call. prestate() plays the twin into the pre-state and keeps it;
    load() puts both envs there: the live state copied in, every other bound buffer holding the
    arena's prefill in both, the same counters, cleared statistics."""

    def __init__(self, make, extra=(), auto=False):
        self.t, self.g = keep(make()), keep(make())
        self.auto = auto
        self.arena = F.guard_env(self.g, extra)
        self.n, self.nseg, self.seg = self.g.n, self.g.done_segments, self.g.done_seg
        self.live = SHIP + (EPISODE if auto else ())
        # what the twin is compared in: without auto-reset its done lists are one record long
        self.fields = tuple(f for f, _ in F.STATE_FIELDS) + (LISTS if auto else ())

    def prestate(self, steps=3):
        t = self.t
        t.reset()
        for k in range(steps):
            t.step(t.gen_actions(k))
        if self.auto:
            t.fuel[::3] = 0.5  # a move from here runs dry: the episode finishes
        torch.cuda.synchronize()
        self.saved = {f: getattr(t, f).clone() for f in self.live}
        self.counters = t.counters
        self.load()
        return self

    def twin_field(self, f):
        v = getattr(self.t, f)
        return v[:2 * self.nseg] if f == "done_count" else v

    def load(self):
        g, t = self.g, self.t
        for e in (g, t):
            e.set_counters(*self.counters)  # clears the counts: before the prefill
            e.clear_stats()
        self.arena.fill_out(*F.BIND_ORDER)
        for f in self.live:
            getattr(g, f).copy_(self.saved[f])
            getattr(t, f).copy_(self.saved[f])
        for f in self.fields:
            if f not in self.live:
                self.twin_field(f).copy_(getattr(g, f))
        return self.arena.snapshot()

    def oracle_state(self):
        st = O.OracleState(self.n)
        for f in SHIP:
            v = self.saved[f].cpu().numpy()
            getattr(st, f)[:] = np.where(v == 255, -1, v.astype(i32)) if f in ("origin", "dest") else v
        return st

    def oracle_world(self):
        e = self.g
        return O.OracleWorld(e.water, e.port_x, e.port_y, e.port_fuel, e.port_cargo)

    def verify(self, what, inputs=(), readonly=(), twin=True):
        """Claims 1, 2, 3 and the state part of 5, in that order -> the arena's host image."""
        a = self.arena
        image = a.host()
        a.assert_clean(image=image, what=f"{what}: guards")
        a.assert_clean(unchanged=inputs, image=image, what=f"{what}: inputs")
        a.assert_clean(unchanged=readonly, image=image, what=f"{what}: read-only state")
        if twin:
            for f in self.fields:
                same(a.get(f, image), self.twin_field(f), f"{what}: {f} against the twin")
            assert self.g.counters == self.t.counters, what
        return image


def default_pair(n, blocks, monkeypatch, extra=(), auto=False, env=()):
    from shippingenv_amd.vec import VecEnv

    names = ("SHIPENV_STEP_BLOCKS", "SHIPENV_DONE_PAD", "SHIPENV_SEQ_FUSE", "SHIPENV_SEQ_GATE_POOL", "SHIPENV_SEQ_RING")
    want = dict(env, SHIPENV_STEP_BLOCKS=blocks)
    for name in names:
        if want.get(name) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, want[name])
    return Pair(lambda: VecEnv(n, seed=SEED, auto_reset=auto, device="cuda:0"), extra, auto).prestate()


def open_pair(n, blocks, monkeypatch, extra=()):
    if blocks is None:
        monkeypatch.delenv("SHIPENV_STEP_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("SHIPENV_STEP_BLOCKS", blocks)
    return Pair(lambda: OPEN.env(n, seed=SEED), extra).prestate()


def agent_actions(p, t, hostile=True):
    """The synthetic agent's mix; with hostile, every 11th index past the action space and every
    17th below -4 (both raise SE_ERR_BAD_INDEX)."""
    acts = O.gen_actions(p.n, p.g.P, SEED, 0, t)
    if hostile:
        acts[5::11] = 4 + p.g.P + 250 + 3
        acts[2::17] = -9
    return acts


def unchanged_envs(p, image, snap, sel, fields, what):
    for f in fields:
        same(p.arena.get(f, image)[sel], p.arena.get(f, snap)[sel], f"{what}: {f} of the envs left alone")


def none_to_minus1(v):
    return np.where(v == 255, -1, v.astype(i32))


def against_oracle(p, image, st, what, outs=True):
    a = p.arena
    for f in SHIP:
        got = a.get(f, image)
        if f == "fuel":
            same(got, st.fuel, f"{what}: fuel bits against the oracle")
        else:
            got = none_to_minus1(got) if f in ("origin", "dest") else got.astype(i32)
            np.testing.assert_array_equal(got, getattr(st, f), err_msg=f"{what}: {f} against the oracle")
    if outs:
        np.testing.assert_array_equal(a.get("reward", image), st.reward.astype(f32), err_msg=f"{what}: reward")
        np.testing.assert_array_equal(a.get("done", image).astype(i32), st.done, err_msg=f"{what}: done")
        np.testing.assert_array_equal(a.get("err", image).astype(i32), st.err, err_msg=f"{what}: err")


# ------------------------------------------------------------------------------ reset
@pytest.mark.parametrize("auto", [False, True], ids=["plain", "auto"])
@sizes
def test_reset_and_reset_to(monkeypatch, n, blocks, auto):
    """se_reset / se_reset_to with mask NULL, all-zero and every third env: the masked envs equal
    the twin's (se_reset: the oracle's, with reward, done, err and ep_return 0 and the stamp the
    step counter); the unmasked envs keep every byte of all eleven per-env fields, reward, done and
    err included; the done lists are not touched, auto-reset or not."""
    p = default_pair(n, blocks, monkeypatch, [("mask", u8, n), ("to_origin", i32, n), ("to_dest", i32, n)], auto)
    a, g, t = p.arena, p.g, p.t
    P = g.P
    origin = (np.arange(n) * 3) % P
    dest = (origin + 1 + np.arange(n) % (P - 1)) % P
    per_env = tuple(f for f, _ in F.STATE_FIELDS)
    for which in ("reset", "reset_to"):
        for kind in ("null", "zero", "third"):
            what = f"se_{which} n={n} mask={kind} auto={auto}"
            p.load()
            mask = {"null": np.ones(n, u8), "zero": np.zeros(n, u8), "third": (np.arange(n) % 3 == 1).astype(u8)}[kind]
            a.set("mask", mask * 201)  # any nonzero byte selects
            a.set("to_origin", origin)
            a.set("to_dest", dest)
            snap = a.snapshot()
            mp = None if kind == "null" else a.cptr("mask")
            tm = None if kind == "null" else dev(t, mask * 201)
            if which == "reset":
                ok(lib().se_reset(g._h, mp, g._stream()))
                t.reset(tm)
            else:
                ok(lib().se_reset_to(g._h, mp, a.cptr("to_origin"), a.cptr("to_dest"), g._stream()))
                t.reset_to(origin, dest, tm)
            image = p.verify(what, inputs=("mask", "to_origin", "to_dest"), readonly=LISTS)
            sel = mask != 0
            unchanged_envs(p, image, snap, ~sel, per_env, what)
            st = p.oracle_state()
            if which == "reset":
                O.reset(p.oracle_world(), st, mask=mask, seed=SEED, epoch=p.counters[1])
            else:
                O.reset(p.oracle_world(), st, mask=mask, origin=origin, dest=dest)
            against_oracle(p, image, st, what, outs=False)
            zero = dict(reward=f32(0), done=u8(0), err=np.int8(0), ep_return=f32(0), ep_start=i32(p.counters[0]))
            for f, v in zero.items():
                got = a.get(f, image)[sel]
                same(got, np.full(len(got), v), f"{what}: {f} of the envs it reset")


# ------------------------------------------------------------------------------ plain steps
@pytest.mark.parametrize("typed", [False, True], ids=["agent", "typed"])
@sizes
def test_step_without_auto_reset(monkeypatch, n, blocks, typed):
    """se_step / se_step_typed: ep_return, ep_start, done_recs and done_count are bound but never
    written; a raising step leaves its env's six state fields byte for byte; everything equals the
    twin and the oracle."""
    p = default_pair(n, blocks, monkeypatch, [("actions", i32, n), ("type", i32, n), ("a", i32, n), ("b", i32, n)])
    a, g, t = p.arena, p.g, p.t
    what = f"{'se_step_typed' if typed else 'se_step'} n={n}"
    st = p.oracle_state()
    if typed:
        ty, aa, bb, bad = O.decode_agent(agent_actions(p, 11, hostile=False), g.P)
        assert (bad == 0).all()
        ty[3::13] = 0   # SE_ERR_BAD_CATEGORY
        ty[7::19] = 5
        for f, v in (("type", ty), ("a", aa), ("b", bb)):
            a.set(f, v)
        snap = a.snapshot()
        ok(lib().se_step_typed(g._h, a.cptr("type"), a.cptr("a"), a.cptr("b"), g._stream()))
        t.step_typed(ty, aa, bb)
        O.step(p.oracle_world(), st, act_type=ty, act_a=aa, act_b=bb, seed=SEED, t=p.counters[0])
    else:
        acts = agent_actions(p, 11)
        a.set("actions", acts)
        snap = a.snapshot()
        ok(lib().se_step(g._h, a.cptr("actions"), g._stream()))
        t.step(dev(t, acts))
        O.step(p.oracle_world(), st, actions=acts, seed=SEED, t=p.counters[0])
    image = p.verify(what, inputs=("actions", "type", "a", "b"), readonly=EPISODE + LISTS)
    raised = a.get("err", image) != 0
    unchanged_envs(p, image, snap, raised, SHIP, what)
    if n >= 63:
        assert raised.any() and not raised.all()
    assert not a.unwritten("reward", image).any()  # every env's outputs are written
    against_oracle(p, image, st, what)


# ------------------------------------------------------------------------------ the auto-reset step
@pytest.mark.parametrize("pad", [None, "1"], ids=["unpadded", "padded"])
@sizes
def test_step_with_auto_reset_done_lists_and_statistics(monkeypatch, n, blocks, pad):
    """se_step on an auto-reset env: records past a segment's count are the prefill or filler, the
    other parity half of done_recs / done_count is untouched, ep_start changes only where an env
    finished; the twin and the oracle agree. Then se_done_compact into exactly n records and one
    count (out_count records written, the rest prefill) and se_episode_stats into exactly three
    doubles, both leaving every bound buffer as it was. n = 1 and 3 are the regression cases of the
    tail kernel's counts: with no full group only it runs, and it used to write one segment's count
    of the four, leaving the rest as se_bind had cleared them."""
    extra = [("actions", i32, n), ("out", i32, (n, 4)), ("out_count", i32, 1), ("stats", f64, 3)]
    p = default_pair(n, blocks, monkeypatch, extra, auto=True, env={"SHIPENV_DONE_PAD": pad})
    a, g, t = p.arena, p.g, p.t
    what = f"se_step auto n={n} pad={pad}"
    acts = agent_actions(p, 12)
    a.set("actions", acts)
    snap = a.snapshot()
    ok(lib().se_step(g._h, a.cptr("actions"), g._stream()))
    t.step(dev(t, acts))
    image = p.verify(what, inputs=("actions",))
    step_t = p.counters[0]
    half = step_t & 1
    recs = a.get("done_recs", image).reshape(2, p.nseg * p.seg, 4)
    counts = a.get("done_count", image).reshape(2, p.nseg)
    pre_recs = a.prefill("done_recs").reshape(2, p.nseg * p.seg, 4)
    same(recs[1 - half], pre_recs[1 - half], f"{what}: the other half's records")
    same(counts[1 - half], a.prefill("done_count").reshape(2, p.nseg)[1 - half], f"{what}: the other half's counts")
    done = a.get("done", image) != 0
    assert ((counts[half] >= 0) & (counts[half] <= p.seg)).all() and counts[half].sum() == done.sum(), what
    listed = []
    for s in range(p.nseg):
        k = counts[half][s]
        listed.append(recs[half][s * p.seg:s * p.seg + k])
        rest = recs[half][s * p.seg + k:(s + 1) * p.seg]
        untouched = (rest == pre_recs[half][s * p.seg + k:(s + 1) * p.seg]).all(1)
        filler = (rest[:, 0] == -1) & (rest[:, 3] == np.array(step_t & 0xFFFFFFFF, np.uint32).view(i32))
        assert (untouched | filler).all() and (pad is not None or untouched.all()), f"{what}: segment {s} past its count"
    listed = np.concatenate(listed)
    np.testing.assert_array_equal(listed[:, 0], np.nonzero(done)[0], err_msg=f"{what}: listed envs")
    if n >= 63:
        assert done.sum() >= n // 6, what  # the low-fuel third mostly moved and ran dry
    unchanged_envs(p, image, snap, ~done, ("ep_start",), what)
    st = p.oracle_state()
    st.ep_return[:] = p.saved["ep_return"].cpu().numpy()
    st.ep_len[:] = (step_t - p.saved["ep_start"].cpu().numpy().astype(np.int64)).astype(i32)
    O.step_autoreset(p.oracle_world(), st, acts, seed=SEED, t=step_t)
    against_oracle(p, image, st, what)
    same(a.get("ep_return", image), st.ep_return, f"{what}: ep_return against the oracle")

    a.snapshot()
    ok(lib().se_done_compact(g._h, a.cptr("out"), a.cptr("out_count"), g._stream()))
    image = p.verify(f"{what}: se_done_compact", inputs=("actions",), readonly=F.BIND_ORDER)
    k = int(a.get("out_count", image)[0])
    assert k == done.sum()
    same(a.get("out", image)[:k], listed, f"{what}: compacted records")
    assert a.unwritten("out", image)[k:].all(), f"{what}: se_done_compact wrote past out_count records"
    ids, ret, length, step = t.done_list()
    for col, want in enumerate((ids, ret, length, step)):
        same(a.get("out", image)[:k, col], want, f"{what}: compacted column {col} against the twin")

    a.snapshot()
    ok(lib().se_episode_stats(g._h, a.cptr("stats"), g._stream()))
    image = p.verify(f"{what}: se_episode_stats", inputs=("actions", "out", "out_count"), readonly=F.BIND_ORDER)
    same(a.get("stats", image), t.episode_stats(), f"{what}: statistics against the twin")
    assert a.get("stats", image)[1] == done.sum()


# ------------------------------------------------------------------------------ replayed steps
@pytest.mark.parametrize("agent", [False, True], ids=["typed", "agent"])
@sizes
def test_replayed_steps_write_only_used(monkeypatch, n, blocks, agent):
    """se_step_replay / se_step_agent_replay: of the tape only tape[i].used changes; an env whose
    tape lacks a variate answers SE_ERR_NEED_DRAW and keeps every state byte; the step counter
    stays; the episode fields and the done lists are not written."""
    from shippingenv_amd.vec import TAPE_DTYPE

    assert TAPE_DTYPE.itemsize == TAPE_BYTES
    extra = [("actions", i32, n), ("type", i32, n), ("a", i32, n), ("b", i32, n), ("tape", u8, (n, TAPE_BYTES))]
    p = default_pair(n, blocks, monkeypatch, extra)
    a, g, t = p.arena, p.g, p.t
    what = f"{'se_step_agent_replay' if agent else 'se_step_replay'} n={n}"
    rng = np.random.default_rng(n)
    tape = np.zeros(n, TAPE_DTYPE)
    for f in ("u_fuel", "u_gate", "u_type", "beta"):
        tape[f] = rng.random(n)
    dest = none_to_minus1(p.saved["dest"].cpu().numpy())
    tape["arrive_dest"] = (np.maximum(dest, 0) + 1 + rng.integers(0, g.P - 1, n)) % g.P
    blank = np.arange(n) % 5 == 2  # no variates: a move there needs a draw
    for f in ("u_fuel", "u_gate", "u_type", "beta"):
        tape[f][blank] = np.nan
    tape["arrive_dest"][blank] = -1
    tape["used"] = 0x7A7A7A7A
    a.set("tape", tape.view(u8).reshape(n, TAPE_BYTES))
    acts = agent_actions(p, 13, hostile=agent)
    if agent:
        a.set("actions", acts)
        snap = a.snapshot()
        ok(lib().se_step_agent_replay(g._h, a.cptr("actions"), a.cptr("tape"), g._stream()))
        used_twin = t.step_agent_replay(acts, tape)[3]["used"]
    else:
        ty, aa, bb, _ = O.decode_agent(acts, g.P)
        for f, v in (("type", ty), ("a", aa), ("b", bb)):
            a.set(f, v)
        snap = a.snapshot()
        ok(lib().se_step_replay(g._h, a.cptr("type"), a.cptr("a"), a.cptr("b"), a.cptr("tape"), g._stream()))
        t.step_replay(ty, aa, bb, tape)
        used_twin = t._keep[3].cpu().numpy().view(TAPE_DTYPE)["used"]
    image = p.verify(what, inputs=("actions", "type", "a", "b"), readonly=EPISODE + LISTS)
    assert g.counters == p.counters
    got = a.get("tape", image)
    same(got[:, :TAPE_BYTES - 4], a.get("tape", snap)[:, :TAPE_BYTES - 4], f"{what}: the tape's variates")
    np.testing.assert_array_equal(got[:, TAPE_BYTES - 4:].copy().view(i32)[:, 0], used_twin, err_msg=f"{what}: used")
    err = a.get("err", image)
    need = err == 10
    unchanged_envs(p, image, snap, need, SHIP, what)
    unchanged_envs(p, image, snap, err != 0, SHIP, what)
    assert not (need & ~blank).any()
    if n >= 63:
        assert need.any() and (err == 0).any()


# ------------------------------------------------------------------------------ step sequences
SEQ_MODES = {"fused": {}, "no-gate-pool": {"SHIPENV_SEQ_GATE_POOL": "0"}, "no-ring": {"SHIPENV_SEQ_RING": "0"},
             "per-step": {"SHIPENV_SEQ_FUSE": "0"}}


@pytest.mark.parametrize("mode", list(SEQ_MODES))
@sizes
def test_step_seq_reads_its_rows_and_writes_the_last_step(monkeypatch, n, blocks, mode):
    """se_step_seq over K = 1, 2, 9 rows of a [K, ld] matrix with ld > n carved with its own guards
    (the ld - n padding columns hold the prefill, the twin's hold zeros: they are not read, and
    not changed): state and outputs equal K se_step calls on the twin, so the outputs are the last
    step's; the episode fields and the done lists are not written."""
    ld = (n + 3) // 4 * 4 + 4
    extra = [(f"rows{K}", i32, (K, ld)) for K in (1, 2, 9)]
    p = default_pair(n, blocks, monkeypatch, extra, env=SEQ_MODES[mode])
    a, g, t = p.arena, p.g, p.t
    for K in (1, 2, 9):
        what = f"se_step_seq {mode} n={n} K={K}"
        p.load()
        rows = np.stack([agent_actions(p, 20 + k) for k in range(K)])
        mat = a.prefill(f"rows{K}").copy()
        mat[:, :n] = rows
        a.set(f"rows{K}", mat)
        a.snapshot()
        ok(lib().se_step_seq(g._h, a.cptr(f"rows{K}"), ld, K, g._stream()))
        for k in range(K):
            t.step(dev(t, rows[k]))
        image = p.verify(what, inputs=[f"rows{j}" for j in (1, 2, 9)], readonly=EPISODE + LISTS)
        assert not a.unwritten("reward", image).any(), what
    # the same rows through the wrapper's own [K, n] view of a padded tensor
    p.load()
    padded = torch.zeros((9, ld), dtype=torch.int32, device=t.device)
    padded[:, :n] = dev(t, rows)
    t.step_seq(padded[:, :n])
    ok(lib().se_step_seq(g._h, a.cptr("rows9"), ld, 9, g._stream()))
    p.verify(f"se_step_seq {mode} n={n} against step_seq", readonly=EPISODE + LISTS)


@sizes
def test_step_seq_with_auto_reset_is_a_launch_per_step(monkeypatch, n, blocks):
    """se_step_seq on an auto-reset env, K = 2 rows at ld > n: two se_step calls on the twin, the
    done lists of both parity halves, the stamps and the statistics included."""
    ld = (n + 3) // 4 * 4 + 4
    p = default_pair(n, blocks, monkeypatch, [("rows", i32, (2, ld)), ("stats", f64, 3)], auto=True)
    a, g, t = p.arena, p.g, p.t
    rows = np.stack([agent_actions(p, 40 + k) for k in range(2)])
    mat = a.prefill("rows").copy()
    mat[:, :n] = rows
    a.set("rows", mat)
    a.snapshot()
    ok(lib().se_step_seq(g._h, a.cptr("rows"), ld, 2, g._stream()))
    for k in range(2):
        t.step(dev(t, rows[k]))
    what = f"se_step_seq auto n={n}"
    image = p.verify(what, inputs=("rows",))
    counts = a.get("done_count", image)
    assert ((counts >= 0) & (counts <= p.seg)).all(), what  # both halves were written
    ok(lib().se_episode_stats(g._h, a.cptr("stats"), g._stream()))
    same(a.get("stats"), t.episode_stats(), f"{what}: statistics")


# ------------------------------------------------------------------------------ se_step_record
@pytest.mark.parametrize("slack", [0, 4])
@sizes
def test_step_record_cut_and_ring(monkeypatch, n, blocks, slack):
    """se_step_record on rings of capacity n and n + 4, two steps (the second wraps the ring): cut
    has exactly n bytes, all written; state, stamps, done lists and cut equal se_replay_begin +
    se_step_record on the twin; the ring never holds more than its capacity and a minibatch of
    every stored transition is the twin's."""
    from shippingenv_amd.dqn import MiniBatch, ReplayBuffer

    p = default_pair(n, blocks, monkeypatch, [("actions", i32, n), ("cut", u8, n)], auto=True)
    a, g, t = p.arena, p.g, p.t
    rbs = [keep(ReplayBuffer(e, n + slack)) for e in (g, t)]
    cut_t = torch.full((n,), 0x55, dtype=torch.uint8, device=t.device)
    for k in range(2):
        what = f"se_step_record n={n} capacity={n + slack} step {k}"
        acts = agent_actions(p, 30 + k)
        a.set("actions", acts)
        a.fill_out("cut")
        a.snapshot()
        ok(lib().se_replay_begin(rbs[0]._h, a.cptr("actions"), g._stream()))
        ok(lib().se_step_record(rbs[0]._h, a.cptr("actions"), a.cptr("cut"), 5, g._stream()))
        at = dev(t, acts)
        rbs[1].begin(at)
        rbs[1].step_end(at, cut_t, 5)
        image = p.verify(what, inputs=("actions",))
        assert not a.unwritten("cut", image).any(), what
        same(a.get("cut", image), cut_t, f"{what}: cut")
        assert set(np.unique(a.get("cut", image)).tolist()) <= {0, 1}
        assert rbs[0].size == rbs[1].size == min((k + 1) * n, n + slack) <= rbs[0].capacity == n + slack
    B = rbs[0].size
    outs = [MiniBatch(B, e.obs_size, e.device) for e in (g, t)]
    for rb, out in zip(rbs, outs):
        rb.sample(out, t=3)
    for name in ("obs", "next_obs", "act", "rew", "done", "weight"):
        same(raw(getattr(outs[0], name)), getattr(outs[1], name), f"ring n={n} capacity={n + slack}: {name}")
    p.verify(f"se_replay_sample n={n}", twin=False)


# ------------------------------------------------------------------------------ the views
@sizes
def test_views_and_action_generators_only_read_the_state(monkeypatch, n, blocks):
    """se_observe (ld = W and W + 3), se_valid_mask, se_gen_actions, se_sample_actions: every bound
    buffer is byte-identical afterwards; the outputs equal the twin's (the first two the oracle's);
    the three padding columns of the wide observation keep the prefill."""
    W, A = 6 + 4 * 5, 4 + 5 + 250
    stride = (A + 7) // 8
    extra = [("obs", f32, (n, W)), ("wide", f32, (n, W + 3)), ("bits", u8, (n, stride)), ("actions", i32, n),
             ("type", i32, n), ("a", i32, n), ("b", i32, n)]
    p = default_pair(n, blocks, monkeypatch, extra)
    a, g, t = p.arena, p.g, p.t
    assert g.obs_size == W and g.action_space_size == A
    s = g._stream()
    ok(lib().se_observe(g._h, a.cptr("obs"), W, s))
    ok(lib().se_observe(g._h, a.cptr("wide"), W + 3, s))
    ok(lib().se_valid_mask(g._h, a.cptr("bits"), s))
    ok(lib().se_gen_actions(g._h, a.cptr("actions"), 77, s))
    ok(lib().se_sample_actions(g._h, a.cptr("type"), a.cptr("a"), a.cptr("b"), 78, s))
    what = f"views n={n}"
    image = p.verify(what, readonly=F.BIND_ORDER)
    same(a.get("obs", image), t.observe(), f"{what}: obs")
    same(a.get("wide", image)[:, :W], a.get("obs", image), f"{what}: wide rows")
    assert a.unwritten("wide", image)[:, W:].all(), f"{what}: se_observe wrote its padding columns"
    same(a.get("bits", image), t.valid_mask(), f"{what}: valid mask")
    same(a.get("actions", image), t.gen_actions(77), f"{what}: gen_actions")
    for f, want in zip(("type", "a", "b"), t.sample_actions(78)):
        same(a.get(f, image), want, f"{what}: sample_actions {f}")
    st, world = p.oracle_state(), p.oracle_world()
    same(a.get("obs", image), O.observe(world, st), f"{what}: obs against the oracle")
    same(a.get("bits", image), O.valid_mask(world, st), f"{what}: valid mask against the oracle")
    same(a.get("actions", image), O.gen_actions(n, g.P, SEED, 0, 77), f"{what}: gen_actions against the oracle")


# ------------------------------------------------------------------------------ rollouts
@sizes
def test_rollout_family_writes_m_entries(monkeypatch, n, blocks):
    """se_rollout, se_rollout_plan and se_rollout_nav with m = the size under test over 65 source
    envs (some sources bad), and se_nav_actions on the 65: m (n) entries per output, the optional
    outputs passed as NULL absent, the env's state and counters unchanged, outputs the twin's."""
    from shippingenv_amd import _native as N
    from shippingenv_amd.nav import VecNavigator

    m, K = n, 5
    ld = (m + 3) // 4 * 4 + 4
    ints = ("steps", "status", "pcounted", "pstatus", "praised", "pfirst_err", "px", "pcargo",
            "ncounted", "nstatus", "narrivals", "nstuck_at", "ndest")
    extra = ([("src", i32, m), ("plen", i32, m), ("ids", i64, m)] + [(k, i32, (K, ld)) for k in ("ptype", "pa", "pb")]
             + [(k, f64, m) for k in ("ret", "pret", "nret", "nfuel")] + [(k, i32, m) for k in ints]
             + [(k, i32, 65) for k in ("vtype", "va", "vb", "vstatus", "vdist")])
    p = open_pair(65, blocks, monkeypatch, extra)
    a, g, t = p.arena, p.g, p.t
    navs = [keep(VecNavigator(e, load=2)) for e in (g, t)]
    src = (np.arange(m) * 7) % 65
    src[3::9] = 65
    src[5::31] = -1
    rng = np.random.default_rng(m)
    plan = [a.prefill(k).copy() for k in ("ptype", "pa", "pb")]
    ty, aa, bb, _ = O.decode_agent(rng.integers(0, 4 + g.P + 30, K * m), g.P)
    for mat, v in zip(plan, (ty, aa, bb)):
        mat[:, :m] = v.reshape(K, m)
    plan[0][:, 1:m:6] = 0  # a pad: raises
    plen = rng.integers(-1, K + 2, m)
    ids = rng.integers(0, 50, m)
    for k, v in (("src", src), ("plen", plen), ("ids", ids), ("ptype", plan[0]), ("pa", plan[1]), ("pb", plan[2])):
        a.set(k, v)
    a.snapshot()
    s = g._stream()
    ok(lib().se_rollout(g._h, a.cptr("src"), m, 5, 10, 100, a.cptr("ret"), a.cptr("steps"), a.cptr("status"), s))
    pout = N.SePlanOut(a.ptr("praised"), a.ptr("pfirst_err"), None, a.ptr("px"), None, None, a.ptr("pcargo"), None, None)
    ok(lib().se_rollout_plan(g._h, a.cptr("src"), m, a.cptr("ptype"), a.cptr("pa"), a.cptr("pb"), ld, K, a.cptr("plen"),
                             a.cptr("ids"), 0, a.cptr("pret"), a.cptr("pcounted"), a.cptr("pstatus"), C.byref(pout), s))
    nout = N.SeNavOut(a.ptr("narrivals"), None, a.ptr("nstuck_at"),
                      N.SePlanOut(None, None, None, None, None, a.ptr("nfuel"), None, None, a.ptr("ndest")))
    rb = navs[1].refuel_below
    ok(lib().se_rollout_nav(navs[0]._h, a.cptr("src"), m, K, rb, 2, None, 7, a.cptr("nret"), a.cptr("ncounted"),
                            a.cptr("nstatus"), C.byref(nout), s))
    ok(lib().se_nav_actions(navs[0]._h, rb, 2, a.cptr("vtype"), a.cptr("va"), a.cptr("vb"), a.cptr("vstatus"), None,
                            a.cptr("vdist"), s))
    what = f"rollouts m={m}"
    inputs = ("src", "plen", "ids", "ptype", "pa", "pb")
    image = p.verify(what, inputs=inputs, readonly=F.BIND_ORDER)
    r = t.rollout(src, max_steps=5, max_attempts=10, rollout_base=100)
    for k, want in zip(("ret", "steps", "status"), r):
        same(a.get(k, image), want, f"{what}: se_rollout {k}")
    tw = [torch.zeros((K, ld), dtype=torch.int32, device=t.device) for _ in range(3)]
    for d, v in zip(tw, plan):
        d[:, :m] = dev(t, v[:, :m])
    r = t.rollout_plan(src, tw[0][:, :m], tw[1][:, :m], tw[2][:, :m], lengths=plen, ids=ids, return_end=True)
    for k, want in (("pret", r.ret), ("pcounted", r.steps), ("pstatus", r.status), ("praised", r.raised),
                    ("pfirst_err", r.first_err), ("px", r.x), ("pcargo", r.cargo)):
        same(a.get(k, image), want, f"{what}: se_rollout_plan {k}")
    r = navs[1].rollout(src, steps=K, rollout_base=7, return_end=True)
    for k, want in (("nret", r.ret), ("ncounted", r.steps), ("nstatus", r.status), ("narrivals", r.arrivals),
                    ("nstuck_at", r.stuck_at), ("nfuel", r.fuel), ("ndest", r.dest)):
        same(a.get(k, image), want, f"{what}: se_rollout_nav {k}")
    r = navs[1].actions(dist=True)
    for k, want in zip(("vtype", "va", "vb", "vstatus", "vdist"), r):
        same(a.get(k, image), want, f"{what}: se_nav_actions {k}")
    if m >= 63:
        assert (a.get("status", image) == 4).any() and (a.get("pstatus", image) == 4).any()


# ------------------------------------------------------------------------------ SARSA
@sizes
def test_sarsa_step_and_choose(monkeypatch, n, blocks):
    """se_sarsa_step / se_sarsa_choose on OPEN with the table carved at exactly rows * A doubles
    and the se_sarsa_state fields and the five outputs at n entries: a learning step equals the
    twin's in the table, the learner's state, the outputs and the env; learn = 0 leaves every table
    byte; choose modifies nothing but its three outputs."""
    from shippingenv_amd import _native as N
    from shippingenv_amd.sarsa import VecSARSAAgent

    from sarsa_support import Layout

    lay = Layout(OPEN.oracle(O))
    extra = ([("q", f64, (lay.rows, lay.A)), ("type", i32, n), ("a", i32, n), ("b", i32, n), ("fresh", u8, n),
              ("ep_len", i32, n), ("sarsa_return", f64, n), ("s_reward", f64, n), ("ended", u8, n), ("status", i32, n),
              ("fin_return", f64, n), ("fin_len", i32, n)] + [(k, i32, n) for k in ("ctype", "ca", "cb")])
    p = open_pair(n, blocks, monkeypatch, extra)
    a, g, t = p.arena, p.g, p.t
    ags = [keep(VecSARSAAgent(e, max_steps=3, max_attempts=4)) for e in (g, t)]
    assert (ags[0].rows, ags[0].A) == (lay.rows, lay.A)
    learner = ("type", "a", "b", "fresh", "ep_len", "sarsa_return")
    q0 = np.random.default_rng(9).standard_normal((lay.rows, lay.A)) * 0.01
    a.set("q", q0)
    ags[1].q.copy_(dev(t, q0))
    for k, v in (("type", 0), ("a", 0), ("b", 0), ("fresh", 1), ("ep_len", 0), ("sarsa_return", 0.0)):
        a.set(k, np.full(n, v))
    sst = N.SeSarsaState(*[a.ptr(k) for k in learner])
    ok(lib().se_sarsa_bind(ags[0]._h, a.cptr("q"), C.byref(sst)))
    outs = ("s_reward", "ended", "status", "fin_return", "fin_len")

    def step(learn, tt):
        ok(lib().se_sarsa_step(ags[0]._h, 0.1, 0.9, 0.3, learn, 3, 4, tt, *[a.cptr(k) for k in outs], g._stream()))
        ags[1].t = tt
        ags[1].step(learn=bool(learn), epsilon=0.3)

    for tt, learn in ((0, 1), (1, 1), (2, 0)):
        what = f"se_sarsa_step n={n} t={tt} learn={learn}"
        a.fill_out(*outs)
        a.snapshot()
        step(learn, tt)
        image = p.verify(what, readonly=LISTS + (() if learn else ("q",)))
        same(a.get("q", image), ags[1].q, f"{what}: the table")
        tw = ags[1]
        for k, want in zip(learner + outs, (tw.type, tw.a, tw.b, tw.fresh, tw.ep_len, tw.ep_return, tw.reward,
                                            tw.ended, tw.status, tw.fin_return, tw.fin_len)):
            same(a.get(k, image), want, f"{what}: {k}")
    if n >= 63:
        assert not np.array_equal(a.get("q", image), q0)  # the learning steps did write
    what = f"se_sarsa_choose n={n}"
    a.snapshot()
    ok(lib().se_sarsa_choose(ags[0]._h, 0.3, 5, a.cptr("ctype"), a.cptr("ca"), a.cptr("cb"), g._stream()))
    ags[1].t = 5
    image = p.verify(what, readonly=F.BIND_ORDER + ("q",) + learner + outs)
    for k, want in zip(("ctype", "ca", "cb"), ags[1].choose_action(epsilon=0.3)):
        same(a.get(k, image), want, f"{what}: {k}")


# ------------------------------------------------------------------------------ MCTS
@pytest.mark.parametrize("nav", [False, True], ids=["random", "navigator"])
@sizes
def test_mcts_choose_tree_entries(monkeypatch, n, blocks, nav):
    """se_mcts_choose / se_mcts_choose_nav with S = 3 simulations and playouts of 5 steps: the four
    outputs and tree_count have n entries, tree n * (S + 1) nodes; tree[i * (S + 1) + j] holds the
    prefill for j >= tree_count[i] and the twin's node below; the env is unchanged."""
    from shippingenv_amd.mcts import VecMCTSAgent
    from shippingenv_amd.nav import VecNavigator

    S = 3
    extra = [(k, i32, n) for k in ("type", "a", "b", "status", "tree_count")] + [("tree", i32, (n, S + 1, 8))]
    p = open_pair(n, blocks, monkeypatch, extra)
    a, g, t = p.arena, p.g, p.t
    navs = [keep(VecNavigator(e, load=2)) if nav else None for e in (g, t)]
    ags = [keep(VecMCTSAgent(e, num_simulations=S, max_rollout_steps=5, max_attempts=10, navigator=v))
           for e, v in zip((g, t), navs)]
    what = f"{'se_mcts_choose_nav' if nav else 'se_mcts_choose'} n={n}"
    a.snapshot()
    tail = (0, a.cptr("type"), a.cptr("a"), a.cptr("b"), a.cptr("status"), a.cptr("tree"), a.cptr("tree_count"), g._stream())
    if nav:
        ok(lib().se_mcts_choose_nav(ags[0]._h, navs[0]._h, navs[1].refuel_below, 2, S, 1.4, 5, *tail))
    else:
        ok(lib().se_mcts_choose(ags[0]._h, S, 1.4, 5, 10, *tail))
    image = p.verify(what, readonly=F.BIND_ORDER)
    ty, aa, bb, status, tree = ags[1].choose_action(return_tree=True)
    for k, want in (("type", ty), ("a", aa), ("b", bb), ("status", status), ("tree_count", tree.count)):
        same(a.get(k, image), want, f"{what}: {k}")
    count = a.get("tree_count", image)
    assert ((count >= 1) & (count <= S + 1)).all()
    got = a.get("tree", image)
    written = np.arange(S + 1)[None, :] < count[:, None]
    assert a.unwritten("tree", image).all(-1)[~written].all(), f"{what}: nodes from tree_count[i] on were written"
    for col, want in enumerate((tree.parent, tree.type, tree.a, tree.b, tree.visits)):
        np.testing.assert_array_equal(got[:, :, col][written], want.cpu().numpy()[written], err_msg=f"{what}: column {col}")
    assert (got[:, :, 5][written] == 0).all()  # reserved
    total = np.ascontiguousarray(got[:, :, 6:8]).view(f64).reshape(n, S + 1)
    same(total[written], tree.total_reward.cpu().numpy()[written], f"{what}: total_reward")


# ------------------------------------------------------------------------------ the DQN policy
@sizes
def test_policy_actions_have_n_entries(monkeypatch, n, blocks):
    """se_policy / se_policy_f32 with q_out NULL: `actions` has n entries between its guards, the
    twin's values; the env is unchanged."""
    from shippingenv_amd.policy import DQNNetwork, QPolicy

    p = default_pair(n, blocks, monkeypatch, [("bf16", i32, n), ("f32", i32, n)])
    a, g, t = p.arena, p.g, p.t
    torch.manual_seed(5)
    model = DQNNetwork(g.obs_size, g.action_space_size)
    pols = [keep(QPolicy(e, model)) for e in (g, t)]
    a.snapshot()
    ok(lib().se_policy(pols[0]._h, a.cptr("bf16"), 0.3, 4, None, 0, g._stream()))
    ok(lib().se_policy_f32(pols[0]._h, a.cptr("f32"), 0.3, 4, None, 0, g._stream()))
    what = f"se_policy n={n}"
    image = p.verify(what, readonly=F.BIND_ORDER)
    same(a.get("bf16", image), pols[1].act(0.3, 4).clone(), f"{what}: actions")
    same(a.get("f32", image), pols[1].act(0.3, 4, precision="f32").clone(), f"{what}: fp32 actions")
