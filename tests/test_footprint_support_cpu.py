"""The guarded arenas of tests/footprint_support.py, without a GPU.

First the helper itself: on a sample layout with the se_state fields and a call's own buffers, one
flipped byte anywhere a kernel must not write (the last byte before a buffer, the first after it,
either end of either guard, a byte of an input) is reported with the buffer's name and the side,
and an untouched arena reports nothing. That is how test_gpu_footprint.py would fail if a kernel
stored outside its bytes: no wrong kernel is built for it.

Then the host stepper (se_host_step_replay, se_host_reset_to: "no alignment is required") on numpy
arenas whose every buffer starts at an odd address, n = 1, 3, 4, 5, over the in-contract records
of tests/golden/step_edges.npz: the results equal the fixture, the guards are intact, the inputs
unchanged (every se_tape record's input bytes, all but `used`, included), and under a reset mask the
unmasked envs keep every byte of every field.
"""
import ctypes as C

import numpy as np
import pytest

import footprint_support as F
import step_edge_support as S

TAPE_BYTES = 40  # sizeof(se_tape): four doubles, arrive_dest, used; `used`, the last 4, is the one output
SAMPLE_N = 5
SAMPLE = F.state_specs(SAMPLE_N, 2 * 4 * 8, 2 * 4) + [
    ("actions", np.int32, SAMPLE_N), ("obs", np.float32, (SAMPLE_N, 29)), ("tape", np.uint8, (SAMPLE_N, TAPE_BYTES)),
    ("ret", np.float64, 3), ("ids", np.int64, SAMPLE_N)]
NAMES = [s[0] for s in SAMPLE]


def sample_arena(odd=False):
    a = F.Arena(SAMPLE, odd=odd)
    a.set("actions", np.arange(SAMPLE_N) - 2)
    a.set("tape", np.arange(SAMPLE_N * TAPE_BYTES).reshape(SAMPLE_N, TAPE_BYTES) % 251)
    a.snapshot()
    return a


@pytest.mark.parametrize("odd", [False, True])
def test_layout_is_exact(odd):
    """Every buffer 16-byte aligned (or one past), as long as its entries, at least GUARD bytes of
    guard on either side, the trailing guard at the very next byte, no two regions overlapping."""
    a = sample_arena(odd)
    at = 0
    for name, dtype, shape in SAMPLE:
        b = a.bufs[name]
        assert b.nbytes == int(np.prod(shape)) * np.dtype(dtype).itemsize == a.view(name).nbytes
        assert a.ptr(name) % F.ALIGN == (1 if odd else 0)
        assert b.lo == at and b.start - b.lo >= F.GUARD and b.hi - b.end == F.GUARD
        assert a.view(name).ctypes.data == a.ptr(name) and a.view(name).shape == b.shape
        at = b.hi
    assert at == a.size
    image = a.host()
    guards = np.concatenate([image[b.lo:b.start] for b in a.bufs.values()])
    assert guards.min() > 0 and len(np.unique(guards[:251])) > 200  # never zero, never constant
    assert not np.array_equal(F.guard_pattern(np.arange(4096)), F.out_pattern(np.arange(4096)))
    assert F.out_pattern(np.arange(4096)).min() > 0


def test_untouched_arena_reports_nothing():
    a = sample_arena()
    assert a.check(unchanged=NAMES) == []
    a.assert_clean(unchanged=NAMES)
    for name in NAMES:
        if name not in ("actions", "tape"):
            assert a.unwritten(name).all()
    assert not a.unwritten("actions").any()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("where", ["last_before", "first_after", "guard_before_first", "guard_after_last"])
def test_one_flipped_guard_byte_is_named(name, where):
    a = sample_arena()
    b = a.bufs[name]
    pos, side, off = {"last_before": (b.start - 1, "before", -1), "first_after": (b.end, "after", 0),
                      "guard_before_first": (b.lo, "before", b.lo - b.start),
                      "guard_after_last": (b.hi - 1, "after", F.GUARD - 1)}[where]
    a.mem[pos] ^= 0x40
    found = a.check(unchanged=NAMES)
    assert found == [f"{name}: guard {side} the buffer damaged, offsets {off}..{off} (1 bytes)"], found
    with pytest.raises(AssertionError, match=f"{name}: guard {side}"):
        a.assert_clean(what="flip")
    a.mem[pos] ^= 0x40
    assert a.check(unchanged=NAMES) == []


def test_a_zeroed_or_stale_guard_is_seen():
    """A kernel that rewrites guard bytes with zeros, or with the bytes of 16 positions earlier."""
    a = sample_arena()
    b = a.bufs["fuel"]
    a.mem[b.end:b.end + 32] = 0
    assert a.check() == ["fuel: guard after the buffer damaged, offsets 0..31 (32 bytes)"]
    a = sample_arena()
    a.mem[b.lo + 16:b.lo + 48] = a.mem[b.lo:b.lo + 32].copy()
    (msg,) = a.check()
    assert msg.startswith("fuel: guard before the buffer damaged")


@pytest.mark.parametrize("name", NAMES)
def test_one_flipped_input_byte_is_named(name):
    a = sample_arena()
    b = a.bufs[name]
    for at in {0, b.nbytes // 2, b.nbytes - 1}:
        a.mem[b.start + at] ^= 1
        found = a.check(unchanged=NAMES)
        size = b.dtype.itemsize
        assert found == [f"{name}: content changed, bytes {at}..{at} (entries {at // size}..{at // size}, 1 bytes)"]
        assert a.check(unchanged=[k for k in NAMES if k != name]) == []
        if name not in ("actions", "tape"):
            assert int((~a.unwritten(name)).sum()) == 1
        a.mem[b.start + at] ^= 1


def test_negative_zero_and_nan_payloads_count():
    a = F.Arena([("v", np.float64, 3)])
    a.set("v", [0.0, np.nan, 1.0])
    a.snapshot()
    v = a.view("v")
    v[0] = -0.0
    assert a.check(unchanged=["v"]) == ["v: content changed, bytes 7..7 (entries 0..0, 1 bytes)"]
    v[0] = 0.0
    v.view(np.uint64)[1] ^= 1  # another NaN
    assert np.isnan(v[1]) and len(a.check(unchanged=["v"])) == 1


# ------------------------------------------------------------------------------ the host stepper
def host_arena(n):
    specs = F.state_specs(n, 1, 1)[:11] + [
        ("reward64", np.float64, n), ("type", np.int32, n), ("a", np.int32, n), ("b", np.int32, n),
        ("tape", np.uint8, (n, TAPE_BYTES)), ("mask", np.uint8, n), ("to_origin", np.int32, n), ("to_dest", np.int32, n)]
    return F.Arena(specs, odd=True)


def se_state(a, reward64=True):
    from shippingenv_amd import _native as N

    return N.SeState(*[a.ptr(f) for f in F.BIND_ORDER[:11]] + [None, None, a.ptr("reward64") if reward64 else None])


@pytest.fixture(scope="module")
def host_worlds():
    from shippingenv_amd import _native as N
    from shippingenv_amd.shipping._host import _create

    hs = {w: _create(N.lib(), *S.world(w)) for w in range(S.n_worlds())}
    yield hs
    for h in hs.values():
        N.lib().se_host_destroy(h)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_host_step_replay_stays_in_its_bytes(host_worlds, n):
    """Every in-contract record of every world, n at a time (the last chunk of a world wraps round
    to its first records), every buffer at an odd address: the fixture's results, intact guards,
    unchanged inputs, only `used` written in the tape, ep_return / ep_start never touched."""
    from shippingenv_amd import _native as N
    from shippingenv_amd.vec import TAPE_DTYPE

    z = S.fixture()
    a = host_arena(n)
    st = se_state(a)
    calls = 0
    for w, h in host_worlds.items():
        sel_all = S.records(w)
        for lo in range(0, len(sel_all), n if n > 1 else 4):  # one env at a time: every fourth record
            sel = sel_all[np.arange(lo, lo + n) % len(sel_all)]
            a.fill_out()
            for f, v in S.pre_state(sel, u8_none=True).items():
                a.set(f, v)
            for f, k in (("type", "act_type"), ("a", "act_a"), ("b", "act_b")):
                a.set(f, z[k][sel])
            tape = S.tape_of(TAPE_DTYPE, sel)
            tape["used"] = -0x5A5A5A5B
            a.set("tape", tape.view(np.uint8).reshape(n, TAPE_BYTES))
            before = a.snapshot()
            N.check(N.lib().se_host_step_replay(h, n, C.byref(st), a.ptr("type"), a.ptr("a"), a.ptr("b"), a.ptr("tape")))
            calls += 1
            image = a.host()
            what = f"world {w} records {sel.tolist()}"
            a.assert_clean(unchanged=("type", "a", "b", "mask", "to_origin", "to_dest", "ep_return", "ep_start"),
                           image=image, what=what)
            got_tape = a.get("tape", image)
            np.testing.assert_array_equal(got_tape[:, :TAPE_BYTES - 4], a.get("tape", before)[:, :TAPE_BYTES - 4], err_msg=what)
            np.testing.assert_array_equal(got_tape[:, TAPE_BYTES - 4:].copy().view(np.int32)[:, 0], z["used"][sel], err_msg=what)
            got = {f: a.get(f, image) for f in S.FIELDS}
            post = {f: (np.where(got[f] == 255, -1, got[f].astype(np.int32)) if f in ("origin", "dest") else got[f])
                    for f in S.FIELDS}
            S.assert_post(post, sel, what)
            np.testing.assert_array_equal(a.get("reward64", image).view(np.int64), z["reward"][sel].view(np.int64))
            np.testing.assert_array_equal(a.get("reward", image), z["reward"][sel].astype(np.float32))
            np.testing.assert_array_equal(a.get("done", image).astype(np.int32), z["done"][sel])
            np.testing.assert_array_equal(a.get("err", image).astype(np.int32), z["err"][sel])
            raised = z["err"][sel] != 0  # a raising step leaves its env's state bytes as they were
            for f in S.FIELDS:
                np.testing.assert_array_equal(a.get(f, image)[raised].view(np.uint8),
                                              a.get(f, before)[raised].view(np.uint8), err_msg=f"{what}: {f}")
    assert calls >= sum(len(S.records(w)) for w in host_worlds) // max(n, 4)


@pytest.mark.parametrize("masked", [None, "none", "some"])
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_host_reset_to_stays_in_its_bytes(host_worlds, n, masked):
    """se_host_reset_to on world 3 (the 100-side world): masked envs get the reset's values, ep_return
    0 and the stamp 0; unmasked envs keep every byte of every field, reward, done and err included;
    reward64 and the inputs are not touched."""
    from shippingenv_amd import _native as N

    water, px, py, pf, pc = S.world(3)
    P = len(px)
    a = host_arena(n)
    st = se_state(a, reward64=False)
    origin = np.arange(n) % P
    dest = (origin + 1 + np.arange(n) % (P - 1)) % P
    mask = {None: np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "some": (np.arange(n) % 3 == 0).astype(np.uint8)}[masked]
    a.set("mask", mask * 7)  # any nonzero byte selects
    a.set("to_origin", np.where(mask, origin, -5))  # an unmasked env's origin / dest are not looked at
    a.set("to_dest", np.where(mask, dest, 10**6))
    before = a.snapshot()
    N.check(N.lib().se_host_reset_to(host_worlds[3], n, C.byref(st), None if masked is None else a.ptr("mask"),
                                     a.ptr("to_origin"), a.ptr("to_dest")))
    image = a.host()
    a.assert_clean(unchanged=("reward64", "type", "a", "b", "tape", "mask", "to_origin", "to_dest"), image=image,
                   what=f"reset_to n={n} mask={masked}")
    sel = mask != 0
    want = dict(x=px[origin], y=py[origin], fuel=200.0, cargo=0, origin=origin, dest=dest, reward=0.0, done=0, err=0,
                ep_return=0.0, ep_start=0)
    for f, dt in F.STATE_FIELDS:
        got = a.get(f, image)
        np.testing.assert_array_equal(got[~sel].view(np.uint8), a.get(f, before)[~sel].view(np.uint8), err_msg=f)
        np.testing.assert_array_equal(got[sel], np.broadcast_to(np.asarray(want[f]).astype(dt), (n,))[sel], err_msg=f)
