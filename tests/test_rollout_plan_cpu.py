"""Scripted rollouts on the CPU: the yardstick of tests/test_gpu_rollout_plan.py and the C-ABI's
argument checks (no GPU).

(a) The restatement of se_rollout_plan (tests/plan_support.py: the oracle's typed step with a
tape drawn from Philox blocks (k, 12) and (k, 13)), fed the attempts of the random policy,
reproduces oracle.rollout bit for bit. This pins the draw contract the GPU tests hold
se_rollout_plan to: plan position k reads what se_rollout's attempt k reads.
(b) se_rollout_plan is declared and exported, and misuse is a status before anything touches a
device."""
import ctypes as C

import numpy as np
import pytest

import plan_support as PS
import rollout_support as RS

O = pytest.importorskip("oracle.oracle")

BASES = (0, (1 << 32) - 7)  # the second: the ids carry into the high word inside the batch


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    O.build()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("name", list(RS.WORLDS))
def test_random_plans_reproduce_the_random_rollouts(name, base):
    """Every actor x 64 of the world's table at BUDGET: the restatement, fed random_plan's
    attempts, equals oracle.rollout's trace in ret (bits), steps, raised, the final ship and
    DONE-ness; the plan is as long as the rollout's attempts."""
    world, st = RS.WORLDS[name].oracle(O), RS.table(O, name)
    src = RS.table_src(name)
    ms, ma = RS.BUDGET
    ret, steps, status, log = O.rollout(world, st, src, max_steps=ms, max_attempts=ma, seed=RS.SEED,
                                        rollout_base=base, trace=True)
    plans, results = PS.random_table(O, RS, name, base)
    assert len(results) == len(src) == RS.REPS * len(RS.actors(name))
    got_ret = np.array([r.ret for r in results])
    np.testing.assert_array_equal(got_ret.view(np.uint64), ret.view(np.uint64), err_msg="ret")
    np.testing.assert_array_equal([r.steps for r in results], steps, err_msg="steps")
    np.testing.assert_array_equal([r.raised for r in results], log["raised"], err_msg="raised")
    np.testing.assert_array_equal([r.status == PS.DONE for r in results], status == RS.DONE, err_msg="done")
    np.testing.assert_array_equal([r.used & 12 for r in results], log["used"] & 12, err_msg="beta and arrival draws")
    for j, f in enumerate(("x", "y", "fuel", "cargo", "origin", "dest")):
        got = np.array([r.ship[j] for r in results], log[f].dtype)
        if f == "fuel":
            np.testing.assert_array_equal(got.view(np.uint64), log[f].view(np.uint64), err_msg=f)
        else:
            np.testing.assert_array_equal(got, log[f], err_msg=f)
    # an attempt is a counted or a raising step; a rollout whose sample_action raised made none more
    np.testing.assert_array_equal([len(p) for p in plans], steps + log["raised"])
    for r in results:
        assert (r.first_err_at >= 0) == (r.raised > 0) == (r.first_err != 0)


def test_the_tables_go_through_both_blocks_and_every_ending():
    seen, used, raised = set(), 0, 0
    for name in RS.WORLDS:
        for r in PS.random_table(O, RS, name, 0)[1]:
            seen.add(r.status)
            used |= r.used
            raised = max(raised, r.raised)
    assert seen == {PS.DONE, PS.END} and used & PS.USED_BETA and used & PS.USED_ARRIVE and raised > 1


def test_restatement_counts_positions_not_steps():
    """A raising action takes its plan position's draws with it: the plan with a raise put in
    front plays the same actions under the next positions' draws, and a pad at the end changes
    nothing."""
    world = RS.OPEN.oracle(O)
    ship = (3, 4, 100.0, 30, 0, 1)
    moves = [(1, 0, 1), (1, 1, 0), (1, 0, -1), (1, -1, 0)] * 3
    plain = PS.plan_rollout(O, world, ship, moves, RS.SEED, 77)
    padded = PS.plan_rollout(O, world, ship, moves + [(0, 0, 0)] * 3, RS.SEED, 77)
    assert (padded.ret, padded.steps, padded.ship) == (plain.ret, plain.steps, plain.ship)
    assert (padded.raised, padded.first_err, padded.first_err_at) == (3, 7, len(moves))
    shifted = PS.plan_rollout(O, world, ship, [(0, 0, 0)] + moves, RS.SEED, 77)
    assert shifted.steps == plain.steps and shifted.first_err_at == 0
    assert shifted.ship[2] != plain.ship[2]  # other fuel draws
    cut = PS.plan_rollout(O, world, ship, moves, RS.SEED, 77, length=5)
    assert cut.steps == 5 and PS.plan_rollout(O, world, ship, moves, RS.SEED, 77, length=-3).steps == 0
    assert PS.plan_rollout(O, world, ship, moves, RS.SEED, 77, length=99).ret == plain.ret


def test_agent_plans_decode_like_the_agent_step():
    world = RS.OPEN.oracle(O)
    ship = (3, 4, 100.0, 0, 0, 1)
    idx = [0, 1, -1, -4, -5, 2, 3, 4 + world.P + 250, (1 << 31) - 1, -(1 << 31)]
    dec = PS.decode_plan(O, world.P, idx)
    assert [d[3] for d in dec] == [0, 0, 0, 0, 9, 0, 0, 0, 0, 9]  # only an index below -4 fails to decode
    got = PS.plan_rollout(O, world, ship, idx, RS.SEED, 5, agent=True)
    typed = PS.plan_rollout(O, world, ship, [d[:3] if not d[3] else (0, 0, 0) for d in dec], RS.SEED, 5)
    assert (got.ret, got.steps, got.ship, got.raised) == (typed.ret, typed.steps, typed.ship, typed.raised)
    assert got.first_err == 9 and got.first_err_at == 4 and typed.first_err == 7


# ---------------------------------------------------------------------------- the C-ABI
@pytest.fixture(scope="module")
def lib():
    from shippingenv_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def aligned(nbytes, offset=0):
    """(keep-alive, address): host memory 16-byte aligned (+ offset). Never dereferenced: every
    call below fails its argument checks."""
    raw = C.create_string_buffer(nbytes + 32)
    return raw, (C.addressof(raw) + 15) // 16 * 16 + offset


def test_declared_exported_and_constants(lib):
    from shippingenv_amd import _native as N

    assert "se_rollout_plan" in N.EXPORTS and hasattr(lib, "se_rollout_plan")
    assert (N.PLAN_DONE, N.PLAN_END, N.PLAN_BAD_SRC) == (0, 1, 4) == (PS.DONE, PS.END, PS.BAD_SRC)
    assert C.sizeof(N.SePlanOut) == 9 * C.sizeof(C.c_void_p)
    assert lib.se_abi_version() == 2


def test_misuse_is_a_status_before_any_device(lib):
    keep, bufs = [], []
    for _ in range(7):
        k, p = aligned(256)
        keep.append(k)
        bufs.append(p)
    src, ty, a, b, ret, cnt, status = bufs
    m, ld, K = 8, 8, 3

    def call(env=None, src=src, m=m, ty=ty, a=a, b=b, ld=ld, K=K, length=None, ids=None, base=0,
             ret=ret, cnt=cnt, status=status):
        rc = lib.se_rollout_plan(env, src, m, ty, a, b, ld, K, length, ids, base, ret, cnt, status, None, None)
        return rc, lib.se_last_error().decode()

    rc, msg = call()
    assert rc == -1 and "null env" in msg  # the arguments are fine: the env is what is wrong
    assert call(a=None, b=None)[1] == msg  # the agent-index form too
    for kw, word in (
        (dict(ld=m - 1), "stride"),
        (dict(a=None), "a and b"), (dict(b=None), "a and b"),
        (dict(K=-1), ">= 0"), (dict(m=-1, ld=8), ">= 0"), (dict(base=-1), ">= 0"),
        (dict(src=None), "null plan buffer"), (dict(ret=None), "null plan buffer"),
        (dict(cnt=None), "null plan buffer"), (dict(status=None), "null plan buffer"),
        (dict(ty=None), "null plan buffer"), (dict(ty=None, a=None, b=None), "null plan buffer"),
        (dict(ty=ty + 4), "aligned"), (dict(a=a + 8), "aligned"), (dict(b=b + 4), "aligned"),
        (dict(ld=9), "aligned"),
    ):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # what is not misuse gets as far as the env: one row needs no stride, no row needs no plan
    assert "null env" in call(ld=9, K=1)[1]
    assert "null env" in call(ty=None, a=None, b=None, K=0)[1]
    assert "null env" in call(m=0, ld=0, src=None, ret=None, cnt=None, status=None)[1]
