"""Network-policy rollouts on the CPU: the yardstick of tests/test_gpu_qnet_rollout.py (no GPU).

(a) The restatement of se_rollout_qnet (tests/qnet_rollout_support.py) under the explore law alone
(epsilon = 1), and under the integer and the zero network at epsilon 0 and 0.3, replayed through
plan_support.plan_rollout as an agent-index plan under the same id, gives the same result (the plan
equality of include/shipenv.h on the host).
(b) Its valid-action enumeration is oracle.valid_mask on the recorded worlds and states of
tests/golden/views_edges.npz, whose bits the reference's is_valid_action gave.
(c) The hand ships and worlds the GPU file plays reach every status and both outcomes of every
branch of the position, by the restatement alone.
(d) The C-ABI: declared, exported, laid out as the header says, and every argument check answers
SE_EINVAL whatever the handle."""
import math

import numpy as np
import pytest

import plan_support as PS
import qnet_rollout_support as QS
import views_edge_support as VS

O = pytest.importorskip("oracle.oracle")

CHOOSERS = [(None, 1.0), ("integer", 0.0), ("integer", 0.3), ("zero", 0.0), ("zero", 0.3)]


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    O.build()


@pytest.mark.parametrize("net,eps", CHOOSERS)
@pytest.mark.parametrize("name", list(QS.WORLDS))
def test_emitted_actions_replay_as_an_agent_index_plan(name, net, eps):
    """Every world's ships: the plan of the emitted agent indices gives ret (bits), counted,
    first_err(_at), the end ship and DONE / END; a RAISED rollout emitted counted + 1 actions, its
    plan skips the last and reads END."""
    w, m, steps = QS.WORLDS[name]
    world, ships, src = w.oracle(O), QS.ships_for(w), QS.world_src(name)
    rolls, _ = QS.suite(O, name, net, eps)
    sp = PS.Stepper(O, world, QS.SEED)
    assert len(rolls) == m
    for r, ro in enumerate(rolls):
        if ro is QS.BAD:
            assert not 0 <= src[r] < len(ships)
            continue
        plan = PS.plan_rollout(O, world, ships[src[r]], ro.actions, QS.SEED, QS.BASE + r, agent=True, stepper=sp)
        a, b = ro.res, plan
        assert math.copysign(1, a.ret) == math.copysign(1, b.ret) and a.ret == b.ret, r
        assert (a.steps, a.raised, a.first_err, a.first_err_at, a.ship) == (b.steps, b.raised, b.first_err, b.first_err_at, b.ship), r
        assert len(ro.actions) == a.steps + a.raised == len(ro.kinds) and len(ro.actions) <= steps
        if a.status == QS.RAISED:
            assert b.status == QS.END and a.raised == 1 and a.first_err_at == a.steps and a.first_err in (QS.ERR_OOB, QS.ERR_NO_DEST)
        else:
            assert a.status == b.status and a.raised == 0 and (a.first_err, a.first_err_at) == (0, -1)
            assert len(ro.actions) == steps or a.status == QS.DONE
        assert ro.explored == ro.kinds.count("explore") and (eps > 0 or ro.explored == 0)
        assert eps < 1 or ro.explored == len(ro.actions)


@pytest.mark.parametrize("name", VS.worlds())
def test_valid_actions_are_the_reference_bits(name):
    """Player.valid on every recorded state of the world is the set bits of the reference's
    is_valid_action, ascending, and the explore law's count 4 + nsel + cst + fst."""
    water, px, py, pf, pc = VS.world(name)
    world = O.OracleWorld(water, px, py, pf, pc)
    pl = QS.Player(O, world)
    cols = VS.states(name)
    bits = VS.want_bits(name)
    for i in range(len(cols["x"])):
        ship = tuple(int(cols[f][i]) if f != "fuel" else float(cols[f][i]) for f in QS.SHIP)
        got = pl.valid(ship)
        want = np.flatnonzero(np.unpackbits(bits[i])[:pl.A]).tolist()
        assert got == want and got == sorted(got) and got[:4] == [0, 1, 2, 3], (name, i)
        here = [p for p in range(world.P) if (px[p], py[p]) == (ship[0], ship[1])]
        cst = min(int(pc[here[0]]), 49) if here else 0
        fst = min(int(pf[here[0]]), 199) if here else 0
        nsel = len([p for p in here if p != ship[4]])
        assert len(got) == 4 + nsel + cst + fst, (name, i)


def test_the_hand_suite_reaches_every_status_and_branch():
    """By the restatement alone, over the cases the GPU file plays: DONE, END, RAISED by a move with
    no destination, RAISED by a move off the map, BAD_SRC; a position that explored and one that
    did not under one epsilon; slot 13 drawn for a partial loss and for an arrival; greedy moves,
    SELECTs and both TAKEs; exact ties decided by the first maximum; every kind of action explored."""
    statuses, kinds, used, tied = set(), set(), 0, 0
    for name, (w, m, steps) in QS.WORLDS.items():
        P = w.P
        family = lambda a: "move" if a < 4 else "select" if a < 4 + P else "cargo" if a < 54 + P else "fuel"  # noqa: E731
        for net, eps in CHOOSERS:
            rolls, pl = QS.suite(O, name, net, eps)
            tied += pl.tied
            for ro in rolls:
                if ro is QS.BAD:
                    statuses.add(QS.BAD_SRC)
                    continue
                s = ro.res
                statuses.add((QS.RAISED, s.first_err) if s.status == QS.RAISED else s.status)
                used |= s.used
                kinds |= {(k, family(a)) for k, a in zip(ro.kinds, ro.actions)}
                if 0 < eps < 1 and "explore" in ro.kinds and "greedy" in ro.kinds:
                    kinds.add("both in one rollout")
    assert statuses == {QS.DONE, QS.END, QS.BAD_SRC, (QS.RAISED, QS.ERR_NO_DEST), (QS.RAISED, QS.ERR_OOB)}, statuses
    assert {(k, f) for k in ("greedy", "explore") for f in ("move", "select", "cargo", "fuel")} <= kinds, kinds
    assert "both in one rollout" in kinds and tied > 0
    assert used & PS.USED_BETA and used & PS.USED_ARRIVE
    # the short runs the GPU file also plays
    for steps in (0, 1, 2):
        short = QS.suite(O, "hand", "integer", 0.3, steps=steps, m=67)[0]
        assert all(ro is QS.BAD or len(ro.actions) <= steps for ro in short)
        assert steps > 0 or all(ro is QS.BAD or (ro.res.status == QS.END and ro.res.ret == 0.0) for ro in short)


def test_integer_networks_are_exact_in_bf16():
    """Every weight, bias, input and activation of the integer networks is an integer bf16 holds
    (|v| <= 256; IntNet.q asserts the activations), and every Q stays below 2^13: each product and
    each partial sum is then exact in f32 in any order."""
    for name, (w, _, _) in QS.WORLDS.items():
        for make in QS.NETS.values():
            net = make(w.P)
            for t in (net.w1, net.b1, net.w2, net.b2, net.w3, net.b3):
                assert np.abs(t).max() <= 8
            for ship in QS.ships_for(w):
                assert np.abs(net.q(ship)).max() < 1 << 13
    net = QS.IntNet.integer(5)
    q = net.q((7, 3, 100.0, 0, 2, QS.NONE))
    h =np.array([7, 3, 3, 0, 4, 0, 1, 0])  # x, y, origin + 1, dest + 1, relu(x - y), relu(y - x), 1, relu(3 - x)
    np.testing.assert_array_equal(q, net.w3[:, :8] @ h + net.b3)


# ---------------------------------------------------------------------------- the C-ABI
@pytest.fixture(scope="module")
def lib():
    from shippingenv_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def test_declared_exported_and_misuse_is_a_status_before_any_device(lib):
    """se_rollout_qnet is declared and exported, se_qnet_out has the header's layout, the ABI
    version stays 2, and every argument check answers SE_EINVAL whatever the handle: here there is
    none, and a call whose arguments are fine gets as far as saying so."""
    import ctypes as C

    from shippingenv_amd import _native as N

    assert "se_rollout_qnet" in N.EXPORTS and hasattr(lib, "se_rollout_qnet")
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(N.SeQnetOut) == 12 * ptr and (N.SeQnetOut.ld.offset, N.SeQnetOut.explored.offset, N.SeQnetOut.end.offset) == (ptr, 2 * ptr, 3 * ptr)
    assert lib.se_abi_version() == 2 and (N.PLAN_RAISED, N.QROLL_PAD) == (QS.RAISED, QS.PAD) == (6, -5)
    keep = [C.create_string_buffer(256 + 32) for _ in range(5)]
    src, ret, cnt, status, act = [(C.addressof(k) + 15) // 16 * 16 for k in keep]  # never dereferenced
    m = 8

    def call(mode=0, eps=0.0, src=src, m=m, base=0, steps=3, ret=ret, cnt=cnt, status=status, act=act, ld=8, out=True):
        o = N.SeQnetOut(act, ld, None, N.SePlanOut())
        rc = lib.se_rollout_qnet(None, mode, eps, src, m, None, base, steps, ret, cnt, status, C.byref(o) if out else None, None)
        return rc, lib.se_last_error().decode()

    rc, msg = call()
    assert rc == -1 and "null qnet" in msg  # the arguments are fine: the handle is what is wrong
    for kw, word in (
        (dict(m=-1), ">= 0"), (dict(steps=-1), ">= 0"), (dict(base=-1), ">= 0"),
        (dict(eps=float("nan")), "epsilon"), (dict(eps=-1e-300), "epsilon"),
        (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(mode=1), "fp32-faithful rollout is not built"),
        (dict(ld=m - 1), "ld"), (dict(ld=9), "aligned"), (dict(act=act + 4), "aligned"),
        (dict(src=None), "null rollout buffer"), (dict(ret=None), "null rollout buffer"),
        (dict(cnt=None), "null rollout buffer"), (dict(status=None), "null rollout buffer"),
    ):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # what is not misuse gets as far as the handle: one row needs no stride, no rows need no ld, epsilon past 1
    for kw in (dict(ld=9, steps=1), dict(act=None, ld=0), dict(out=False), dict(eps=float("inf")), dict(eps=-0.0),
               dict(m=0, src=None, ret=None, cnt=None, status=None)):
        assert "null qnet" in call(**kw)[1], kw
