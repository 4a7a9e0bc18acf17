"""The optional outputs of se_rollout_plan and se_rollout_nav, each on its own.

VecEnv.rollout_plan and VecNavigator.rollout pass either every pointer of se_plan_out / se_nav_out
or all but the six end-ship fields. Here the library is called directly: with `out` NULL, with an
`out` of null pointers only, and with exactly one field set, each field in turn. ret, counted,
status and the one requested field must equal the all-fields call's, bit for bit (ret and fuel as
uint64), and every output that was not asked for must stay as it was. 65 rollouts (a full wave and
one lane) of 5 steps on world `open`, one source among them bad; typed and agent-index plans."""
import ctypes as C

import numpy as np
import pytest

import plan_support as PS
from test_gpu_rollout_plan import agent_menu, menu_plans, rows, table_env

torch = pytest.importorskip("torch")
O = pytest.importorskip("oracle.oracle")

pytestmark = pytest.mark.gpu

M, K, BAD_AT = 65, 5, 40
POISON = -7
PLAN_OUT = ("raised", "first_err", "first_err_at", "x", "y", "fuel", "cargo", "origin", "dest")
NAV_OUT = ("arrivals", "nav_status", "stuck_at") + PLAN_OUT
HEAD = ("ret", "counted", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    O.build()


def poisoned(env, names):
    """One POISON-filled device tensor of M entries per name: f64 for ret and fuel, else int32."""
    return {f: torch.full((M,), POISON, dtype=torch.float64 if f in ("ret", "fuel") else torch.int32, device=env.device)
            for f in names}


def collect(t, asked):
    """The tensors as numpy arrays (f64 as its bits), after checking that those not asked for are untouched."""
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in t.items()}
    for f, v in got.items():
        if f not in HEAD and f not in asked:
            assert (v == POISON).all(), f"{f} was written without being asked for (asked: {asked})"
    return {f: v.view(np.uint64) if v.dtype == np.float64 else v for f, v in got.items()}


def addr(t, f, asked):
    return t[f].data_ptr() if f in asked else None


def call_plan(env, src, plan, base, asked):
    """se_rollout_plan with the fields `asked` of se_plan_out set; asked None: out NULL."""
    from shippingenv_amd import _native as N

    t = poisoned(env, HEAD + PLAN_OUT)
    fields = asked or ()
    out = N.SePlanOut(*[addr(t, f, fields) for f in PLAN_OUT])
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())  # noqa: E731
    N.check(N.lib().se_rollout_plan(env._h, ptr(src), M, ptr(plan[0]), ptr(plan[1]), ptr(plan[2]), plan[0].stride(0), K,
                                    None, None, base, ptr(t["ret"]), ptr(t["counted"]), ptr(t["status"]),
                                    None if asked is None else C.byref(out), env._stream()))
    return collect(t, fields)


def call_nav(nav, src, base, asked):
    """se_rollout_nav with the fields `asked` of se_nav_out set; asked None: out NULL."""
    from shippingenv_amd import _native as N

    env = nav.env
    t = poisoned(env, HEAD + NAV_OUT)
    fields = asked or ()
    out = N.SeNavOut(*[addr(t, f, fields) for f in NAV_OUT[:3]], N.SePlanOut(*[addr(t, f, fields) for f in PLAN_OUT]))
    ptr = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    N.check(N.lib().se_rollout_nav(nav._h, ptr(src), M, K, nav.refuel_below, nav.load, None, base, ptr(t["ret"]),
                                   ptr(t["counted"]), ptr(t["status"]), None if asked is None else C.byref(out),
                                   env._stream()))
    return collect(t, fields)


def assert_each_field_alone(call, names, what):
    """call(asked) for: every field, out NULL, no field, and each field alone."""
    full = call(names)
    assert full["status"][BAD_AT] == PS.BAD_SRC and (full["status"] == PS.BAD_SRC).sum() == 1
    assert all((full[f] != POISON).any() for f in names), "the all-fields call writes every field"
    for asked in [None, ()] + [(f,) for f in names]:
        got = call(asked)
        for f in HEAD + tuple(asked or ()):
            np.testing.assert_array_equal(got[f], full[f], err_msg=f"{what}, asked {asked}: {f}")
    return full


@pytest.mark.parametrize("kind", ["typed", "agent"])
def test_plan_outputs_one_at_a_time(kind):
    env, _, st = table_env("open")
    rng = np.random.default_rng(65)
    src_h = rng.integers(0, st.n, M).astype(np.int32)
    src_h[BAD_AT] = st.n
    src = torch.as_tensor(src_h, device=env.device)
    if kind == "typed":
        ty, a, b, _ = PS.pack(menu_plans(rng, M, K), K=K)
        plan = (rows(env, ty), rows(env, a), rows(env, b))
    else:
        menu = agent_menu(4)
        plan = (rows(env, np.array([[menu[j] for j in rng.integers(0, len(menu), M)] for _ in range(K)], np.int32)), None, None)
    full = assert_each_field_alone(lambda asked: call_plan(env, src, plan, (1 << 32) - 30, asked), PLAN_OUT, kind)
    assert (full["raised"] > 0).any() and (full["counted"] > 0).any() and full["x"][BAD_AT] == -1
    env.close()


def test_nav_outputs_one_at_a_time():
    from test_gpu_nav import make, navigator

    env, _, st, rb, load = make("open")
    nav = navigator(env, rb, load)
    rng = np.random.default_rng(66)
    src_h = rng.integers(0, st.n, M).astype(np.int32)
    src_h[BAD_AT] = -1
    src = torch.as_tensor(src_h, device=env.device)
    full = assert_each_field_alone(lambda asked: call_nav(nav, src, (1 << 32) - 30, asked), NAV_OUT, "nav")
    assert (full["status"] == 5).any() and (full["counted"] > 0).any() and full["x"][BAD_AT] == -1  # 5: SE_PLAN_STUCK
    nav.close()
    env.close()
