"""bench.py's headline leg and its --dump-outputs files, on a small batch.

The leg (run_config with step_seq: reset, pre-roll, warm-up, K timed steps issued by
VecEnv.step_seq) must leave what the same sequence of VecEnv.step calls leaves, also when
the run is longer than the resident action table and goes round it, and the dump must hold
exactly that, identically from run to run."""
import argparse
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, SEED, PREROLL = 5004, 2026, 40  # no multiple of a wave or a block; 16-byte rows in the table


@pytest.fixture(scope="module")
def bench():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from shippingenv_amd import build

    build.build(verbose=False)
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def expected(steps, warmup, rows):
    """The leg's sequence through VecEnv.step: pre-roll rows t = 10^6 + k, then warm-up rows
    0 .. W - 1 and timed rows W .. W + K - 1, each taken modulo the table's `rows`."""
    from shippingenv_amd.vec import VecEnv

    env = VecEnv(N, seed=SEED)
    env.reset()
    for t in range(PREROLL):
        env.step(env.gen_actions(1_000_000 + t))
    for k in list(range(warmup)) + list(range(warmup, warmup + steps)):
        env.step(env.gen_actions(k % rows))
    torch.cuda.synchronize()
    out = {f: getattr(env, f).cpu().numpy() for f in
           ("reward", "done", "err", "x", "y", "origin", "dest", "cargo", "fuel")}
    env.close()
    return out


@pytest.mark.parametrize("table_rows", [None, 7])  # the whole run resident; 26 steps round 7 rows
def test_headline_leg_dump_is_what_step_calls_leave(bench, tmp_path, monkeypatch, table_rows):
    steps, warmup = 23, 3
    if table_rows:
        monkeypatch.setattr(bench, "ACTION_TABLE_BYTES", table_rows * N * 4)
    args = argparse.Namespace(steps=steps, warmup=warmup, seed=SEED)
    dist = bench.Dist(1)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        wall, k_ms, _, _ = bench.run_config(N, None, False, args, dist, "test", preroll=PREROLL,
                                            step_seq=True, dump=d)
        assert wall > 0 and k_ms > 0
    want = expected(steps, warmup, table_rows or steps + warmup)
    assert sorted(os.listdir(dirs[0])) == sorted(f"{name}.npy" for name, _ in bench.DUMP_FIELDS)
    for name, dtype in bench.DUMP_FIELDS:
        a, b = (np.load(os.path.join(d, f"{name}.npy")) for d in dirs)
        assert a.dtype == np.dtype(dtype) and a.shape == (N,), name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name  # run to run, bit for bit
        assert np.array_equal(a, want[name].astype(dtype)), name
        assert np.array_equal(a.astype(want[name].dtype), want[name]), name  # nothing lost in the cast
    assert np.any(np.load(os.path.join(dirs[0], "fuel.npy")) > 0)  # a stepped state, not an empty one
