"""VecMCTSAgent: the reference's MCTSAgent (agents/mcts.py) for the N envs of a VecEnv.

One se_mcts_choose launch runs choose_action (:240-292) for every env: num_simulations
sequential simulations per env on a private copy of its state (UCB1 selection, one expansion,
a random rollout, backpropagation), then best_child(c_param=0). The env's state is only read.
With a VecNavigator the rollout is the navigator's instead of the random policy's
(se_mcts_choose_nav, an extension: the tree stays the reference's).
Nothing here falls back to the host: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _native as N
from ._native import _ptr

# se_mcts_choose statuses (include/shipenv.h SE_MCTS_*); STUCK from se_mcts_choose_nav alone
OK, CUT, RAISED, NEVER_RETURNS = N.MCTS_OK, N.MCTS_CUT, N.MCTS_RAISED, N.MCTS_NEVER_RETURNS
STUCK = N.MCTS_STUCK

# Every node of every env's search tree, [n, simulations + 1] device tensors in creation order
# (node 0 the root: parent -1, no action); count [n] = nodes written per env.
MCTSTree = namedtuple("MCTSTree", "parent type a b visits total_reward count")


class VecMCTSAgent:
    """MCTSAgent(env, num_simulations, exploration_param, max_rollout_steps) with the
    reference's defaults (utils/constants.py:49-53). max_attempts bounds the reference's
    unbounded retry of raising rollout steps (default 8 * max_rollout_steps, as
    VecEnv.rollout); a rollout it cuts is reported as status CUT.

    Simulation s of env i of call k draws from Philox(seed, id) with
    id = mcts_base + (env_id_base + i) * num_simulations + s; mcts_base advances by
    stride * num_simulations per call. stride defaults to env.n: in a sharded run set it to
    the global number of envs, so that the ids of all shards and calls stay disjoint.

    navigator: a VecNavigator of the same env. Every playout is then the navigator's policy
    (its refuel_below, the derived default included, and its load) for max_rollout_steps
    positions on the simulation's ship, drawn as VecNavigator.rollout draws for the simulation's
    id; max_attempts is ignored in that mode (there is nothing to retry), CUT does not occur, and
    a decision one of whose playouts ended where the navigator had no action has status STUCK.
    A navigator whose tables were made for other ports (env.set_ports) is rebuilt first, as in
    its own calls. With navigator=None nothing changes."""

    def __init__(self, env, num_simulations=50, exploration_param=1.4, max_rollout_steps=100,
                 max_attempts=None, navigator=None):
        if navigator is not None and navigator.env is not env:
            raise ValueError("the navigator was made on another env")
        self.env = env
        self.navigator = navigator
        self.num_simulations = int(num_simulations)
        self.exploration_param = float(exploration_param)
        self.max_rollout_steps = int(max_rollout_steps)
        self.max_attempts = 8 * self.max_rollout_steps if max_attempts is None else int(max_attempts)
        self.mcts_base = 0
        self.stride = env.n
        self.calls = 0  # decisions made: the t of step()'s sample_actions draw
        self._h = C.c_void_p()
        with torch.cuda.device(env.device):
            N.check(N.lib().se_mcts_create(C.byref(self._h), env._h, self.num_simulations))
        self._out = tuple(torch.zeros(env.n, dtype=torch.int32, device=env.device) for _ in range(4))

    def choose_action(self, return_tree=False):
        """-> (type, a, b, status) int32 device tensors, the typed actions of step_typed;
        with return_tree=True also an MCTSTree. The four tensors are reused by the next call.
        Where status is RAISED or NEVER_RETURNS the type is the negative SAMPLE_* code.
        Status STUCK (navigator playouts alone) still comes with the chosen action."""
        env, S = self.env, self.num_simulations
        ty, a, b, status = self._out
        raw = cnt = None
        if return_tree:
            raw = torch.zeros((env.n, S + 1, 8), dtype=torch.int32, device=env.device)  # se_mcts_node
            cnt = torch.zeros(env.n, dtype=torch.int32, device=env.device)
        tail = (self.mcts_base, _ptr(ty), _ptr(a), _ptr(b), _ptr(status), _ptr(raw), _ptr(cnt), env._stream())
        nav = self.navigator
        if nav is None:
            N.check(N.lib().se_mcts_choose(self._h, S, self.exploration_param, self.max_rollout_steps,
                                           self.max_attempts, *tail))
        else:  # through the navigator's call: a stale handle is rebuilt and asked once more
            nav._call(lambda h, *args: N.lib().se_mcts_choose_nav(self._h, h, *args), nav.refuel_below,
                      nav.load, S, self.exploration_param, self.max_rollout_steps, *tail)
        self.mcts_base += self.stride * S
        self.calls += 1
        if not return_tree:
            return ty, a, b, status
        total = raw[:, :, 6:8].contiguous().view(torch.float64).reshape(env.n, S + 1)
        tree = MCTSTree(raw[:, :, 0], raw[:, :, 1], raw[:, :, 2], raw[:, :, 3], raw[:, :, 4], total, cnt)
        return ty, a, b, status, tree

    def step(self):
        """One iteration of train's inner loop (:342-354): choose, step, and where the step
        raised (or the choice itself did) one sample_action and a second step. Returns
        (reward, done, err) of the step that counted as new tensors; err != 0 where the second
        step raised too (the reference's `continue`). Always two step_typed calls: the envs
        whose first step went through take a no-op (category 0, which raises and leaves the
        state untouched) in the second. Episode bookkeeping stays with the caller."""
        env = self.env
        ty, a, b, _ = self.choose_action()
        reward, done, err = (t.clone() for t in env.step_typed(ty, a, b))
        failed = err != 0
        sty, sa, sb = env.sample_actions(self.calls - 1)
        zero = torch.zeros_like(sty)
        r2, d2, e2 = env.step_typed(torch.where(failed, sty, zero), torch.where(failed, sa, zero),
                                    torch.where(failed, sb, zero))
        return torch.where(failed, r2, reward), torch.where(failed, d2, done), torch.where(failed, e2, err)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            torch.cuda.synchronize(self.env.device)
            N.lib().se_mcts_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
