"""VecNavigator: route tables, an expert policy and navigated rollouts for the N envs of a VecEnv.

An extension: the reference has no such component. The map is static and known when the env is
made, so for every port the number of moves over water from every cell to that port (the field),
and for every cell the move that goes down that field (the direction), are built once on the host
(one breadth-first pass per port) and kept on the device. With them "sail to the destination,
refuel when low" is one byte read per env and step: se_nav_actions computes the policy's action
for every env, se_rollout_nav plays it on private copies of envs as rollout_plan plays a plan.
include/shipenv.h states the policy and the draw contract. Nothing here falls back to the host
for the device calls: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as N
from ._native import _ptr

# se_nav_actions statuses, se_rollout_nav's statuses (include/shipenv.h SE_NAV_*, SE_PLAN_*)
OK, NO_DEST, UNREACHABLE = N.NAV_OK, N.NAV_NO_DEST, N.NAV_UNREACHABLE
DONE, END, BAD_SRC, STUCK = N.PLAN_DONE, N.PLAN_END, N.PLAN_BAD_SRC, N.PLAN_STUCK
INF, NONE = N.NAV_INF, N.NAV_NONE


class NavResult(NamedTuple):
    """What VecNavigator.rollout returns: device tensors of m entries (the ship's six are None
    without return_end)."""
    ret: torch.Tensor           # f64: the counted steps' rewards summed in order
    steps: torch.Tensor         # counted steps
    status: torch.Tensor        # PLAN_DONE / PLAN_END / PLAN_BAD_SRC / PLAN_STUCK
    arrivals: torch.Tensor      # steps that arrived at their destination
    nav_status: torch.Tensor    # NAV_OK, or why the navigator had no action (status PLAN_STUCK)
    stuck_at: torch.Tensor      # the position it had none at, -1 if it always had one
    raised: torch.Tensor        # raising steps (by the policy's construction: 0)
    first_err: torch.Tensor     # ERR_* of the first raising step, 0 if none
    first_err_at: torch.Tensor  # its position, -1 if none
    x: Optional[torch.Tensor] = None
    y: Optional[torch.Tensor] = None
    fuel: Optional[torch.Tensor] = None
    cargo: Optional[torch.Tensor] = None
    origin: Optional[torch.Tensor] = None
    dest: Optional[torch.Tensor] = None


def build_tables(water, port_x, port_y):
    """(field uint16 [P, H, W], dir uint8 [P, H, W]) of a water mask and ports, built on the host
    by the library (se_nav_build_host: no device). field is the least number of moves over
    non-ground cells to the port (INF where there is none), dir the move 0..3 = N, E, S, W of
    the agent index that goes down it (NONE where no neighbour has a finite value)."""
    water = np.ascontiguousarray(water, np.uint8)
    H, W = water.shape
    px, py = np.ascontiguousarray(port_x, np.int32), np.ascontiguousarray(port_y, np.int32)
    P = len(px)
    field = np.empty((P, H, W), np.uint16)
    dirs = np.empty((P, H, W), np.uint8)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(N.lib().se_nav_build_host(H, W, as_p(water), P, as_p(px), as_p(py), as_p(field), as_p(dirs)))
    return field, dirs


class VecNavigator:
    """VecNavigator(env, refuel_below=None, load=0): the expert policy on env's world.

    The policy, per env: without a destination in port, select the nearest other reachable port;
    in port with fuel < refuel_below, take the port's whole fuel stock; in port with no cargo
    and load > 0, take min(load, stock) cargo; otherwise move down the destination's field.

    refuel_below=None means 1.1 * (max_leg + 1), max_leg being the largest number of moves
    between two ports. A move of one cell costs 1 + uniform(-0.1, 0.1), at most 1.1 fuel, and a
    move is refused (the episode ends) only when the fuel is below its cost. A ship that leaves a
    port with at least 1.1 * (max_leg + 1) fuel still holds at least 1.1 after max_leg moves, so
    none of the at most max_leg moves to any reachable port is refused, with one move to spare.
    The value is derived, not tuned.

    A call that finds the tables made for other ports (env.set_ports has run since) rebuilds
    them first: the library's stale-handle status never reaches the caller."""

    def __init__(self, env, refuel_below=None, load=0):
        if int(load) < 0:
            raise ValueError("load must be >= 0")
        self.env = env
        self.load = int(load)
        self._refuel_below = None if refuel_below is None else float(refuel_below)
        self._h = C.c_void_p()
        with torch.cuda.device(env.device):
            N.check(N.lib().se_nav_create(C.byref(self._h), env._h))
        self._host = None
        self._out = tuple(torch.zeros(env.n, dtype=torch.int32, device=env.device) for _ in range(6))

    # ------------------------------------------------------------------ the tables
    def _call(self, fn, *args):
        """fn(handle, *args); a handle made for other ports (SE_ESTATE after env.set_ports) is
        rebuilt and asked once more."""
        rc = fn(self._h, *args)
        if rc == -3:  # SE_ESTATE
            self.rebuild()
            rc = fn(self._h, *args)
        return N.check(rc)

    def rebuild(self):
        """Build and upload the tables for the env's current world (after env.set_ports).
        Synchronises the device."""
        with torch.cuda.device(self.env.device):
            N.check(N.lib().se_nav_rebuild(self._h))
        self._host = None

    @property
    def max_leg(self):
        """The largest number of moves between two ports that can reach each other, 0 if none."""
        leg = C.c_int32()
        self._call(N.lib().se_nav_tables, None, None, C.byref(leg))
        return leg.value

    @property
    def refuel_below(self):
        return 1.1 * (self.max_leg + 1) if self._refuel_below is None else self._refuel_below

    def _tables(self):
        self._call(N.lib().se_nav_tables, None, None, None)  # a stale handle is rebuilt: the copy goes with it
        if self._host is None:
            self._host = build_tables(self.env.water, self.env.port_x, self.env.port_y)
        return self._host

    def fields(self):
        """numpy uint16 [P, H, W]: moves to each port, INF where there is no way."""
        return self._tables()[0]

    def directions(self):
        """numpy uint8 [P, H, W]: the move 0..3 = N, E, S, W towards each port, NONE where none."""
        return self._tables()[1]

    # ------------------------------------------------------------------ the policy
    def actions(self, agent=False, dist=False):
        """-> (type, a, b, status[, agent][, dist]) int32 device tensors reused by the next
        call: step_typed's actions, status NAV_OK / NAV_NO_DEST / NAV_UNREACHABLE (the action is
        then (0, 0, 0), a no-op for step_typed); agent: step's index of the action, -1 where
        there is none; dist: moves to the destination, -1 where there is none."""
        ty, a, b, status, ag, ds = self._out
        self._call(N.lib().se_nav_actions, self.refuel_below, self.load, _ptr(ty), _ptr(a), _ptr(b),
                   _ptr(status), _ptr(ag if agent else None), _ptr(ds if dist else None), self.env._stream())
        return (ty, a, b, status) + ((ag,) if agent else ()) + ((ds,) if dist else ())

    def distance(self):
        """Moves from every env's ship to its destination as an int32 device tensor (reused by
        the next call), -1 where it has none or cannot reach it."""
        return self.actions(dist=True)[4]

    def step(self):
        """actions() and env.step_typed on them -> (reward, done, err, status). Where status is
        not NAV_OK the env took the no-op: err is ERR_BAD_CATEGORY and its state is untouched."""
        ty, a, b, status = self.actions()
        reward, done, err = self.env.step_typed(ty, a, b)
        return reward, done, err, status

    def rollout(self, src=None, steps=100, ids=None, rollout_base=0, return_end=False):
        """Navigated rollouts (se_rollout_nav): rollout r plays the policy for `steps` positions
        on a private copy of env src[r] (int32 [m]; None: every env once); env state and
        counters are untouched. ids (int64 [m]) names each rollout's Philox stream instead of
        rollout_base + r. Position k draws what rollout_plan's position k draws: the rollout
        equals rollout_plan of the actions it emitted. Returns a NavResult of fresh tensors."""
        env = self.env
        if src is None:
            src = torch.arange(env.n, dtype=torch.int32, device=env.device)
        elif not isinstance(src, torch.Tensor):
            src = torch.as_tensor(np.asarray(src))
        m = src.numel()
        s = env._dev(src, torch.int32, count=m)
        idt = None if ids is None else env._dev(ids, torch.int64, count=m)
        # own: arrivals, nav_status, stuck_at
        ret, (steps_t, status), own, noted, end, plan_out = env._episode_outputs(m, return_end, extra=3)
        out = N.SeNavOut(*[t.data_ptr() for t in own], plan_out)
        self._call(N.lib().se_rollout_nav, _ptr(s), m, int(steps), self.refuel_below, self.load, _ptr(idt),
                   int(rollout_base), _ptr(ret), _ptr(steps_t), _ptr(status), C.byref(out), env._stream())
        self._keep = (s, idt)
        return NavResult(ret, steps_t, status, *own, *noted, *end)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            torch.cuda.synchronize(self.env.device)
            N.lib().se_nav_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
