"""VecSARSAAgent: the reference's SARSAAgent (agents/sarsa.py) for the N envs of a VecEnv.

One learner owns one f64 Q-table in device memory, dense (every row of the layout) or sparse (a
hash table of the rows met, for worlds whose dense table does not fit); every se_sarsa_step runs the body of
train's inner loop (:255-272) for all envs at once: _try_action on the pending action,
choose_action on the new state, the update, and the restart of finished episodes. All envs
read the table as the previous vector step left it; where several update one entry in a step,
the lowest env index wins (include/shipenv.h, DESIGN.md "Tabular SARSA"). With one env, or
without collisions, it is the reference's learner step for step.
Nothing here falls back to the host: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native as N
from ._native import _ptr

# se_sarsa_step statuses (include/shipenv.h SE_SARSA_*)
OK, CUT, RAISED, NEVER_RETURNS = N.SARSA_OK, N.SARSA_CUT, N.SARSA_RAISED, N.SARSA_NEVER_RETURNS

MOVE, SELECT, TAKE_FUEL, TAKE_CARGO = 1, 2, 3, 4
MOVES = ((0, -1), (0, 1), (-1, 0), (1, 0))  # _get_possible_actions' order (:105-110)
# fuel class -> (cargo_bucket, fuel_bucket) of discretize_state, both read from the fuel
BUCKETS = ((0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (4, 3), (4, 4))


class TableRollout(NamedTuple):
    """What VecSARSAAgent.rollout returns: device tensors of m entries (the ship's six are None
    without return_end, the action rows None without return_actions)."""
    ret: torch.Tensor           # f64: the counted steps' rewards summed in order
    counted: torch.Tensor       # counted steps
    status: torch.Tensor        # PLAN_DONE / PLAN_END / PLAN_BAD_SRC / PLAN_STUCK
    stuck_at: torch.Tensor      # the position whose sample_action raised, -1 if none did
    sample_type: torch.Tensor   # its SAMPLE_* type (status PLAN_STUCK), else 0
    raised: torch.Tensor        # raising steps
    first_err: torch.Tensor     # ERR_* of the first raising step, 0 if none
    first_err_at: torch.Tensor  # its position, -1 if none
    x: Optional[torch.Tensor] = None
    y: Optional[torch.Tensor] = None
    fuel: Optional[torch.Tensor] = None
    cargo: Optional[torch.Tensor] = None
    origin: Optional[torch.Tensor] = None
    dest: Optional[torch.Tensor] = None
    act_type: Optional[torch.Tensor] = None  # [steps, m] views of rows rollout_plan takes as they
    act_a: Optional[torch.Tensor] = None     # are: the action of every position played, type 0
    act_b: Optional[torch.Tensor] = None     # behind the end


def sparse_home(rows, capacity):
    """The sparse table's home buckets of an int64 array of rows (include/shipenv.h: the
    splitmix64 finaliser masked to the capacity), as se_sarsa_sparse_home gives them one by one."""
    z = np.asarray(rows, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z & np.uint64(capacity - 1)).astype(np.int64)


def sparse_image(rows, pages, capacity):
    """(keys int64[capacity], pages f64[capacity, A]) on the host holding the distinct `rows` with
    their `pages`: every row in the first empty slot of its probe."""
    rows = np.asarray(rows, np.int64)
    pages = np.asarray(pages, np.float64).reshape(len(rows), -1)
    if len(rows) > capacity:
        raise ValueError(f"{len(rows)} rows do not fit a sparse table of capacity {capacity}")
    keys = np.full(capacity, -1, np.int64)
    out = np.zeros((capacity, pages.shape[1]), np.float64)
    pos, todo = sparse_home(rows, capacity), np.arange(len(rows))
    while todo.size:
        at = pos[todo]
        free = keys[at] < 0
        slots, first = np.unique(at[free], return_index=True)  # one taker per empty slot
        took = todo[free][first]
        keys[slots] = rows[took]
        out[slots] = pages[took]
        placed = np.zeros(len(rows), bool)
        placed[took] = True
        todo = todo[~placed[todo]]
        pos[todo] = (pos[todo] + 1) & (capacity - 1)
    return keys, out


def _pow2_at_least(v):
    c = 64
    while c < v:
        c *= 2
    return c


class VecSARSAAgent:
    """SARSAAgent(env, learning_rate, discount_factor, epsilon, epsilon_min, epsilon_decay) with
    the reference's defaults (utils/constants.py:40-46). max_steps restarts an episode after
    that many counted steps (ours: a greedy policy can repeat a legal SELECT forever; 0: never);
    max_attempts (1..64) bounds _try_action's unbounded retry, a step it cuts has status CUT.
    max_table_bytes refuses a table (with its claim words, 12 bytes per entry) beyond it.

    table="sparse" keeps a hash table of rows instead (include/shipenv.h): keys int64[capacity] and
    pages f64[capacity, A], a page per state some update met, `capacity` a power of two >= 64 (the
    default: the smallest one >= max(64, 4 n)); max_table_bytes then bounds capacity * (A * 12 + 8).
    It computes what the dense table does, bit for bit, in worlds of any port count. train grows it;
    a caller who steps it by hand calls reserve() or watches stats() and calls grow(): an update
    that finds the table full is dropped and counted in stats()["dropped"].

    The envs must have been reset (env.reset()) or loaded before the first step; every env starts
    fresh, that is, its first step chooses its action first. q is the table, a torch f64 tensor
    [rows, A] in the layout of include/shipenv.h (sparse: keys and pages); t, the vector-step
    number, selects the draws."""

    def __init__(self, env, learning_rate=0.1, discount_factor=0.9, epsilon=1.0, epsilon_min=0.0001,
                 epsilon_decay=0.999, max_steps=1000, max_attempts=8, max_table_bytes=None, table="dense",
                 capacity=None):
        if table not in ("dense", "sparse"):
            raise ValueError(f"table must be 'dense' or 'sparse', not {table!r}")
        if table == "dense" and capacity is not None:
            raise ValueError("capacity belongs to table='sparse'")
        self.table = table
        self.env = env
        self.lr, self.gamma = float(learning_rate), float(discount_factor)
        self.epsilon, self.epsilon_min, self.epsilon_decay = float(epsilon), float(epsilon_min), float(epsilon_decay)
        self.max_steps, self.max_attempts = int(max_steps), int(max_attempts)
        self.t = 0
        self._carry = 0  # finished episodes not yet paid for with a decay (train)
        self._h = C.c_void_p()
        limit = (1 << 63) - 1 if max_table_bytes is None else int(max_table_bytes)
        self._limit = limit
        dev, n = env.device, env.n
        if table == "sparse":
            self.capacity = _pow2_at_least(max(64, 4 * n)) if capacity is None else int(capacity)
            # A = P + 4 + cmax + 20 (include/shipenv.h), known before the handle allocates its claim words
            self._refuse_beyond_limit(self.capacity, env.P + 24 + max([20] + [int(c) for c in env.port_cargo]))
        with torch.cuda.device(env.device):
            if table == "sparse":
                N.check(N.lib().se_sarsa_create_sparse(C.byref(self._h), env._h, self.capacity))
            else:
                N.check(N.lib().se_sarsa_create(C.byref(self._h), env._h, limit))
        rows, A, cmax = C.c_int64(), C.c_int32(), C.c_int32()
        N.check(N.lib().se_sarsa_layout(self._h, C.byref(rows), C.byref(A), C.byref(cmax)))
        self.rows, self.A, self.cmax = rows.value, A.value, cmax.value
        if table == "sparse":
            assert self.A == env.P + 24 + max([20] + [int(c) for c in env.port_cargo]), "A is not the header's"
            self.keys, self.pages = self._empty(self.capacity)
        else:
            self.q = torch.zeros((self.rows, self.A), dtype=torch.float64, device=dev)
        self.type, self.a, self.b = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        self.fresh = torch.ones(n, dtype=torch.uint8, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.reward = torch.zeros(n, dtype=torch.float64, device=dev)
        self.ended = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.fin_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.fin_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self._bind()

    def _bind(self):
        self._state = N.SeSarsaState(*[t.data_ptr() for t in (self.type, self.a, self.b, self.fresh, self.ep_len,
                                                              self.ep_return)])
        if self.table == "sparse":
            torch.cuda.synchronize(self.env.device)  # the bind counts the keys: whatever wrote them has finished
            with torch.cuda.device(self.env.device):
                N.check(N.lib().se_sarsa_bind_sparse(self._h, _ptr(self.keys), _ptr(self.pages), C.byref(self._state)))
        else:
            N.check(N.lib().se_sarsa_bind(self._h, _ptr(self.q), C.byref(self._state)))

    # ------------------------------------------------------------------ the sparse table
    def _sparse_only(self, what):
        if self.table != "sparse":
            raise ValueError(f"{what} belongs to table='sparse'")

    def _refuse_beyond_limit(self, capacity, A=None):
        need = capacity * ((self.A if A is None else A) * 12 + 8)
        if need > self._limit:
            raise ValueError(f"a sparse SARSA table of capacity {capacity} with its claim words needs {need} bytes, "
                             f"more than max_table_bytes ({self._limit})")

    def _empty(self, capacity):
        dev = self.env.device
        return (torch.full((capacity,), -1, dtype=torch.int64, device=dev),
                torch.zeros((capacity, self.A), dtype=torch.float64, device=dev))

    def stats(self):
        """The table's size: dense {"table", "rows", "bytes"}; sparse {"table", "capacity", "used",
        "dropped", "bytes"}: the pages taken and the updates lost to a full table since the agent was
        made (0 unless the table was stepped when full), after a synchronisation of the stream. bytes
        counts the table and the claim words."""
        if self.table != "sparse":
            return {"table": "dense", "rows": self.rows, "bytes": self.rows * self.A * 12}
        cap, used, dropped = C.c_int64(), C.c_int64(), C.c_int64()
        N.check(N.lib().se_sarsa_sparse_stats(self._h, C.byref(cap), C.byref(used), C.byref(dropped), self.env._stream()))
        return {"table": "sparse", "capacity": cap.value, "used": used.value, "dropped": dropped.value,
                "bytes": cap.value * (self.A * 12 + 8)}

    def grow(self, capacity=None):
        """Move the sparse table into new buffers of `capacity` slots (the default: twice as many);
        keys and pages are new tensors afterwards, the old ones are left as they were."""
        self._sparse_only("grow")
        capacity = 2 * self.capacity if capacity is None else int(capacity)
        self._refuse_beyond_limit(capacity)
        if capacity < 64 or capacity & (capacity - 1):
            raise ValueError("a sparse table's capacity must be a power of two >= 64")
        keys, pages = self._empty(capacity)
        with torch.cuda.device(self.env.device):
            N.check(N.lib().se_sarsa_sparse_grow(self._h, _ptr(keys), _ptr(pages), capacity, self.env._stream()))
        self.keys, self.pages, self.capacity = keys, pages, capacity

    def reserve(self, new_rows):
        """Grow (doubling) until the table has room for new_rows more rows (never more than the
        layout has) and is at most half full: what train does before every run of steps, for a
        caller who steps by hand (k steps add at most k * n rows). One synchronisation."""
        self._sparse_only("reserve")
        used = self.stats()["used"]
        want = min(self.rows, used + new_rows)
        capacity = self.capacity
        while capacity < want or 2 * used > capacity:
            capacity *= 2
        if capacity != self.capacity:
            self.grow(capacity)

    def _rows_and_pages(self):
        """The occupied slots on the host: (rows int64[m], pages f64[m, A])."""
        keys = self.keys.cpu()
        occ = torch.nonzero(keys >= 0).view(-1)
        return keys[occ].numpy(), self.pages[occ.to(self.pages.device)].cpu().numpy()

    def _install(self, rows, pages):
        """Replace the sparse table by the given rows, through the host."""
        need = _pow2_at_least(2 * len(rows))
        if need > self.capacity:
            self.grow(need)
        keys, out = sparse_image(rows, pages, self.capacity)
        self.keys.copy_(torch.from_numpy(keys))
        self.pages.copy_(torch.from_numpy(out))
        self._bind()  # counts the rows

    def to_dense(self):
        """The table as the dense [rows, A] tensor (dense: q itself); refused beyond max_table_bytes."""
        if self.table != "sparse":
            return self.q
        need = self.rows * self.A * 8
        if need > self._limit:
            raise ValueError(f"the dense SARSA table needs {need} bytes, more than max_table_bytes ({self._limit})")
        q = torch.zeros((self.rows, self.A), dtype=torch.float64, device=self.env.device)
        occ = torch.nonzero(self.keys >= 0).view(-1)
        q[self.keys[occ]] = self.pages[occ]
        return q

    # ------------------------------------------------------------------ stepping
    def step(self, learn=True, epsilon=None):
        """One vector step -> (reward f64, ended u8, status i32) device tensors, reused by the
        next call; fin_return / fin_len hold the finished episodes' totals where ended."""
        eps = self.epsilon if epsilon is None else float(epsilon)
        N.check(N.lib().se_sarsa_step(self._h, self.lr, self.gamma, eps, 1 if learn else 0, self.max_steps,
                                      self.max_attempts, self.t & 0xFFFFFFFF, _ptr(self.reward), _ptr(self.ended),
                                      _ptr(self.status), _ptr(self.fin_return), _ptr(self.fin_len),
                                      self.env._stream()))
        self.t += 1
        return self.reward, self.ended, self.status

    def choose_action(self, epsilon=None):
        """choose_action from every env's current state -> (type, a, b) int32 device tensors, the
        typed actions of step_typed; type < 0 where its sample_action raises. Draws the words a
        fresh env's first choice would at vector step t; nothing is modified."""
        eps = self.epsilon if epsilon is None else float(epsilon)
        out = tuple(torch.zeros(self.env.n, dtype=torch.int32, device=self.env.device) for _ in range(3))
        N.check(N.lib().se_sarsa_choose(self._h, eps, self.t & 0xFFFFFFFF, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                        self.env._stream()))
        return out

    def decay_epsilon(self):
        self.epsilon = max(self.epsilon_min, self.epsilon * self.epsilon_decay)  # :199

    def restart(self):
        """Reset every env and mark it fresh (the start of train or test_policy)."""
        self.env.reset()
        self.fresh.fill_(1)
        self.ep_len.zero_()
        self.ep_return.zero_()

    def train(self, steps, sync_every=64):
        """`steps` learning vector steps -> (episodes finished, the sum of their returns).

        The reference decays epsilon once per episode of its one env. Here n envs run their
        episodes side by side, so epsilon decays once per n finished episodes, counted from
        `ended` every sync_every steps (one host synchronisation each) with the remainder
        carried: each env's episodes see the reference's schedule on average. This pacing is
        ours; the reference has no counterpart for it.

        The sparse table is grown at the same synchronisations: before every run of k steps until
        it has room for the k * n rows those steps can add at most (never more than the layout's
        rows) and is no more than half full, so that no update is dropped; a table that max_table_bytes
        does not let grow that far raises (a smaller sync_every needs less room)."""
        n = max(self.env.n, 1)
        count = torch.zeros((), dtype=torch.int64, device=self.env.device)
        total = torch.zeros((), dtype=torch.float64, device=self.env.device)
        episodes, ret, done_steps = 0, 0.0, 0
        while done_steps < steps:
            k = min(int(sync_every), steps - done_steps)
            count.zero_()
            total.zero_()
            if self.table == "sparse":
                self.reserve(k * self.env.n)
            for _ in range(k):
                _, ended, _ = self.step(learn=True)
                count += ended.sum()
                total += self.fin_return.sum()  # 0 where the episode goes on
            done_steps += k
            c = int(count.item())
            episodes += c
            ret += float(total.item())
            self._carry += c
            while self._carry >= n:
                self._carry -= n
                self.decay_epsilon()
        if self.table == "sparse":
            self.reserve(0)
        return episodes, ret

    def test_policy(self, steps):
        """Greedy evaluation (test_policy :315-356: deterministic choices, no update) for `steps`
        vector steps from fresh resets -> {start port: mean return of the episodes that finished}.
        The learner's step number t advances; the table does not change.
        evaluate() values the table from the envs' current states without touching them or t."""
        env = self.env
        self.restart()
        P = env.P
        sums = torch.zeros(P, dtype=torch.float64, device=env.device)
        cnts = torch.zeros(P, dtype=torch.float64, device=env.device)
        start = env.origin.to(torch.int64).clone()
        for _ in range(int(steps)):
            _, ended, _ = self.step(learn=False, epsilon=0.0)
            fin = ended != 0
            idx = start.clamp(max=P - 1)
            sums.index_add_(0, idx, self.fin_return)  # 0 where the episode goes on
            cnts.index_add_(0, idx, fin.to(torch.float64))
            start = torch.where(fin, env.origin.to(torch.int64), start)
        s, c = sums.cpu().tolist(), cnts.cpu().tolist()
        self.restart()
        return {p: s[p] / c[p] for p in range(P) if c[p] > 0}

    # ------------------------------------------------------------------ rollouts
    def rollout(self, src=None, steps=100, epsilon=0.0, ids=None, rollout_base=0, return_end=False,
                return_actions=False):
        """Table-policy rollouts (se_rollout_sarsa): rollout r plays the table, greedy or
        epsilon-greedy, for `steps` positions on a private copy of env src[r] (int32 [m]; None:
        every env once). The envs, their counters, the table, the learner state and t are
        untouched. ids (int64 [m]) names each rollout's Philox stream instead of rollout_base + r.
        A step that raises makes the next position sample its action, as _try_action does; a
        sample_action that raises ends the rollout (PLAN_STUCK). Position k draws what
        rollout_plan's position k draws: the rollout equals rollout_plan of the actions it
        emitted (return_actions), and with epsilon = 1 env.rollout of the same base. Returns a
        TableRollout of fresh tensors."""
        env = self.env
        if src is None:
            src = torch.arange(env.n, dtype=torch.int32, device=env.device)
        elif not isinstance(src, torch.Tensor):
            src = torch.as_tensor(np.asarray(src))
        m, steps = src.numel(), int(steps)
        s = env._dev(src, torch.int32, count=m)
        idt = None if ids is None else env._dev(ids, torch.int64, count=m)
        # own: stuck_at, sample_type
        ret, (counted, status), own, noted, end, plan_out = env._episode_outputs(m, return_end, extra=2)
        acts, ld = (None, None, None), (m + 3) & ~3  # rows 16-byte aligned
        if return_actions:
            acts = tuple(torch.empty((max(steps, 0), ld), dtype=torch.int32, device=env.device) for _ in range(3))
        out = N.SeTableOut(*[t.data_ptr() for t in own], *[None if t is None else t.data_ptr() for t in acts], ld,
                           plan_out)
        N.check(N.lib().se_rollout_sarsa(self._h, float(epsilon), _ptr(s), m, _ptr(idt), int(rollout_base), steps,
                                         _ptr(ret), _ptr(counted), _ptr(status), C.byref(out), env._stream()))
        self._keep = (s, idt)
        return TableRollout(ret, counted, status, *own, *noted, *end, *[None if t is None else t[:, :m] for t in acts])

    def evaluate(self, steps=100, ids=None, rollout_base=0):
        """What the table is worth from where the envs stand -> {start port: mean ret of the greedy
        (epsilon = 0) rollouts of `steps` positions from the envs whose current origin is that
        port}; envs without an origin are left out. One launch, the means on the device and one
        host read; the envs, t and the table are untouched, so it may run in the middle of
        training, and under the same ids it is comparable draw for draw with
        VecNavigator.rollout and, at epsilon = 1, env.rollout."""
        env, P = self.env, self.env.P
        ret = self.rollout(None, steps, 0.0, ids, rollout_base).ret
        origin = env.origin.to(torch.int64)
        has = (origin >= 0) & (origin < P)  # SE_NONE (255) names no port
        idx = torch.where(has, origin, torch.zeros_like(origin))
        acc = torch.zeros((2, P), dtype=torch.float64, device=env.device)
        acc[0].index_add_(0, idx, torch.where(has, ret, torch.zeros_like(ret)))
        acc[1].index_add_(0, idx, has.to(torch.float64))
        s, c = acc.cpu().tolist()
        return {p: s[p] / c[p] for p in range(P) if c[p] > 0}

    # ------------------------------------------------------------------ the table
    def entry_key(self, entry):
        """Flat table entry -> the reference's dict key
        (((x, y), cargo_bucket, fuel_bucket, prev, dest), (type, value))."""
        P, A, W = self.env.P, self.A, self.env.W
        row, slot = divmod(int(entry), A)
        row, dest = divmod(row, P + 1)
        row, origin = divmod(row, P + 1)
        cell, cls = divmod(row, 7)
        x, y = divmod(cell, W)
        cb, fb = BUCKETS[cls]
        if slot < P:
            action = (SELECT, slot)
        elif slot < P + 4:
            action = (MOVE, MOVES[slot - P])
        elif slot < P + 4 + self.cmax:
            action = (TAKE_CARGO, slot - (P + 3))
        else:
            action = (TAKE_FUEL, slot - (P + 3 + self.cmax))
        return ((x, y), cb, fb, origin - 1, dest - 1), action

    def q_items(self):
        """The non-zero entries as {reference dict key: value}."""
        if self.table == "sparse":
            rows, pages = self._rows_and_pages()
            s, k = np.nonzero(pages)
            return {self.entry_key(e): v for e, v in zip((rows[s] * self.A + k).tolist(), pages[s, k].tolist())}
        flat = self.q.view(-1)
        idx = torch.nonzero(flat, as_tuple=False).view(-1)
        vals = flat[idx].cpu().tolist()
        return {self.entry_key(e): v for e, v in zip(idx.cpu().tolist(), vals)}

    def save(self, path):
        doc = {"epsilon": self.epsilon, "lr": self.lr, "gamma": self.gamma, "layout": (self.rows, self.A, self.cmax),
               "table": self.table}
        if self.table == "sparse":  # the rows held and their pages: where they lay is not part of the table
            rows, pages = self._rows_and_pages()
            doc["rows"], doc["pages"] = torch.from_numpy(rows), torch.from_numpy(pages)
        else:
            doc["q"] = self.q.cpu()
        torch.save(doc, path)

    def load(self, path):
        data = torch.load(path, map_location="cpu")
        if tuple(data["layout"]) != (self.rows, self.A, self.cmax):
            raise ValueError(f"the saved table's layout {tuple(data['layout'])} is not this world's "
                             f"{(self.rows, self.A, self.cmax)}")
        saved_sparse = data.get("table", "dense") == "sparse"  # a checkpoint of either kind loads into either
        if self.table == "sparse":
            if saved_sparse:
                rows, pages = data["rows"], data["pages"]
            else:  # the rows with a non-zero entry
                rows = torch.nonzero((data["q"] != 0).any(1)).view(-1)
                pages = data["q"][rows]
            self._install(rows.numpy(), pages.numpy())
        elif saved_sparse:
            self.q.zero_()
            self.q[data["rows"].to(self.q.device)] = data["pages"].to(self.q.device)
        else:
            self.q.copy_(data["q"])
        self.epsilon = data.get("epsilon", self.epsilon_min)  # :402-404
        self.lr = data.get("lr", self.lr)
        self.gamma = data.get("gamma", self.gamma)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            torch.cuda.synchronize(self.env.device)
            N.lib().se_sarsa_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
