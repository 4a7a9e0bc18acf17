"""The sparse SARSA table of include/shipenv.h restated in plain Python, for the tests of
se_sarsa_create_sparse / VecSARSAAgent(table="sparse").

The table is an open-addressing hash table of rows: keys[s] is -1 (empty) or a row number of
the dense layout, pages[s] the row's A doubles in the dense slot order. The home bucket of a
row is mix(row) & (capacity - 1) with the splitmix64 finaliser, probing is linear with step 1
and wraps, nothing is ever deleted: a lookup ends at the row or at the first empty slot, and
after at most `capacity` slots. A row that is absent reads as zeros, so a table is a map
{entry: value bits} of its non-zero entries, and two tables are equal when their maps are:
where a row landed is not part of the contract.

Table is the sequential restatement (find, find_or_insert); check_valid holds a (keys, pages)
pair read back from the device to the invariants; as_map converts it; TrackingLearner is
sarsa_support.Learner counting what the sparse tests assert about a run (the distinct rows
written, and the steps in which several envs wrote one row that was new).
"""
import numpy as np

import sarsa_support as SS

M64 = (1 << 64) - 1
EMPTY = -1


def mix(z):
    """The splitmix64 finaliser on a 64-bit word."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def home(row, capacity):
    assert capacity >= 64 and capacity & (capacity - 1) == 0
    return mix(row) & (capacity - 1)


def pow2_at_least(v):
    c = 64
    while c < v:
        c *= 2
    return c


class Table:
    """The sequential table: keys int64[capacity], pages f64[capacity, A], used."""

    def __init__(self, capacity, A):
        assert capacity >= 64 and capacity & (capacity - 1) == 0
        self.capacity, self.A = capacity, A
        self.keys = np.full(capacity, EMPTY, np.int64)
        self.pages = np.zeros((capacity, A), np.float64)
        self.used = 0

    def find(self, row):
        """The row's slot, -1 where the table does not hold it."""
        s = home(row, self.capacity)
        for _ in range(self.capacity):
            k = int(self.keys[s])
            if k == row:
                return s
            if k == EMPTY:
                return -1
            s = (s + 1) & (self.capacity - 1)
        return -1

    def find_or_insert(self, row):
        """The row's slot, taking the first empty one of its probe; -1 where the table is full."""
        s = home(row, self.capacity)
        for _ in range(self.capacity):
            k = int(self.keys[s])
            if k == row:
                return s
            if k == EMPTY:
                self.keys[s] = row
                self.used += 1
                return s
            s = (s + 1) & (self.capacity - 1)
        return -1

    def get(self, row, slot):
        s = self.find(row)
        return 0.0 if s < 0 else float(self.pages[s, slot])

    def set(self, row, slot, value):
        s = self.find_or_insert(row)
        if s < 0:
            return False
        self.pages[s, slot] = value
        return True


def check_valid(keys, pages, rows, used=None):
    """The invariants of a (keys, pages) pair: the keys distinct and in [0, rows) or empty; every
    key reachable from its home before an empty slot; unoccupied pages all zero bits; `used`
    (when given) the occupied count. -> the occupied count."""
    keys = np.asarray(keys, np.int64).reshape(-1)
    cap = len(keys)
    assert cap >= 64 and cap & (cap - 1) == 0, f"capacity {cap}"
    pages = np.asarray(pages, np.float64).reshape(cap, -1)
    occ = keys != EMPTY
    held = keys[occ]
    assert ((held >= 0) & (held < rows)).all(), f"keys outside [0, {rows}): {held[(held < 0) | (held >= rows)][:4]}"
    assert len(np.unique(held)) == len(held), "a row is held twice"
    for s in np.flatnonzero(occ).tolist():
        p = home(int(keys[s]), cap)
        while p != s:
            assert keys[p] != EMPTY, f"row {int(keys[s])} at slot {s} lies behind the empty slot {p} of its probe"
            p = (p + 1) & (cap - 1)
    idle = pages[~occ].view(np.uint64)
    assert not idle.any(), f"{int(np.count_nonzero(idle))} non-zero words in pages without a key"
    count = int(occ.sum())
    if used is not None:
        assert used == count, f"used {used}, occupied {count}"
    return count


def as_map(keys, pages):
    """A valid table as {entry: value bits} over its entries with non-zero bits (entry = row * A + slot)."""
    keys = np.asarray(keys, np.int64).reshape(-1)
    pages = np.ascontiguousarray(pages, np.float64).reshape(len(keys), -1)
    A = pages.shape[1]
    word = pages.view(np.uint64)
    s, k = np.nonzero(word)
    assert (keys[s] != EMPTY).all()
    return dict(zip((keys[s] * A + k).tolist(), word[s, k].tolist()))


def dense_map(flat):
    """A flat dense table as the same map."""
    word = np.ascontiguousarray(flat, np.float64).reshape(-1).view(np.uint64)
    e = np.flatnonzero(word)
    return dict(zip(e.tolist(), word[e].tolist()))


def learner_map(learner, layout):
    """The restatement's table (its dict over its optional dense start) as the same map."""
    m = {} if learner.dense is None else dense_map(learner.dense)
    for key, v in learner.q.items():
        e, b = layout.entry(key), int(np.float64(v).view(np.uint64))
        if b:
            m[e] = b
        else:
            m.pop(e, None)
    return m


def from_dense(flat, A, capacity, first=()):
    """A valid table holding every row of the flat dense table that has a non-zero word,
    inserted in row order after the rows of `first` (which are inserted whatever they hold)."""
    q = np.ascontiguousarray(flat, np.float64).reshape(-1, A)
    t = Table(capacity, A)
    held, ahead = np.flatnonzero(q.view(np.uint64).any(1)).tolist(), set(first)
    for row in list(first) + [r for r in held if r not in ahead]:
        s = t.find_or_insert(row)
        assert s >= 0, "the table is too small for the dense image"
        t.pages[s] = q[row]
    return t


class TrackingLearner(SS.Learner):
    """sarsa_support.Learner that also counts, per run: rows_written, the distinct rows any env's
    update went to (the winners' and the losers'); shared_inserts, the vector steps in which more
    than one env wrote one row the table did not hold before that step; first_step_rows, the
    distinct rows of the first learning step. `held` starts as the rows a preloaded table holds."""

    def __init__(self, world, held=(), **kw):
        super().__init__(world, **kw)
        self.lay = SS.Layout(world)
        self.held = set(held)
        self.rows_written = set()
        self.shared_inserts = 0
        self.first_step_rows = None

    def vector_step(self, envs, eps, learn, driver, t):
        outs, writes, by_row = [], {}, {}
        for i, env in enumerate(envs):
            driver.begin(i, t)
            out, write = self._one(env, eps, learn, driver)
            outs.append(out)
            if write is not None:
                row = self.lay.entry(write[0]) // self.lay.A
                by_row[row] = by_row.get(row, 0) + 1
                if write[0] in writes:
                    self.collisions += 1  # a lower index came first
                else:
                    writes[write[0]] = write[1]
        self.q.update(writes)  # after every read of this step
        if any(c > 1 for row, c in by_row.items() if row not in self.held):
            self.shared_inserts += 1
        if learn and self.first_step_rows is None:
            self.first_step_rows = set(by_row)
        self.held |= set(by_row)
        self.rows_written |= set(by_row)
        return outs
